"""HarDNetFeatureExtraction.set_train_mode(mode, batch_stats=True, dropout=True) under .train():
HarDNet-85, ``train_blocks(1)``, two images of 64 x 96 (the last block sees 16 x 24 pixels per image, 1 252 concatenated channels).

The mask is rebuilt from ``last_dropout_key`` with tests/dropout_restated.py; the references are those of
tests/test_hardnet_bn_train.py with the ``nn.Dropout`` replaced by a multiply with that mask, and the bars are the ones that file
applies to the same quantities - dropout adds one exact multiply and gets no margin of its own.  Gradients: |err| <= (n + 8) 2^-24 T
against the float64 backward restated from the node's saved forward (bn_train_restated.bn_section_reference's graph, one block).
Feature map and running statistics: max |err| / max |ref| <= 4 x what torch's float32 CPU run of the same step shows against
the float64 one (bn_train_restated.module_oracle on a copy of ``base`` whose Dropout is the mask multiply)."""
import copy
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_train_restated as R  # noqa: E402
import dropout_restated as D  # noqa: E402
import hardnet_dropout_restated as H  # noqa: E402
from dw_grads_restated import assert_within  # noqa: E402
from test_hardnet_bn_train import BUFFERS, bn_state, nchw  # noqa: E402


def seeded85(dev, seed=0):
    """tests/test_block_grads.py's seeded_backbone for HarDNet-85."""
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    torch.manual_seed(seed)
    m = HarDNetFeatureExtraction(depth_wise=True, arch=85)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                C = mod.num_features
                mod.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(C, generator=g) + 0.5)
                mod.weight.copy_(torch.rand(C, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(C, generator=g) * 0.1 + 0.2)
    m.requires_grad_(False)
    return m.to(dev).eval()


def trainable(m, dropout=True):
    m.train_blocks(1, batch_stats=True, dropout=dropout)
    for p in m.trainable_parameters():
        p.requires_grad_(True)
    return m


def images(seed, dev):
    return torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(seed)).to(dev)


def clear(m):
    for p in m.parameters():
        p.grad = None


def seeded_forward(m, x, seed):
    m.dropout_generator = torch.Generator().manual_seed(seed)
    return m(x)


class MaskMul(torch.nn.Module):
    """The nn.Dropout of the oracle: a multiply with a fixed mask (kept: the f32 scale, dropped: 0)."""

    def __init__(self, mask):
        super().__init__()
        self.register_buffer("mask", mask)

    def forward(self, x):
        return x * self.mask


def mask_of(f, key):
    """The mask of the forward behind ``f`` as NCHW float32 [N, C, h, w] (scale where kept, 0 where dropped), from the key."""
    blk = f.grad_fn.saved["blocks"][-1]
    drop = blk["dropout"]
    N, h, w, _ = blk["buf"].shape
    assert [v & 0xFFFFFFFF for v in drop["key"].cpu().tolist()] == list(key)
    keep = D.keep_mask(N * h * w, drop["C"], drop["p"], key, drop["ordinal"])
    scale = D.params(drop["p"])[1]
    return (torch.from_numpy(keep).float() * float(scale)).view(N, h, w, drop["C"]).permute(0, 3, 1, 2).contiguous()


def saved_reference(m, f, gy, mask):
    """{name: (gradient, T, n)} of ``train_blocks(1)``'s section from the node's saved forward (test_hardnet_bn_train's
    saved_reference for one block, the transition's input multiplied by ``mask``)."""
    from two_stage_object_detection_amd import hip_ops
    sv = f.grad_fn.saved
    base = copy.deepcopy(m.base).cpu().double()
    (x0, off0), C = sv["inputs"][0], sv["C"]
    b, = sv["blocks"]
    assert b["down"] is None and sv.get("stem") is None
    blk, tr = base[b["index"]], b["transition"]
    real, offs, _ = blk.slice_table()
    section = dict(index=b["index"], block=blk, tr_index=tr["index"], transition=base[tr["index"]],
                   slices=[nchw(b["buf"][..., o:o + r]) for o, r in zip(offs, real)],
                   ys=[nchw(lay["y"][..., :lay["cout"]]) for lay in b["layers"]],
                   zs=[nchw(lay["bnt"]["z"][..., :lay["cout"]]) for lay in b["layers"]],
                   dw_zs=[nchw(lay["dw_bnt"]["z"][..., :lay["cout"]]) for lay in b["layers"]],
                   tr_y=nchw(x0[..., off0:off0 + C]), tr_z=nchw(tr["bnt"]["z"][..., :tr["cout"]]))
    w1, _, sh1, _ = sv["packs"][0]
    with torch.no_grad():
        tail_mask = nchw(hip_ops.dwconv3x3_nhwc(x0, w1, None, sh1, 2, True, C=C, in_off=off0) > 0)
    i1, i2, ip = sv["tail_indices"]
    return H.section_reference(section, (i1, base[i1], i2, base[i2], ip, base[ip]), gy.cpu(), tail_mask, mask)


def oracle(m, mask, x, gy, dtype, before):
    """bn_train_restated.module_oracle on a copy of ``base`` whose nn.Dropout is the multiply with ``mask``."""
    base = copy.deepcopy(m.base).cpu()
    idx, = [i for i, mod in enumerate(base) if isinstance(mod, torch.nn.Dropout)]
    base[idx] = MaskMul(mask)
    return R.module_oracle(types.SimpleNamespace(base=base), m._mode_start(1), x, gy, dtype, before)


@pytest.fixture(scope="module")
def step(dev):
    """One training step with active dropout, shared by the tests that only read it."""
    m = trainable(seeded85(dev)).train()
    x = images(1, dev)
    before = bn_state(m)
    torch.manual_seed(11)
    f = m(x)
    key = m.last_dropout_key
    gy = torch.randn(f.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    f.backward(gy)
    return dict(m=m, x=x, f=f, gy=gy, key=key, before=before, after=bn_state(m), mask=mask_of(f, key),
                grads={k: p.grad.clone() for (k, _), p in zip(m._trainable_named(), m.trainable_parameters())})


@pytest.mark.gpu
def test_feature_map_and_running_statistics(step):
    m, mask, before, after = step["m"], step["mask"], step["before"], step["after"]
    start = m._mode_start(1)
    drop = step["f"].grad_fn.saved["blocks"][-1]["dropout"]
    assert drop["p"] == 0.1 and drop["ordinal"] == 0 and drop["C"] == 1252 and mask.shape == (2, 1252, 16, 24)
    kept = float((mask != 0).double().mean())
    assert abs(kept - 0.9) < 4 * (0.09 / mask.numel()) ** 0.5, kept
    out64, _, b64, _ = oracle(m, mask, step["x"], step["gy"], torch.float64, before)
    out32, _, b32, _ = oracle(m, mask, step["x"], step["gy"], torch.float32, before)
    report, bad = [], []

    def check(name, got, ref, f32):
        scale = float(ref.abs().max())
        err = float((got.double().cpu() - ref.double()).abs().max()) / scale
        t32 = float((f32.double() - ref.double()).abs().max()) / scale
        report.append(f"{name} {err:.2e}/{R.MARGIN * t32:.2e}")
        if not err <= R.MARGIN * t32:
            bad.append(name)
    check("features", step["f"].detach(), out64, out32)
    moved = 0
    for k in before:
        if int(k.split(".")[1]) < start:                                  # frozen BN: not a bit
            assert torch.equal(before[k], after[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(before[k]) + 1 == int(b64[k]), k
        else:
            check(k, after[k], b64[k], b32[k])
            moved += int(not torch.equal(before[k], after[k]))
    print("err/bound " + ", ".join(report))
    assert not bad, (bad, report)
    assert moved == 2 * len(m._section_norms(start)) and all(k.endswith(BUFFERS) for k in before)
    # without the mask the oracle is somewhere else: the map really went through the dropped copy
    plain64 = R.module_oracle(m, start, step["x"], step["gy"], torch.float64, before)[0]
    assert R.norm_error(step["f"].detach(), plain64) > 100 * R.norm_error(step["f"].detach(), out64)


@pytest.mark.gpu
def test_gradients_against_the_saved_forward(step):
    m = step["m"]
    ref = saved_reference(m, step["f"], step["gy"], step["mask"])
    names = [k for k, _ in m._trainable_named()]
    assert set(ref) == set(names) == set(step["grads"])
    worst = {}
    for name, p in zip(names, m.trainable_parameters()):
        got = step["grads"][name]
        assert got.shape == p.shape, name
        g, T, cnt = ref[name]
        assert_within(got, g, T, cnt, name)
        kind = ".".join(name.split(".")[-2:])
        ratio = float(((got.double().cpu() - g).abs() / ((cnt + 8) * 2.0 ** -24 * T).clamp_min(1e-300)).max())
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    print("largest err / bar per tensor kind: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    ours = {id(p) for p in m.trainable_parameters()}
    assert all(p.grad is None for p in m.parameters() if id(p) not in ours)


@pytest.mark.gpu
def test_seeds_keys_and_interleaved_backwards(dev):
    m = trainable(seeded85(dev)).train()
    xa, xb = images(4, dev), images(5, dev)
    # the same torch.manual_seed: the same key, the same bits; the next forward draws another key
    torch.manual_seed(21)
    want = tuple(torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist())
    torch.manual_seed(21)
    f1 = m(xa).detach().clone()
    k1 = m.last_dropout_key
    f2 = m(xa).detach().clone()
    k2 = m.last_dropout_key
    torch.manual_seed(21)
    f3 = m(xa).detach().clone()
    assert k1 == want and m.last_dropout_key == k1 and k2 != k1
    assert torch.equal(f1, f3) and not torch.equal(f1, f2)
    # owner.dropout_generator takes over from the default generator, which is then left alone
    state = torch.get_rng_state()
    f4 = seeded_forward(m, xa, 21).detach().clone()
    assert m.last_dropout_key == k1 and torch.equal(f4, f1) and torch.equal(torch.get_rng_state(), state)
    # a backward issued after a later forward uses its own forward's mask
    gen = torch.Generator().manual_seed(6)
    ga, gb = torch.randn(f1.shape, generator=gen).to(dev), torch.randn(f1.shape, generator=gen).to(dev)
    singles = []
    for x, gy, seed in ((xa, ga, 31), (xb, gb, 32)):
        clear(m)
        seeded_forward(m, x, seed).backward(gy)
        singles.append([p.grad.clone() for p in m.trainable_parameters()])
    clear(m)
    fa = seeded_forward(m, xa, 31)
    ka = m.last_dropout_key
    fb = seeded_forward(m, xb, 32)
    assert m.last_dropout_key != ka
    fb.backward(gb)
    fa.backward(ga)
    for (name, _), p, s1, s2 in zip(m._trainable_named(), m.trainable_parameters(), *singles):
        assert torch.equal(p.grad, s2 + s1), name


def dropout_launches(plan):
    from two_stage_object_detection_amd._ffi import lib
    return sum(1 for fn, _ in plan.steps if fn is lib().tsod_dropout_segs_f32)


@pytest.mark.gpu
def test_paths_that_stay_as_they_were(dev):
    from test_block_grads import seeded_backbone
    x = images(3, dev)
    m = seeded85(dev)
    # .eval(): one plan, the same bits with and without the flag
    plain = trainable(m, dropout=False).eval()(x).detach().clone()
    keys = set(m._plans)
    assert torch.equal(trainable(m, dropout=True).eval()(x).detach(), plain) and set(m._plans) == keys
    assert m.last_dropout_key is None
    # dropout=False under .train(): the batch-statistics plan of before - no dropout launch, no key, nothing drawn
    state = torch.get_rng_state()
    off = trainable(m, dropout=False).train()(x).detach().clone()
    plan_off, = [p for k, p in m._plans.items() if k[-1] == "batch_stats"]
    assert dropout_launches(plan_off) == 0 and plan_off.dropout_key is None and m.last_dropout_key is None
    assert torch.equal(torch.get_rng_state(), state)
    on = trainable(m, dropout=True).train()(x).detach().clone()
    plan_on, = [p for k, p in m._plans.items() if k[-1] == "dropout"]
    assert dropout_launches(plan_on) == 1 and len(plan_on.steps) == len(plan_off.steps) + 1 and m.last_dropout_key is not None
    assert not torch.equal(on, off)
    assert torch.equal(trainable(m, dropout=False).train()(x).detach(), off)          # (and back: the same plan, the same bits)
    # HarDNet-39 has no Dropout: the flag changes neither the plan nor a bit
    a = seeded_backbone(dev)
    x39 = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(7)).to(dev)
    for dropout in (False, True):
        a.train_blocks(1, batch_stats=True, dropout=dropout)
        for p in a.trainable_parameters():
            p.requires_grad_(True)
    with_flag = a.train()(x39).detach().clone()
    plans = dict(a._plans)
    n_steps = len(next(iter(plans.values())).steps)
    a.train_blocks(1, batch_stats=True)
    assert torch.equal(a(x39).detach(), with_flag) and dict(a._plans) == plans and len(plans) == 1
    assert len(next(iter(a._plans.values())).steps) == n_steps and dropout_launches(next(iter(plans.values()))) == 0
    assert a.last_dropout_key is None
    b = seeded_backbone(dev)                                              # a module that never saw the flag
    b.train_blocks(1, batch_stats=True)
    for p in b.trainable_parameters():
        p.requires_grad_(True)
    assert torch.equal(b.train()(x39).detach(), with_flag) and list(b._plans) == list(plans)
    assert len(next(iter(b._plans.values())).steps) == n_steps


@pytest.mark.gpu
def test_trainer_step_with_dropout(dev):
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    torch.manual_seed(0)
    tr = FasterRCNNTrainer("train", 3, backbone="hardnet85", head_grads=True, backbone_grads=1, bn_batch_stats=True, dropout=True)
    tr.feat_extra.load_state_dict(seeded85("cpu").state_dict(), strict=True)
    tr = tr.to(dev).train()
    tr.requires_grad_(False)
    fe = tr.feat_extra
    for p in list(fe.train_blocks(1, batch_stats=True, dropout=True).trainable_parameters()) + tr._head_params():
        p.requires_grad_(True)
    x = images(8, dev)
    bboxes = [torch.tensor([[8.0, 10.0, 52.0, 60.0], [30.0, 20.0, 90.0, 58.0]], device=dev),      # xyxy inside 96 x 64
              torch.tensor([[4.0, 6.0, 40.0, 50.0]], device=dev)]
    labels = [torch.tensor([0, 2], device=dev), torch.tensor([1], device=dev)]
    name = f"base.{len(fe.base) - 5}.conv.weight"                         # the last transition layer
    weight = dict(fe._trainable_named())[name]

    def run(dropout, seed):
        tr.dropout = dropout
        clear(tr)
        fe.dropout_generator = torch.Generator().manual_seed(seed)
        losses = tr(x, bboxes, labels)[0]
        assert len(losses) == 5 and all(bool(torch.isfinite(l)) for l in losses)
        losses[-1].backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in fe.trainable_parameters())
        return weight.grad.clone()

    got = run(True, 41)
    key = fe.last_dropout_key
    assert fe._dropout and key is not None
    assert not torch.equal(run(False, 41), got) and not fe._dropout
    # the restated gradient: the backbone alone with the same key, fed the trainer's own d loss / d features
    tr.dropout = True
    clear(tr)
    fe.set_train_mode(1, True, True)
    feats = seeded_forward(fe, x, 41)
    assert fe.last_dropout_key == key
    leaf = feats.detach().clone().requires_grad_(True)
    tr(x, bboxes, labels, features=leaf)[0][-1].backward()
    g, T, n = saved_reference(fe, feats, leaf.grad, mask_of(feats, key))[name]
    assert_within(got, g, T, n, name)
