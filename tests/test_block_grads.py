"""HarDNetFeatureExtraction.train_blocks and FasterRCNNTrainer(backbone_grads=n): the gradients of the
tail plus the last n HarDBlocks against tests/pw_grads_restated.py's float64 section, fed the section's input and every layer's
saved output read back from the HIP run (``f.grad_fn.saved``), so that only the backward is under test.
The bar: |err| <= (n + 8) 2^-24 T elementwise, n summed along the deepest path."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_grads_restated import assert_within, section_reference  # noqa: E402


def seeded_backbone(dev, seed=0):
    """test_tail_grads.py's seeding, plus non-trivial BatchNorm statistics and affine terms (the folding rule needs a mean)."""
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    torch.manual_seed(seed)
    m = HarDNetFeatureExtraction(depth_wise=True, arch=39)
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


def unfreeze(m, n):
    m.train_blocks(n)
    for p in m.trainable_parameters():
        p.requires_grad_(True)
    return m


def images(seed, dev):
    return torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(seed)).to(dev)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def reference_for(m, f, gy):
    """{name: (gradient, T, n)} of the section that produced ``f``, from the node's saved tensors."""
    from two_stage_object_detection_amd import hip_ops
    sv = f.grad_fn.saved
    base = copy.deepcopy(m.base).cpu().double()
    (x0, off0), C = sv["inputs"][0], sv["C"]
    section = []
    for b in sv["blocks"]:
        blk = base[b["index"]]
        real, offs, _ = blk.slice_table()
        tr, down = b["transition"], b["down"]
        assert [lay["off"] for lay in b["layers"]] == offs[1:] and [lay["cout"] for lay in b["layers"]] == real[1:]
        section.append(dict(
            index=b["index"], block=blk, tr_index=tr["index"], transition=base[tr["index"]],
            down=None if down is None else base[down["index"]], down_index=None if down is None else down["index"],
            slices=[nchw(b["buf"][..., o:o + r]) for o, r in zip(offs, real)],
            ys=[nchw(lay["y"][..., :lay["cout"]]) for lay in b["layers"]],
            tr_y=nchw(x0[..., off0:off0 + C]) if tr["y"] is None else nchw(tr["y"][..., :tr["cout"]])))
    w1, _, sh1, _ = sv["packs"][0]
    with torch.no_grad():
        a = hip_ops.dwconv3x3_nhwc(x0, w1, None, sh1, 2, True, C=C, in_off=off0)
    i1, i2, ip = sv["tail_indices"]
    return section_reference(section, (i1, base[i1], i2, base[i2], ip, base[ip]), section[0]["slices"][0], gy.cpu(), nchw(a > 0))


def check_section(dev, n, first_name):
    m = seeded_backbone(dev)
    x = images(1, dev)
    with torch.no_grad():
        plain = m(x).clone()
    # the tail's six gradients of train_tail, for the same upstream gradient
    gy = torch.randn(plain.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    for p in m.tail_parameters():
        p.requires_grad_(True)
    m.train_tail(True)(x).backward(gy)
    tail = [p.grad.clone() for p in m.tail_parameters()]
    for p in m.tail_parameters():
        p.grad = None
    unfreeze(m, n)
    names = [k for k, _ in m._trainable_named()]
    assert names[0] == first_name
    f = m(x)
    assert f.requires_grad and torch.equal(f.detach(), plain)
    with torch.no_grad():
        assert not m(x).requires_grad
    f.backward(gy)
    ref = reference_for(m, f, gy)
    assert set(ref) == set(names)
    worst = {}
    for name, p in zip(names, m.trainable_parameters()):
        assert p.grad is not None and p.grad.shape == p.shape, name
        g, T, cnt = ref[name]
        assert_within(p.grad, g, T, cnt, name)
        kind = ".".join(name.split(".")[-2:])
        ratio = float(((p.grad.double().cpu() - g).abs() / ((cnt + 8) * 2.0 ** -24 * T).clamp_min(1e-300)).max())
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    print(f"train_blocks({n}): largest err / bar per tensor kind: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    ours = {id(p) for p in m.trainable_parameters()}
    assert all(p.grad is None for p in m.parameters() if id(p) not in ours)
    assert all(torch.equal(p.grad, t) for p, t in zip(m.tail_parameters(), tail))
    assert len({k[3:] for k in m._plans}) == 3                     # plain, train_tail, train_blocks(n): three plan kinds
    return m


@pytest.mark.gpu
def test_train_blocks_1_output_unchanged_and_gradients_match_f64(dev):
    check_section(dev, 1, "base.12.layers.0.layer1.conv.weight")


@pytest.mark.gpu
def test_train_blocks_2_covers_the_8_layer_block_and_the_dwconv_between(dev):
    m = check_section(dev, 2, "base.9.layers.0.layer1.conv.weight")
    assert m.base[11].dwconv.weight.grad is not None and m.base[9].layers[7].layer1.norm.weight.grad is not None


@pytest.mark.gpu
def test_two_forwards_then_their_backwards_in_reverse_order(dev):
    m = unfreeze(seeded_backbone(dev), 2)
    xa, xb = images(3, dev), images(4, dev)
    gen = torch.Generator().manual_seed(5)
    ga, gb = torch.randn(2, 512, 4, 6, generator=gen).to(dev), torch.randn(2, 512, 4, 6, generator=gen).to(dev)
    singles = []
    for x, gy in ((xa, ga), (xb, gb)):
        for p in m.trainable_parameters():
            p.grad = None
        m(x).backward(gy)
        singles.append([p.grad.clone() for p in m.trainable_parameters()])
    for p in m.trainable_parameters():
        p.grad = None
    fa = m(xa)
    fb = m(xb)
    fb.backward(gb)
    fa.backward(ga)
    for (name, _), p, s1, s2 in zip(m._trainable_named(), m.trainable_parameters(), *singles):
        assert torch.equal(p.grad, s2 + s1), name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["grad", "no_grad", "inference_mode", "train_blocks_0"])
def test_forward_follows_an_optimizer_step(dev, mode):
    from two_stage_object_detection_amd import optim
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    m = unfreeze(seeded_backbone(dev), 2)
    x = images(6, dev)
    with torch.no_grad():
        stale = m(x).clone()                                     # (the grad-free plan and its packs exist before the step)
    f = m(x)
    f.backward(torch.ones_like(f))
    optim.AdamW(m.trainable_parameters(), lr=1e-3).step()
    if mode == "grad":
        after = m(x).detach().clone()
    elif mode == "no_grad":
        with torch.no_grad():
            after = m(x).clone()
    elif mode == "inference_mode":
        with torch.inference_mode():
            after = m(x).clone()
    else:
        after = m.train_blocks(0)(x).detach().clone()
    fresh = HarDNetFeatureExtraction(depth_wise=True, arch=39)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(x)
    assert not torch.equal(after, stale) and torch.equal(after, want)


@pytest.mark.gpu
def test_trainer_backbone_grads_1(dev, golden_dir):
    from test_trainer_grads import PARAMS, reference_state_dict
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    z = np.load(os.path.join(golden_dir, "trainer_ref.npz"))
    x = (torch.from_numpy(z["img_u8"]).float() / 255)[None].to(dev)
    bbox, label = torch.from_numpy(z["bbox"]).to(dev), torch.from_numpy(z["label"]).to(dev)

    def trainer(**kw):
        tr = FasterRCNNTrainer("train", 80, **kw)
        tr.load_state_dict(reference_state_dict(), strict=True)
        tr = tr.to(dev).eval()
        tr.feat_extra.requires_grad_(False)
        return tr

    tr = trainer(backbone_grads=1, head_grads=True)
    ours = unfreeze(tr.feat_extra, 1).trainable_parameters()
    named = dict(tr.named_parameters())

    def step():
        for p in tr.parameters():
            p.grad = None
        losses = tr(x, [bbox], [label])[0]
        losses[-1].backward()
        assert all(named[k].grad is not None for k in PARAMS) and all(p.grad is not None and p.grad.shape == p.shape for p in ours)
        return [l.detach().clone() for l in losses], [named[k].grad.clone() for k in PARAMS] + [p.grad.clone() for p in ours]

    losses, grads = step()
    assert any(bool(g.any()) for g in grads[len(PARAMS):len(PARAMS) + 3])          # the first block layer does get a gradient
    with torch.no_grad():
        want = trainer()(x, [bbox], [label])[0]
    assert all(torch.equal(a, b) for a, b in zip(losses, want))
    losses2, grads2 = step()
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2)) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
