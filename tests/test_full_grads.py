"""HarDNetFeatureExtraction.train_full and FasterRCNNTrainer(backbone_grads="full"): the gradients of
every backbone parameter against the float64 restatements (tests/pw_grads_restated.py for the blocks and the tail,
tests/stem_grads_restated.py for the stem), fed every layer's saved output read back from the HIP run (``f.grad_fn.saved``), so
that only the backward is under test.  The bar: |err| <= (n + 8) 2^-24 T elementwise, n summed along the deepest path."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_grads_restated import assert_within, section_reference  # noqa: E402
from stem_grads_restated import STEM_NAMES, backbone_reference  # noqa: E402
from test_block_grads import images, nchw, seeded_backbone  # noqa: E402


def unfreeze_all(m):
    m.train_full()
    for p in m.trainable_parameters():
        p.requires_grad_(True)
    return m


def full_reference(m, f, gy, stem_only=False):
    """{name: (gradient, T, n)} of every backbone parameter (``stem_only``: of the nine stem tensors) for the forward that
    produced ``f``, from the node's saved tensors."""
    from two_stage_object_detection_amd import hip_ops
    sv = f.grad_fn.saved
    base = copy.deepcopy(m.base).cpu().double()
    (x0, off0), C = sv["inputs"][0], sv["C"]
    section = []
    for b in sv["blocks"]:
        blk = base[b["index"]]
        real, offs, _ = blk.slice_table()
        tr, down = b["transition"], b["down"]
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
    tail, mask, gy = (i1, base[i1], i2, base[i2], ip, base[ip]), nchw(a > 0), gy.cpu()
    st = sv["stem"]
    stem = dict(m0=base[0], m1=base[1], m2=base[2], x=nchw(st["x4"][..., :3]), y0=nchw(st["y0"]), y1=nchw(st["base1"]["y"]),
                out=section[0]["slices"][0])
    ref = {} if stem_only else section_reference(section, tail, section[0]["slices"][0], gy, mask)
    ref.update(backbone_reference(stem, section, tail, gy, mask))
    return ref


def check_gradients(m, names, params, ref, what):
    assert set(ref) == set(names)
    worst = {}
    for name, p in zip(names, params):
        assert p.grad is not None and p.grad.shape == p.shape, name
        g, T, cnt = ref[name]
        assert_within(p.grad, g, T, cnt, name)
        kind = name if name in STEM_NAMES else ".".join(name.split(".")[-2:])
        ratio = float(((p.grad.double().cpu() - g).abs() / ((cnt + 8) * 2.0 ** -24 * T).clamp_min(1e-300)).max())
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    print(f"{what}: largest err / bar, the nine stem tensors: " + ", ".join(f"{k} {worst[k]:.4f}" for k in STEM_NAMES))
    print(f"{what}: largest err / bar per tensor kind elsewhere: " +
          ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items()) if k not in STEM_NAMES))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 96), (61, 93)])
def test_train_full_output_unchanged_and_all_gradients_match_f64(dev, size):
    m = seeded_backbone(dev)
    x = images(1, dev) if size == (64, 96) else torch.rand(2, 3, *size, generator=torch.Generator().manual_seed(7)).to(dev)
    with torch.no_grad():
        plain = m(x).clone()
    gy = torch.randn(plain.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    unfreeze_all(m)
    names = [k for k, _ in m._trainable_named()]
    assert names == [k for k, _ in m.named_parameters()]
    f = m(x)
    assert f.requires_grad and torch.equal(f.detach(), plain)
    with torch.no_grad():
        assert not m(x).requires_grad
    f.backward(gy)
    check_gradients(m, names, m.trainable_parameters(), full_reference(m, f, gy), f"train_full {size}")
    # train_blocks(all) on the same model: the same gradients everywhere but in the stem, which gets none
    full = {k: p.grad.clone() for k, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    m.train_blocks(m.n_blocks)(x).backward(gy)
    for k, p in m.named_parameters():
        assert (p.grad is None) if k in STEM_NAMES else torch.equal(p.grad, full[k]), k
    assert ("train_full",) in {k[3:] for k in m._plans}


@pytest.mark.gpu
def test_two_forwards_then_their_backwards_in_reverse_order(dev):
    m = unfreeze_all(seeded_backbone(dev))
    xa, xb = images(3, dev), images(4, dev)
    gen = torch.Generator().manual_seed(5)
    ga, gb = torch.randn(2, 512, 4, 6, generator=gen).to(dev), torch.randn(2, 512, 4, 6, generator=gen).to(dev)
    singles = []
    for x, gy in ((xa, ga), (xb, gb)):
        for p in m.parameters():
            p.grad = None
        m(x).backward(gy)
        singles.append([p.grad.clone() for p in m.parameters()])
    for p in m.parameters():
        p.grad = None
    fa = m(xa)
    fb = m(xb)
    fb.backward(gb)
    fa.backward(ga)
    for (name, p), s1, s2 in zip(m.named_parameters(), *singles):
        assert torch.equal(p.grad, s2 + s1), name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["grad", "no_grad", "inference_mode", "train_tail_off"])
def test_forward_follows_an_optimizer_step_over_all_parameters(dev, mode):
    from two_stage_object_detection_amd import optim
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    m = unfreeze_all(seeded_backbone(dev))
    x = images(6, dev)
    with torch.no_grad():
        stale = m(x).clone()                                     # (the grad-free plan and its packs exist before the step)
    f = m(x)
    f.backward(torch.ones_like(f))
    before = [p.detach().clone() for p in m.base[:3].parameters()]
    optim.AdamW(list(m.parameters()), lr=1e-3).step()
    assert all(not torch.equal(a, p) for a, p in zip(before, m.base[:3].parameters()))      # the stem did move
    if mode == "grad":
        after = m(x).detach().clone()
    elif mode == "no_grad":
        with torch.no_grad():
            after = m(x).clone()
    elif mode == "inference_mode":
        with torch.inference_mode():
            after = m(x).clone()
    else:
        after = m.train_tail(False)(x).detach().clone()
    fresh = HarDNetFeatureExtraction(depth_wise=True, arch=39)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(x)
    assert not torch.equal(after, stale) and torch.equal(after, want)


@pytest.mark.gpu
def test_trainer_backbone_grads_full(dev, golden_dir):
    from test_trainer_grads import PARAMS, reference_state_dict
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    z = np.load(os.path.join(golden_dir, "trainer_ref.npz"))
    x = (torch.from_numpy(z["img_u8"]).float() / 255)[None].to(dev)
    bbox, label = torch.from_numpy(z["bbox"]).to(dev), torch.from_numpy(z["label"]).to(dev)

    def trainer(**kw):
        tr = FasterRCNNTrainer("train", 80, **kw)
        tr.load_state_dict(reference_state_dict(), strict=True)
        return tr.to(dev).eval()

    tr = trainer(backbone_grads="full", head_grads=True)
    losses = tr(x, [bbox], [label])[0]
    losses[-1].backward()
    assert all(p.grad is not None and p.grad.shape == p.shape for p in tr.parameters())
    assert all(bool(p.grad.any()) for p in tr.feat_extra.base[:3].parameters())
    plain = trainer()
    plain.feat_extra.requires_grad_(False)
    with torch.no_grad():
        want = plain(x, [bbox], [label])[0]
    assert all(torch.equal(a.detach(), b) for a, b in zip(losses, want))
    # the d feature map of the features= path for the same forward, then the stem in float64 from a node of the same forward
    with torch.no_grad():
        f = plain.feat_extra(x).clone()
    f.requires_grad_(True)
    plain(x, [bbox], [label], features=f)[0][-1].backward()
    got = {k: p.grad.clone() for k, p in tr.feat_extra.named_parameters()}
    fm = tr.feat_extra.train_full()(x)
    assert torch.equal(fm.detach(), f.detach())
    ref = full_reference(tr.feat_extra, fm, f.grad, stem_only=True)
    for name in STEM_NAMES:
        g, T, n = ref[name]
        assert_within(got[name], g, T, n, f"trainer {name}")
