"""HarDNetFeatureExtraction.train_tail and FasterRCNNTrainer(backbone_grads="tail"): the six tail
gradients against torch's float64 autograd of the four tail modules, fed the tail's own input read back from the HIP run, so
that only the tail is under test.  The bar is tests/dw_grads_restated.py's: |err| <= (n + 8) 2^-24 T elementwise."""
import copy
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dw_grads_restated import assert_within, pack33, tail_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dw1.weight", "dw1.bias", "dw2.weight", "dw2.bias", "pair.weight", "pair.bias")


def seeded_backbone(dev, seed=0):
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    torch.manual_seed(seed)
    m = HarDNetFeatureExtraction(depth_wise=True, arch=39)
    m.requires_grad_(False)
    for p in m.tail_parameters():
        p.requires_grad_(True)
    return m.to(dev).eval()


def images(seed, dev):
    return torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(seed)).to(dev)


def tail_input_and_mask(m, x):
    """The tail's input of the forward that just ran on ``x`` (the plan's buffer, NCHW on the CPU) and the f32 forward's own
    ReLU mask (the first tail conv run again by the forward kernel)."""
    from two_stage_object_detection_amd import hip_ops
    with torch.enable_grad():
        plan = m._plan_for(x, 0)
    t, off = plan.tail_inputs[0]
    conv = m.base[m._tail_indices()[0]]
    C = conv.weight.shape[0]
    with torch.no_grad():
        a = hip_ops.dwconv3x3_nhwc(t.clone(), pack33(conv.weight.detach()), None, conv.bias.detach(), 2, True, C=C, in_off=off)
    x0 = t[..., off:off + C].permute(0, 3, 1, 2).contiguous().cpu()
    return x0, (a > 0).permute(0, 3, 1, 2).cpu()


def reference_for(m, x, gy):
    x0, mask = tail_input_and_mask(m, x)
    return tail_reference(x0, [p.detach().cpu() for p in m.tail_parameters()], gy.cpu(), mask)


@pytest.mark.gpu
def test_train_tail_output_is_unchanged_and_gradients_match_f64(dev):
    m = seeded_backbone(dev)
    x = images(1, dev)
    with torch.no_grad():
        plain = m(x).clone()
        plain_nhwc = m.forward_nhwc(x).clone()
    assert m.train_tail(True) is m
    f = m(x)
    assert tuple(f.shape) == (2, 512, 4, 6) and f.requires_grad and torch.equal(f.detach(), plain)
    with torch.no_grad():                                        # grad mode off: today's path, no node
        assert not m(x).requires_grad
    gy = torch.randn(f.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    f.backward(gy)
    ref = reference_for(m, x, gy)
    for name, p, (g, T, n) in zip(NAMES, m.tail_parameters(), ref):
        assert p.grad is not None and p.grad.shape == p.shape
        assert_within(p.grad, g, T, n, name)
    tail_ids = {id(p) for p in m.tail_parameters()}
    assert all(p.grad is None for p in m.parameters() if id(p) not in tail_ids)
    # the NHWC entry point carries the node too, and gives the same gradients
    first = [p.grad.clone() for p in m.tail_parameters()]
    for p in m.tail_parameters():
        p.grad = None
    fn = m.forward_nhwc(x)
    assert fn.requires_grad and torch.equal(fn.detach(), plain_nhwc)
    fn.backward(gy.permute(0, 2, 3, 1).contiguous())
    assert all(torch.equal(p.grad, g) for p, g in zip(m.tail_parameters(), first))
    # switched off again: today's output, no node, and the plan cache keeps the two kinds apart
    m.train_tail(False)
    out = m(x)
    assert not out.requires_grad and torch.equal(out, plain)
    assert len({k[3:] for k in m._plans}) == 2


@pytest.mark.gpu
def test_two_forwards_then_their_backwards_in_reverse_order(dev):
    m = seeded_backbone(dev).train_tail(True)
    xa, xb = images(3, dev), images(4, dev)
    gen = torch.Generator().manual_seed(5)
    ga, gb = torch.randn(2, 512, 4, 6, generator=gen).to(dev), torch.randn(2, 512, 4, 6, generator=gen).to(dev)
    singles = []
    for x, gy in ((xa, ga), (xb, gb)):
        for p in m.tail_parameters():
            p.grad = None
        m(x).backward(gy)
        singles.append([p.grad.clone() for p in m.tail_parameters()])
    ref_b = reference_for(m, xb, gb)                             # (the plan holds image b's run)
    m(xa)
    ref_a = reference_for(m, xa, ga)
    for p in m.tail_parameters():
        p.grad = None
    fa = m(xa)
    fb = m(xb)
    fb.backward(gb)
    fa.backward(ga)
    for name, p, s1, s2, (g1, T1, n), (g2, T2, _) in zip(NAMES, m.tail_parameters(), singles[0], singles[1], ref_a, ref_b):
        assert_within(p.grad, g1 + g2, T1 + T2, n + 1, f"{name}, b then a")     # one more addition: the accumulation
        assert torch.equal(p.grad, s2 + s1), name                               # each backward gave its own forward's gradient


@pytest.mark.gpu
def test_forward_follows_an_optimizer_step(dev):
    from two_stage_object_detection_amd import optim
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    m = seeded_backbone(dev).train_tail(True)
    x = images(6, dev)
    before = m(x)
    before.backward(torch.ones_like(before))
    opt = optim.AdamW(m.tail_parameters(), lr=1e-2)
    opt.step()
    after = m(x).detach()
    assert not torch.equal(after, before.detach())
    fresh = HarDNetFeatureExtraction(depth_wise=True, arch=39)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(x)
    assert torch.equal(after, want)
    with torch.no_grad():                                        # the refreshed packs serve the plain path too
        assert torch.equal(m(x), want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["no_grad", "inference_mode", "train_tail_off"])
def test_grad_free_forward_right_after_an_optimizer_step(dev, mode):
    """train -> validate: the first forward after ``optimizer.step()`` runs without grad mode (or with train_tail switched off
    again) and must already see the stepped tail, like a fresh model loaded from the stepped state_dict."""
    from two_stage_object_detection_amd import optim
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    m = seeded_backbone(dev).train_tail(True)
    x = images(7, dev)
    with torch.no_grad():
        stale = m(x).clone()                                     # (the grad-free plan and its packs exist before the step)
    f = m(x)
    f.backward(torch.ones_like(f))
    optim.AdamW(m.tail_parameters(), lr=1e-2).step()
    if mode == "no_grad":
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
def test_trainer_backbone_grads_tail(dev, golden_dir):
    from test_trainer_grads import PARAMS, reference_state_dict
    from two_stage_object_detection_amd._ffi import TsodError
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    z = np.load(os.path.join(golden_dir, "trainer_ref.npz"))
    x = (torch.from_numpy(z["img_u8"]).float() / 255)[None].to(dev)
    bbox, label = torch.from_numpy(z["bbox"]).to(dev), torch.from_numpy(z["label"]).to(dev)

    def trainer(**kw):
        # 80 classes: the fixture's weights are an 80-class detector's and its labels (26, 16, 50) need them
        tr = FasterRCNNTrainer("train", 80, **kw)
        tr.load_state_dict(reference_state_dict(), strict=True)
        tr = tr.to(dev).eval()
        tr.feat_extra.requires_grad_(False)
        return tr

    tr = trainer(backbone_grads="tail", head_grads=True)
    tail = tr.feat_extra.tail_parameters()
    for p in tail:
        p.requires_grad_(True)
    losses = tr(x, [bbox], [label])[0]
    losses[-1].backward()
    named = dict(tr.named_parameters())
    assert all(named[k].grad is not None for k in PARAMS) and all(p.grad is not None for p in tail)

    plain = trainer()
    with torch.no_grad():
        want = plain(x, [bbox], [label])[0]
    assert all(torch.equal(a.detach(), b) for a, b in zip(losses, want))
    # the d feature map of the existing features= path for the same forward, then the tail alone in float64
    with torch.no_grad():
        f = plain.feat_extra(x).clone()
    f.requires_grad_(True)
    plain(x, [bbox], [label], features=f)[0][-1].backward()
    x0, mask = tail_input_and_mask(tr.feat_extra.train_tail(True), x)
    ref = tail_reference(x0, [p.detach().cpu() for p in tail], f.grad.cpu(), mask)
    for name, p, (g, T, n) in zip(NAMES, tail, ref):
        assert_within(p.grad, g, T, n, f"trainer {name}")
    # backbone_grads=None with an unfrozen tail: today's error
    strict = trainer(head_grads=True)
    for p in strict.feat_extra.tail_parameters():
        p.requires_grad_(True)
    with pytest.raises(TsodError, match="requires grad"):
        strict(x, [bbox], [label])
    # and in tail mode a body parameter that requires grad is refused
    next(tr.feat_extra.parameters()).requires_grad_(True)
    with pytest.raises(TsodError, match="tail"):
        tr(x, [bbox], [label])


# ------------------------------------------------------------------------------------------------------------ no GPU
def test_exports_exist_in_header_binding_and_library():
    import ctypes
    from two_stage_object_detection_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_dwconv3x3_grad_workspace_bytes", 6), ("tsod_dwconv3x3_grad_f32", 25),
                         ("tsod_gconv1x1_pair_grad_workspace_bytes", 2), ("tsod_gconv1x1_pair_grad_f32", 14)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
    L = _ffi.lib()
    assert L.tsod_version() == 242
    # the queries are host functions: partials only, plus room for g when a ReLU layer's dx is wanted; 0 for a shape the kernel refuses
    a, b = L.tsod_dwconv3x3_grad_workspace_bytes(2, 33, 31, 8, 1, 0), L.tsod_dwconv3x3_grad_workspace_bytes(2, 33, 31, 8, 1, 1)
    assert a > 0 and b == a + 2 * 33 * 31 * 8 * 4
    assert L.tsod_dwconv3x3_grad_workspace_bytes(2, 33, 31, 6, 1, 0) == 0
    assert L.tsod_gconv1x1_pair_grad_workspace_bytes(2046, 512) >= 3 * 512 * 4
    assert L.tsod_gconv1x1_pair_grad_workspace_bytes(0, 512) == 0


def test_backbone_grads_argument():
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    with pytest.raises(ValueError, match="tail"):
        FasterRCNNTrainer("train", 20, backbone="resnet50", backbone_grads="tail")
    with pytest.raises(ValueError, match="backbone_grads"):
        FasterRCNNTrainer("train", 20, backbone_grads="all")
    assert FasterRCNNTrainer("train", 20).backbone_grads is None
    assert FasterRCNNTrainer("train", 20, backbone_grads="tail").backbone_grads == "tail"


def test_train_tail_adds_no_state():
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    m = HarDNetFeatureExtraction(depth_wise=True, arch=39)
    keys = list(m.state_dict())
    assert m.train_mode is None
    m.train_tail(True)
    assert list(m.state_dict()) == keys
    assert len(m.tail_parameters()) == 6 and sum(p.numel() for p in m.tail_parameters()) == 2 * (9216 + 1024) + 1024 + 512
    for clone in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert clone.train_mode == "tail" and list(clone.state_dict()) == keys
    other = HarDNetFeatureExtraction(depth_wise=True, arch=39)
    other.load_state_dict(m.state_dict(), strict=True)
    assert other.train_mode is None
    assert m.train_tail(False).train_mode is None
