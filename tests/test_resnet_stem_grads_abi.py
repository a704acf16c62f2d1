"""The C ABI of csrc/stem_grads.hip, the public switches of DESIGN.md section 4.23 and the float64 restatement the GPU tests lean
on: everything here runs without a GPU."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resnet_stem_grads_restated import (pool_gather_reference, pool_winners, stem_forward_plain,  # noqa: E402
                                        stem_reference, stem_section_reference)
from resnet_stage_grads_restated import projection_forward_plain  # noqa: E402
from test_resnet_grads_abi import ROOT, _lib, _status  # noqa: E402

STEM = ["conv1.weight", "bn1.weight", "bn1.bias", "relu.weight"]
TEN = ["conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "conv3.weight", "bn3.weight", "bn3.bias",
       "relu.weight"]
THIRTEEN = TEN + ["downsample.0.weight", "downsample.1.weight", "downsample.1.bias"]


# ------------------------------------------------------------------------------------------------------------ restatement
def _stem_modules(seed):
    from two_stage_object_detection_amd.models.resnet import _conv
    torch.manual_seed(seed)
    conv, bn, relu = _conv(3, 64, 7, 2, 3).double(), torch.nn.BatchNorm2d(64).double().eval(), torch.nn.PReLU().double()
    torch.nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
    bn.running_mean.normal_(0, 0.2)
    bn.running_var.uniform_(0.5, 1.5)
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.normal_(0, 0.3)
    return conv, bn, relu


@pytest.mark.parametrize("H,W", [(7, 9), (16, 12), (33, 25), (1, 1)])
def test_restatement_against_plain_autograd_of_the_stem(H, W):
    """stem_reference, fed the plain float64 forward's own y as the saved one, is plain autograd of F.conv2d(stride 2, pad 3) /
    F.batch_norm(training=False) / F.prelu / F.max_pool2d(3, 2, 1)."""
    conv, bn, relu = _stem_modules(50 + H)
    gen = torch.Generator().manual_seed(51 + W)
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=gen)
    y, p = stem_forward_plain(conv, bn, relu, x)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert y.shape == (2, 64, OH, OW) and p.shape == (2, 64, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1)
    assert bool((y < 0).any()) and bool((y > 0).any())
    dp = torch.randn(p.shape, dtype=torch.float64, generator=gen)
    params = [conv.weight, bn.weight, bn.bias, relu.weight]
    plain = torch.autograd.grad(p, params, dp)
    ref = stem_reference(conv, bn, relu, dict(x=x, y=y.detach()), dp)
    assert list(ref) == STEM
    for name, prm, want in zip(STEM, params, plain):
        got, T, n = ref[name]
        assert got.shape == prm.shape and T.shape == prm.shape and n > 0 and bool((T >= got.abs() * (1 - 1e-12)).all()), name
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name


@pytest.mark.parametrize("OH,OW", [(1, 1), (2, 2), (5, 7), (4, 6), (9, 12)])
def test_pool_gather_gives_every_tie_to_the_first_maximum_as_autograd_does(OH, OW):
    """Integer-valued activations in -2 .. 2: nearly every window holds its maximum several times; torch's max_pool2d backward
    sends the window's gradient to the first of them in the (kh, kw) scan, and so does the restatement, exactly."""
    gen = torch.Generator().manual_seed(60 + 10 * OH + OW)
    y = torch.randint(-2, 3, (2, 8, OH, OW), generator=gen).double().requires_grad_()
    p = F.max_pool2d(y, 3, 2, 1)
    dp = torch.randint(-3, 4, p.shape, generator=gen).double()
    want, = torch.autograd.grad(p, y, dp)
    dy, T, n = pool_gather_reference(y.detach(), dp)
    assert n == 4 and torch.equal(dy, want) and bool((T >= dy.abs()).all())
    idx = pool_winners(y.detach())
    assert idx.shape == p.shape and int(idx.min()) >= 0 and int(idx.max()) <= 8
    if OH * OW > 1:
        vals = F.unfold(F.pad(y.detach(), (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(2, 8, 9, -1)
        assert bool(((vals == vals.max(2, keepdim=True).values).sum(2) > 1).any())                # the case is about ties
        assert torch.equal(vals.gather(2, idx.view(2, 8, 1, -1)).squeeze(2), p.detach().view(2, 8, -1))
    # every window's gradient lands exactly once
    assert float(dy.sum()) == float(dp.sum())


def test_section_reference_chains_the_stem_in_front_of_the_blocks():
    """stem_section_reference over the stem and one stride-1 projection Bottleneck (layer1.0's kind) is plain autograd of the
    two in a row."""
    from test_resnet_stage_grads_abi import _projection_bottleneck

    class Owner:
        pass
    blk = _projection_bottleneck(1)
    relu = _stem_modules(70)[2]
    conv16 = torch.nn.Conv2d(3, 16, 7, 2, 3, bias=False).double()
    bn16 = torch.nn.BatchNorm2d(16).double().eval()
    bn16.running_mean.normal_(0, 0.2)
    bn16.running_var.uniform_(0.5, 1.5)
    owner = Owner()
    owner.conv1, owner.bn1, owner.relu = conv16, bn16, relu
    gen = torch.Generator().manual_seed(71)
    x = torch.randn(2, 3, 13, 18, dtype=torch.float64, generator=gen)
    y, p = stem_forward_plain(conv16, bn16, relu, x)
    y1, y2, y3 = projection_forward_plain(blk, p)
    gy = torch.randn(y3.shape, dtype=torch.float64, generator=gen)
    names, params = zip(*blk.named_parameters())
    stem_params = [conv16.weight, bn16.weight, bn16.bias, relu.weight]
    plain = torch.autograd.grad(y3, stem_params + list(params), gy)
    ref = stem_section_reference((owner, dict(x=x, y=y.detach())),
                                 [("layer1.0", blk, dict(x=p.detach(), y1=y1.detach(), y2=y2.detach(), y3=y3.detach()))], gy)
    assert set(ref) == set(STEM) | {"layer1.0." + k for k in names}
    for name, want in zip(STEM + ["layer1.0." + k for k in names], plain):
        got, T, n = ref[name]
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
    assert ref["conv1.weight"][2] > ref["layer1.0.conv1.weight"][2]           # the products behind dp are counted


# ------------------------------------------------------------------------------------------------------------------- C ABI
NEW = (("tsod_prelu_grad_pool_workspace_bytes", 4), ("tsod_prelu_grad_pool_f32", 15), ("tsod_conv7x7s2_wgrad_workspace_bytes", 4),
       ("tsod_conv7x7s2_wgrad_f32", 15))


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in NEW:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
    assert _ffi._SIGNATURES["tsod_prelu_grad_pool_f32"][1][8] is ctypes.c_float
    assert "stem_grads.hip" in open(os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "Makefile")).read()


def _caller(L, fn, ok):
    def call(**kw):
        a = dict(ok, **kw)
        return _status(L, fn(*[a[k] for k in ok], None))
    return call


def test_argument_errors():
    """Both entry points refuse bad arguments on the host, before any launch (the pointers are never dereferenced)."""
    _, L = _lib()
    A, odd = 0x10000, 0x10004
    ws = L.tsod_prelu_grad_pool_workspace_bytes(2, 5, 7, 8)
    assert ws > 0
    call = _caller(L, L.tsod_prelu_grad_pool_f32, dict(y=A, N=2, OH=5, OW=7, C=8, y_pitch=8, dp=A, dp_pitch=8, slope=0.25, g=A,
                                                       g_pitch=8, num=A, ws=A, ws_bytes=ws))
    for k in ("y", "dp", "g"):
        assert "INVALID" in call(**{k: None}), k
    assert "INVALID" in call(y_pitch=4) and "INVALID" in call(g_pitch=4) and "INVALID" in call(dp_pitch=4)
    assert "INVALID" in call(N=0) and "INVALID" in call(OH=0) and "INVALID" in call(OW=0) and "INVALID" in call(C=0)
    assert "ALIGN" in call(y=odd) and "ALIGN" in call(dp=odd) and "ALIGN" in call(g=odd)
    assert "ALIGN" in call(C=6) and "ALIGN" in call(y_pitch=10) and "ALIGN" in call(dp_pitch=10) and "ALIGN" in call(g_pitch=10)
    assert "UNSUPPORTED" in call(N=1 << 12, OH=1 << 10, OW=1 << 10)                   # 2^32 rows
    assert "UNSUPPORTED" in call(N=1 << 10, OH=1 << 10, OW=1 << 10, C=8, y_pitch=8)   # 2^31 quads
    assert "WORKSPACE" in call(ws_bytes=ws - 4) and "WORKSPACE" in call(ws=None)

    ws = L.tsod_conv7x7s2_wgrad_workspace_bytes(2, 16, 12, 64)
    assert ws > 0
    call = _caller(L, L.tsod_conv7x7s2_wgrad_f32, dict(g=A, N=2, H=16, W=12, Cout=64, g_pitch=64, x4=A, w=A, scale=A, dw=A, dscale=A,
                                                       dshift=A, ws=A, ws_bytes=ws))
    for k in ("g", "x4", "w", "scale"):
        assert "INVALID" in call(**{k: None}), k
    assert "INVALID" in call(dw=None, dscale=None, dshift=None)
    assert "INVALID" in call(g_pitch=60) and "INVALID" in call(N=0) and "INVALID" in call(H=0) and "INVALID" in call(W=0)
    assert "INVALID" in call(Cout=0)
    assert "ALIGN" in call(g=odd) and "ALIGN" in call(x4=odd) and "ALIGN" in call(w=odd) and "ALIGN" in call(scale=odd)
    assert "ALIGN" in call(dw=odd) and "ALIGN" in call(g_pitch=66) and "ALIGN" in call(Cout=62)
    for cout in (4, 32, 60, 68, 128):                              # only the stem's 64 output channels are built
        assert "UNSUPPORTED" in call(Cout=cout, g_pitch=128), cout
    assert "UNSUPPORTED" in call(N=1 << 10, H=1 << 10, W=1 << 10)                     # 4 N H W beyond 32 bits
    assert "WORKSPACE" in call(ws_bytes=ws - 4) and "WORKSPACE" in call(ws=None) and "WORKSPACE" in call(ws=odd)


def stem7_slices(N, H, W):
    """The shipped slice rule as a function of the shape: pixel pairs numbered (n, oh, ow / 2); ceil(pairs / 256) pairs per slice,
    at least 64 -> (slices, pairs per slice, pairs in the last slice)."""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pairs = N * OH * ((OW + 1) // 2)
    per = max(64, -(-pairs // 256))
    slices = -(-pairs // per)
    return slices, per, pairs - (slices - 1) * per


def test_workspace_queries_and_the_slice_rule():
    _, L = _lib()
    p = L.tsod_prelu_grad_pool_workspace_bytes
    assert p(0, 5, 7, 8) == 0 and p(2, 0, 7, 8) == 0 and p(2, 5, 0, 8) == 0 and p(2, 5, 7, 0) == 0 and p(2, 5, 7, 6) == 0
    assert p(1 << 12, 1 << 10, 1 << 10, 8) == 0 and p(1 << 10, 1 << 10, 1 << 10, 8) == 0
    for N, OH, OW, C in ((1, 1, 1, 4), (2, 5, 7, 68), (2, 40, 56, 64), (8, 400, 667, 64)):
        assert p(N, OH, OW, C) == L.tsod_prelu_grad_workspace_bytes(N * OH * OW, C) > 0           # the same grid rule
    assert p(2, 40, 56, 64) == 4 * 280 and p(8, 400, 667, 64) == 4 * 1024
    q = L.tsod_conv7x7s2_wgrad_workspace_bytes
    for bad in ((0, 16, 12, 64), (2, 0, 12, 64), (2, 16, 0, 64), (2, 16, 12, 0), (2, 16, 12, 32), (2, 16, 12, 128), (2, 16, 12, 62),
                (1 << 10, 1 << 10, 1 << 10, 64)):
        assert q(*bad) == 0, bad
    for (N, H, W), want in (((1, 1, 1), (1, 64, 1)), ((1, 64, 96), (12, 64, 64)), ((2, 61, 93), (24, 64, 16)),
                            ((2, 16, 12), (1, 64, 48)), ((1, 800, 1333), (256, 522, 490)), ((8, 800, 1333), (256, 4175, 4175))):
        assert stem7_slices(N, H, W) == want, (N, H, W)
        assert q(N, H, W, 64) == want[0] * 64 * 225 * 4, (N, H, W)


# ------------------------------------------------------------------------------------------------------------ public surface
def test_trainable_sections_train_full_and_the_trainer():
    from two_stage_object_detection_amd.models import resnet
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    stages = ("layer4", "layer3", "layer2")
    for make, sections, count in ((resnet.resnet50, stages + ("stem",), 176), (resnet.resnet101, stages + ("stem",), 346),
                                  (resnet.resnet34, (), 0), (resnet.resnext50_32x4d, (), 0)):
        m = make(include_top=False)
        keys = list(m.state_dict())
        assert m.trainable_sections == sections and m.trainable_stages == sections[:3]
        if not sections:
            for call in (lambda: m.train_from("stem"), m.train_full):
                with pytest.raises(ValueError, match="trainable_stages"):
                    call()
            assert m.train_mode is None and "_watched" not in m.__dict__
            continue
        assert m.train_full() is m and m.train_mode == "stem" and m.set_train_mode(None).train_from("stem") is m
        named = dict(m.named_parameters())
        got = [k for k, _ in m._trainable_named()]
        assert got == list(named) and len(got) == count == len(m.trainable_parameters())          # every parameter, module order
        assert all(named[k] is p for k, p in m._trainable_named())
        depth = [len(getattr(m, f"layer{i}")) for i in (1, 2, 3, 4)]
        assert got == STEM + [f"layer{li}.{i}.{k}" for li, n in zip((1, 2, 3, 4), depth) for i in range(n)
                              for k in (THIRTEEN if i == 0 else TEN)]
        m.requires_grad_(False)
        assert m._plan_variant() == ()
        m.relu.weight.requires_grad_(True)
        assert m._plan_variant() == ("train_from", "stem")
        with torch.no_grad():
            assert m._plan_variant() == ()
        watched = {"conv1", "bn1", "relu"} | {f"layer{li}.{i}" for li, n in zip((1, 2, 3, 4), depth) for i in range(n)}
        assert set(m.__dict__["_watched"]) == watched
        assert m.train_from("layer4")._plan_variant() == () and set(m.__dict__["_watched"]) == watched   # the widest stays watched
        assert len(m.train_from("layer2").trainable_parameters()) == count - 37
        assert list(m.state_dict()) == keys
    # what makes the stem offerable
    m = resnet.resnet50(include_top=False)
    m.maxpool = torch.nn.MaxPool2d(2, 2)
    assert m.trainable_sections == stages
    m = resnet.resnet50(include_top=False)
    m.conv1 = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=True)
    assert m.trainable_sections == stages
    with pytest.raises(ValueError, match="keeps no stage outputs") as e:
        resnet.resnet50(include_top=False).train_from("layer1")
    assert "trainable_stages" in str(e.value) and "stem" in str(e.value)

    for backbone in ("resnet50", "resnet101"):
        tr = FasterRCNNTrainer("train", 20, backbone=backbone, backbone_grads="stem")
        assert tr.backbone_grads == "stem" and tr.feat_extra.train_mode is None                  # (forward sets the mode)
    for kw in (dict(backbone="hardnet39"), dict(backbone="resnet50", bn_batch_stats=True)):
        with pytest.raises(ValueError, match="backbone_grads|bn_batch_stats"):
            FasterRCNNTrainer("train", 20, backbone_grads="stem", **kw)
