"""The C ABI of csrc/conv_grads.hip, the public switches of DESIGN.md section 4.21 and the float64 restatement the GPU tests lean
on: everything here runs without a GPU."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resnet_grads_restated import block_reference, bottleneck_forward_plain  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from two_stage_object_detection_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi, _ffi.lib()


def _status(L, rc):
    return L.tsod_status_str(rc).decode().upper()


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_prelu_grad_workspace_bytes", 2), ("tsod_prelu_grad_f32", 14),
                         ("tsod_conv3x3_dense_wgrad_workspace_bytes", 5), ("tsod_conv3x3_dense_wgrad_f32", 18)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
    # the float argument is the slope, by value
    assert _ffi._SIGNATURES["tsod_prelu_grad_f32"][1][7] is ctypes.c_float
    assert "float slope" in re.search(r"\btsod_prelu_grad_f32\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)


def test_argument_errors():
    """The entry points refuse bad arguments on the host, before any launch (the pointers are never dereferenced)."""
    _, L = _lib()
    A, odd = 0x10000, 0x10004                                   # a 16-byte aligned address and a misaligned one
    P = L.tsod_prelu_grad_f32
    ws = L.tsod_prelu_grad_workspace_bytes(70, 12)
    assert ws > 0
    assert "INVALID" in _status(L, P(None, 70, 12, 12, A, 12, 0, 0.25, A, 12, A, A, ws, None))
    assert "INVALID" in _status(L, P(A, 70, 12, 12, None, 12, 0, 0.25, A, 12, A, A, ws, None))
    assert "INVALID" in _status(L, P(A, 70, 12, 12, A, 12, 0, 0.25, None, 12, A, A, ws, None))
    assert "INVALID" in _status(L, P(A, 70, 12, 8, A, 12, 0, 0.25, A, 12, A, A, ws, None))          # pitch below C
    assert "INVALID" in _status(L, P(A, 70, 12, 12, A, 12, 4, 0.25, A, 12, A, A, ws, None))         # offset + C beyond the pitch
    assert "ALIGN" in _status(L, P(odd, 70, 12, 12, A, 12, 0, 0.25, A, 12, A, A, ws, None))
    assert "ALIGN" in _status(L, P(A, 70, 12, 12, A, 12, 0, 0.25, odd, 12, A, A, ws, None))
    assert "ALIGN" in _status(L, P(A, 70, 12, 14, A, 12, 0, 0.25, A, 12, A, A, ws, None))
    assert "ALIGN" in _status(L, P(A, 70, 10, 12, A, 12, 0, 0.25, A, 12, A, A, ws, None))           # C not a multiple of 4
    assert "ALIGN" in _status(L, P(A, 70, 12, 12, A, 20, 6, 0.25, A, 12, A, A, ws, None))
    assert "WORKSPACE" in _status(L, P(A, 70, 12, 12, A, 12, 0, 0.25, A, 12, A, A, ws - 4, None))
    assert "WORKSPACE" in _status(L, P(A, 70, 12, 12, A, 12, 0, 0.25, A, 12, A, None, ws, None))

    D = L.tsod_conv3x3_dense_wgrad_f32
    ws = L.tsod_conv3x3_dense_wgrad_workspace_bytes(2, 3, 5, 8, 4)
    assert ws > 0
    ok = dict(g=A, N=2, H=3, W=5, Cout=4, g_pitch=4, x=A, C=8, x_pitch=8, w=A, scale=A, stride=1, dw=A, dscale=A, dshift=A, ws=A,
              ws_bytes=ws)

    def call(**kw):
        a = dict(ok, **kw)
        return _status(L, D(*[a[k] for k in ok], None))
    for k in ("g", "x", "w", "scale"):
        assert "INVALID" in call(**{k: None}), k
    assert "INVALID" in call(dw=None, dscale=None, dshift=None)             # nothing wanted
    assert "INVALID" in call(g_pitch=0) and "INVALID" in call(x_pitch=4) and "INVALID" in call(H=0)
    assert "UNSUPPORTED" in call(stride=2) and "UNSUPPORTED" in call(stride=0)
    assert "ALIGN" in call(x=odd) and "ALIGN" in call(g=odd) and "ALIGN" in call(x_pitch=10) and "ALIGN" in call(C=6, x_pitch=8)
    assert "ALIGN" in call(Cout=2)
    assert "WORKSPACE" in call(ws_bytes=ws - 4) and "WORKSPACE" in call(ws=None) and "WORKSPACE" in call(ws=odd)


def _plan_bytes(M, N, K):
    """csrc/grad_reduce.h's tsod_wgrad_plan_of(M, N, K, cap_by_operands = true), restated."""
    n_tiles, k_tiles = -(-N // 64), -(-K // 128)
    n_pad, k_pad = 64 * n_tiles, 128 * k_tiles
    pairs = (M + 1) // 2
    splits = min(-(-512 // (n_tiles * k_tiles)), -(-pairs // 64), M * (N + K) // (n_pad * k_pad))
    splits = max(splits, 1)
    per = -(-pairs // splits)
    splits = max(1, -(-pairs // per))
    return (n_tiles, k_tiles, splits), splits * n_pad * (k_pad + 1) * 4


def test_workspace_queries():
    _, L = _lib()
    q = L.tsod_conv3x3_dense_wgrad_workspace_bytes
    for bad in ((0, 3, 5, 8, 4), (2, 0, 5, 8, 4), (2, 3, 0, 8, 4), (2, 3, 5, 0, 4), (2, 3, 5, 8, 0), (2, 3, 5, 6, 4), (2, 3, 5, 8, 6),
                (1 << 12, 1 << 10, 1 << 10, 8, 4)):
        assert q(*bad) == 0, bad
    for (N, H, W, C, Cout), want in (((1, 1, 1, 8, 4), (1, 1, 1)), ((2, 3, 5, 48, 68), (2, 4, 1)), ((2, 5, 7, 128, 64), (1, 9, 1)),
                                     ((2, 13, 17, 8, 4), (1, 1, 4)), ((1, 25, 42, 512, 512), None)):
        plan, nbytes = _plan_bytes(N * H * W, Cout, 9 * C)
        assert q(N, H, W, C, Cout) == nbytes == L.tsod_pw_wgrad_workspace_bytes(N * H * W, Cout, 9 * C)
        assert want is None or plan == want
    p = L.tsod_prelu_grad_workspace_bytes
    assert p(0, 8) == 0 and p(8, 0) == 0 and p(8, 6) == 0 and p(-1, 8) == 0
    assert p(1, 4) == 4 and p(257, 68) == 4 * -(-257 * 17 // 256) and p(1 << 20, 2048) == 4 * 1024


def test_n_blocks_train_blocks_and_the_trainer():
    from two_stage_object_detection_amd.models import resnet
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    for make, n in ((resnet.resnet50, 2), (resnet.resnet101, 2), (resnet.resnet34, 0), (resnet.resnext50_32x4d, 0)):
        m = make(include_top=False)
        assert m.n_blocks == n and m.train_mode is None and m.trainable_parameters() == []
        for bad in (0, -1, n + 1):
            with pytest.raises(ValueError, match="n_blocks"):
                m.train_blocks(bad)
        assert m.train_mode is None
    m = resnet.resnet50(include_top=False)
    keys = list(m.state_dict())
    ten = ["conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "conv3.weight", "bn3.weight",
           "bn3.bias", "relu.weight"]
    assert m.train_blocks(1) is m and m.train_mode == 1
    assert [k for k, _ in m._trainable_named()] == [f"layer4.2.{k}" for k in ten]
    assert [id(p) for p in m.trainable_parameters()] == [id(p) for p in m.layer4[2].parameters()]
    m.train_blocks(2)
    assert [k for k, _ in m._trainable_named()] == [f"layer4.{i}.{k}" for i in (1, 2) for k in ten]
    named = dict(m.named_parameters())
    assert all(named[k] is p for k, p in m._trainable_named())
    m.requires_grad_(False)
    assert m._plan_variant() == ()                              # nothing of the section requires grad: the plain plan
    for p in m.trainable_parameters():
        p.requires_grad_(True)
    assert m._plan_variant() == ("train_blocks", 2)
    with torch.no_grad():
        assert m._plan_variant() == ()
    with torch.inference_mode():
        assert m._plan_variant() == ()
    assert m.set_train_mode(None).train_mode is None and m.trainable_parameters() == [] and m._plan_variant() == ()
    assert list(m.state_dict()) == keys
    assert set(m.__dict__["_watched"]) == {"layer4.1", "layer4.2"}          # the widest mode ever set stays watched
    with pytest.raises(ValueError, match="backbone_grads"):
        FasterRCNNTrainer("train", 20, backbone="resnet50", backbone_grads=1)
    assert FasterRCNNTrainer("train", 20, backbone="resnet50", head_grads=True).feat_extra.n_blocks == 2


def test_restatement_against_plain_autograd_of_a_small_bottleneck():
    """block_reference, fed the plain float64 forward's own outputs as the 'saved' ones, is plain autograd of F.conv2d /
    F.batch_norm(training=False) / F.prelu."""
    from two_stage_object_detection_amd.models.resnet import Bottleneck
    torch.manual_seed(4)
    blk = Bottleneck(32, 8).double().eval()
    assert blk.conv2.weight.shape == (8, 8, 3, 3)
    for bn in (blk.bn1, blk.bn2, blk.bn3):
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.normal_(0, 0.3)
    x = torch.randn(2, 32, 5, 7, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(2, 32, 5, 7, dtype=torch.float64)
    names, params = zip(*blk.named_parameters())
    y1, y2, y3 = bottleneck_forward_plain(blk, x)
    plain = torch.autograd.grad(y3, list(params) + [x], gy)
    assert all(bool((y < 0).any()) and bool((y > 0).any()) for y in (y1, y2, y3))          # (both branches are exercised)
    ref, (dx, dxT, n_dx) = block_reference(blk, dict(x=x.detach(), y1=y1.detach(), y2=y2.detach(), y3=y3.detach()), gy)
    assert set(ref) == set(names) and len(names) == 10
    for name, p, g in zip(names, params, plain):
        got, T, n = ref[name]
        assert got.shape == p.shape and T.shape == p.shape and n > 0 and bool((T >= got.abs() * (1 - 1e-12)).all()), name
        assert float((got - g).abs().max()) <= 1e-12 * float(g.abs().max()), name
    assert float((dx - plain[-1]).abs().max()) <= 1e-12 * float(plain[-1].abs().max()) and bool((dxT >= dx.abs() * (1 - 1e-12)).all())
    assert ref["relu.weight"][2] == sum(int((y < 0).sum()) for y in (y1, y2, y3)) + 1
