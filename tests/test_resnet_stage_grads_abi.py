"""The C ABI of what csrc/conv_grads.hip and csrc/conv_strided_grads.hip add for projection Bottlenecks, the public switches of DESIGN.md section 4.22, the 2x2
phase pack and the float64 restatement the GPU tests lean on: everything here runs without a GPU."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resnet_stage_grads_restated import projection_block_reference, projection_forward_plain  # noqa: E402
from test_resnet_grads_abi import ROOT, _lib, _plan_bytes, _status  # noqa: E402

# the input sizes of a stride-2 3x3 at which the phase identity was checked: odd, even, single pixels and rows, several tiles
S2D_SHAPES = [(5, 7), (4, 6), (1, 1), (2, 2), (1, 4), (3, 2), (25, 33)]


def d2s_gather(P, H, W):
    """P [N,4 C,OH+1,OW+1] (NCHW) -> d [N,C,H,W]: d[n,c,ih,iw] = P[n, ((ih & 1) 2 + (iw & 1)) C + c, (ih >> 1) + 1, (iw >> 1) + 1]."""
    N, C4 = P.shape[:2]
    C = C4 // 4
    ih, iw = torch.arange(H).view(H, 1).expand(H, W), torch.arange(W).view(1, W).expand(H, W)
    phase = (ih & 1) * 2 + (iw & 1)
    Pv = P.view(N, 4, C, P.shape[2], P.shape[3])
    return Pv[:, phase, :, (ih >> 1) + 1, (iw >> 1) + 1].permute(2, 3, 0, 1)        # [H,W,N,C] -> [N,C,H,W]


@pytest.mark.parametrize("H,W", S2D_SHAPES)
def test_s2d_conv3x3_weight_is_the_stride_2_dgrad(H, W):
    from two_stage_object_detection_amd import hip_ops
    gen = torch.Generator().manual_seed(31 + 100 * H + W)
    N, C, Cout = 2, 4, 8
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = torch.randn(Cout, C, 3, 3, generator=gen, dtype=torch.float64)
    scale = torch.rand(Cout, generator=gen, dtype=torch.float64) + 0.5
    g = torch.randn(N, Cout, OH, OW, generator=gen, dtype=torch.float64)
    u = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    want, = torch.autograd.grad(F.conv2d(u, w, None, 2, 1) * scale.view(1, -1, 1, 1), u, g)
    pack = hip_ops.s2d_conv3x3_weight(w.permute(0, 2, 3, 1).contiguous(), scale)                 # [4 C,2,2,Cout]
    assert tuple(pack.shape) == (4 * C, 2, 2, Cout) and pack.dtype == torch.float64
    P = F.conv2d(g, pack.permute(0, 3, 1, 2), None, 1, 1)
    assert tuple(P.shape) == (N, 4 * C, OH + 1, OW + 1)
    got = d2s_gather(P, H, W)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12
    # the pack holds every scaled weight exactly once: 1 + 2 + 2 + 4 of the 16 entries per (c, o)
    assert int((pack != 0).sum()) == 9 * C * Cout
    assert float((pack.abs().sum() - (w * scale.view(-1, 1, 1, 1)).abs().sum()).abs()) < 1e-9


NEW = (("tsod_conv3x3_strided_wgrad_workspace_bytes", 6), ("tsod_conv3x3_strided_wgrad_f32", 18),
       ("tsod_prelu_grad_d2s_workspace_bytes", 4), ("tsod_prelu_grad_d2s_f32", 15), ("tsod_pixel_subsample_f32", 10),
       ("tsod_pixel_upsample_add_f32", 10))


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in NEW:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
    assert _ffi._SIGNATURES["tsod_prelu_grad_d2s_f32"][1][8] is ctypes.c_float


def test_argument_errors():
    """The four entry points refuse bad arguments on the host, before any launch (the pointers are never dereferenced)."""
    _, L = _lib()
    A, odd = 0x10000, 0x10004

    def caller(fn, ok):
        def call(**kw):
            a = dict(ok, **kw)
            return _status(L, fn(*[a[k] for k in ok], None))
        return call

    ws = L.tsod_conv3x3_strided_wgrad_workspace_bytes(2, 5, 7, 8, 4, 2)
    assert ws > 0
    call = caller(L.tsod_conv3x3_strided_wgrad_f32,
                  dict(g=A, N=2, H=5, W=7, Cout=4, g_pitch=4, x=A, C=8, x_pitch=8, w=A, scale=A, stride=2, dw=A, dscale=A, dshift=A,
                       ws=A, ws_bytes=ws))
    for k in ("g", "x", "w", "scale"):
        assert "INVALID" in call(**{k: None}), k
    assert "INVALID" in call(dw=None, dscale=None, dshift=None)
    assert "INVALID" in call(g_pitch=0) and "INVALID" in call(x_pitch=4) and "INVALID" in call(H=0)
    assert "UNSUPPORTED" in call(stride=3) and "UNSUPPORTED" in call(stride=0) and "UNSUPPORTED" in call(stride=-1)
    assert "ALIGN" in call(x=odd) and "ALIGN" in call(g=odd) and "ALIGN" in call(x_pitch=10) and "ALIGN" in call(C=6, x_pitch=8)
    assert "ALIGN" in call(Cout=2)
    assert "UNSUPPORTED" in call(N=1 << 12, H=1 << 10, W=1 << 10)                     # 2^32 input rows
    assert "WORKSPACE" in call(ws_bytes=ws - 4) and "WORKSPACE" in call(ws=None) and "WORKSPACE" in call(ws=odd)
    # stride 1 asks for the dense entry point's workspace
    assert "WORKSPACE" in call(stride=1, ws_bytes=L.tsod_conv3x3_dense_wgrad_workspace_bytes(2, 5, 7, 8, 4) - 4)

    ws = L.tsod_prelu_grad_d2s_workspace_bytes(2, 5, 7, 8)
    assert ws > 0
    call = caller(L.tsod_prelu_grad_d2s_f32, dict(y=A, N=2, H=5, W=7, C=8, y_pitch=8, p=A, p_pitch=32, slope=0.25, g=A, g_pitch=8,
                                                  num=A, ws=A, ws_bytes=ws))
    for k in ("y", "p", "g"):
        assert "INVALID" in call(**{k: None}), k
    assert "INVALID" in call(y_pitch=4) and "INVALID" in call(g_pitch=4) and "INVALID" in call(p_pitch=28) and "INVALID" in call(W=0)
    assert "ALIGN" in call(y=odd) and "ALIGN" in call(p=odd) and "ALIGN" in call(g=odd)
    assert "ALIGN" in call(C=6, p_pitch=32) and "ALIGN" in call(y_pitch=10) and "ALIGN" in call(p_pitch=34) and "ALIGN" in call(g_pitch=10)
    assert "UNSUPPORTED" in call(N=1 << 12, H=1 << 10, W=1 << 10)
    assert "WORKSPACE" in call(ws_bytes=ws - 4) and "WORKSPACE" in call(ws=None)

    sub = caller(L.tsod_pixel_subsample_f32, dict(x=A, N=2, H=5, W=7, C=8, x_pitch=12, stride=2, xs=A, xs_pitch=8))
    add = caller(L.tsod_pixel_upsample_add_f32, dict(dx=A, N=2, H=5, W=7, C=8, dx_pitch=12, stride=2, d=A, d_pitch=8))
    for call, big, small in ((sub, "x", "xs"), (add, "dx", "d")):
        assert "INVALID" in call(**{big: None}) and "INVALID" in call(**{small: None})
        assert "INVALID" in call(stride=0) and "INVALID" in call(N=0) and "INVALID" in call(C=0)
        assert "INVALID" in call(**{big + "_pitch": 4}) and "INVALID" in call(**{small + "_pitch": 4})
        assert "ALIGN" in call(**{big: odd}) and "ALIGN" in call(**{small: odd}) and "ALIGN" in call(C=6)
        assert "ALIGN" in call(**{big + "_pitch": 10}) and "ALIGN" in call(**{small + "_pitch": 10})
        assert "UNSUPPORTED" in call(N=1 << 12, H=1 << 10, W=1 << 10)


def test_workspace_queries():
    _, L = _lib()
    q = L.tsod_conv3x3_strided_wgrad_workspace_bytes
    for bad in ((0, 5, 7, 8, 4, 2), (2, 0, 7, 8, 4, 2), (2, 5, 0, 8, 4, 2), (2, 5, 7, 0, 4, 2), (2, 5, 7, 8, 0, 2), (2, 5, 7, 6, 4, 2),
                (2, 5, 7, 8, 6, 2), (2, 5, 7, 8, 4, 0), (2, 5, 7, 8, 4, 3), (1 << 12, 1 << 10, 1 << 10, 8, 4, 2)):
        assert q(*bad) == 0, bad
    for (N, H, W, C, Cout, s), want in (((2, 25, 33, 8, 4, 2), (1, 1, 4)), ((1, 50, 84, 512, 512, 2), None), ((2, 5, 7, 8, 12, 2), (1, 1, 1)),
                                        ((1, 5, 7, 48, 68, 2), (2, 4, 1)), ((1, 1, 1, 4, 4, 2), (1, 1, 1)), ((2, 4, 6, 8, 12, 1), None)):
        OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
        plan, nbytes = _plan_bytes(N * OH * OW, Cout, 9 * C)
        assert q(N, H, W, C, Cout, s) == nbytes, (N, H, W, C, Cout, s)
        assert want is None or plan == want, plan
        if s == 1:
            assert nbytes == L.tsod_conv3x3_dense_wgrad_workspace_bytes(N, H, W, C, Cout)
    p = L.tsod_prelu_grad_d2s_workspace_bytes
    assert p(0, 5, 7, 8) == 0 and p(2, 0, 7, 8) == 0 and p(2, 5, 0, 8) == 0 and p(2, 5, 7, 0) == 0 and p(2, 5, 7, 6) == 0
    assert p(1 << 12, 1 << 10, 1 << 10, 8) == 0
    for N, H, W, C in ((1, 1, 1, 4), (2, 5, 7, 68), (8, 50, 84, 512)):
        assert p(N, H, W, C) == L.tsod_prelu_grad_workspace_bytes(N * H * W, C) > 0               # the same grid rule


TEN = ["conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "conv3.weight", "bn3.weight", "bn3.bias",
       "relu.weight"]
THIRTEEN = TEN + ["downsample.0.weight", "downsample.1.weight", "downsample.1.bias"]


def test_trainable_stages_train_from_and_the_trainer():
    from two_stage_object_detection_amd.models import resnet
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    for make, stages in ((resnet.resnet50, ("layer4", "layer3", "layer2")), (resnet.resnet101, ("layer4", "layer3", "layer2")),
                         (resnet.resnet34, ()), (resnet.resnext50_32x4d, ())):
        m = make(include_top=False)
        assert m.trainable_stages == stages
        with pytest.raises(ValueError, match="keeps no stage outputs"):
            m.train_from("layer1")
        for bad in ("layer5", "tail", "") + tuple(s for s in ("layer4", "layer3", "layer2") if s not in stages):
            with pytest.raises(ValueError, match="trainable_stages"):
                m.train_from(bad)
        assert m.train_mode is None and "_watched" not in m.__dict__
    m = resnet.resnet50(include_top=False)
    keys = list(m.state_dict())
    named = dict(m.named_parameters())
    depth = {"layer2": 4, "layer3": 6, "layer4": 3}
    for stage, count in (("layer4", 33), ("layer3", 96), ("layer2", 139)):
        assert m.train_from(stage) is m and m.train_mode == stage
        got = [k for k, _ in m._trainable_named()]
        want = [f"{st}.{i}.{k}" for st in ("layer2", "layer3", "layer4")[("layer2", "layer3", "layer4").index(stage):]
                for i in range(depth[st]) for k in (THIRTEEN if i == 0 else TEN)]
        assert got == want and len(got) == count == len(m.trainable_parameters())
        assert all(named[k] is p for k, p in m._trainable_named())
        assert got == [k for k in named if k in set(got)]                                        # module order
    m.requires_grad_(False)
    assert m._plan_variant() == ()
    for p in m.trainable_parameters():
        p.requires_grad_(True)
    assert m._plan_variant() == ("train_from", "layer2")
    assert m.train_from("layer4")._plan_variant() == ("train_from", "layer4")
    with torch.no_grad():
        assert m._plan_variant() == ()
    # integer modes and n_blocks keep their meaning, the widest section ever set stays watched
    assert m.n_blocks == 2 and m.train_blocks(2)._plan_variant() == ("train_blocks", 2)
    assert [k for k, _ in m._trainable_named()] == [f"layer4.{i}.{k}" for i in (1, 2) for k in TEN]
    with pytest.raises(ValueError, match="n_blocks"):
        m.train_blocks(3)
    assert m.set_train_mode(None).train_mode is None and m._plan_variant() == () and m.trainable_parameters() == []
    assert set(m.__dict__["_watched"]) == {f"{st}.{i}" for st, n in depth.items() for i in range(n)}
    assert list(m.state_dict()) == keys
    m4 = resnet.resnet50(include_top=False).train_from("layer4")
    assert set(m4.__dict__["_watched"]) == {"layer4.0", "layer4.1", "layer4.2"}

    for stage in ("layer4", "layer3", "layer2"):
        tr = FasterRCNNTrainer("train", 20, backbone="resnet50", backbone_grads=stage)
        assert tr.backbone_grads == stage and tr.feat_extra.train_mode is None                   # (forward sets the mode)
    for bad in (1, 2, "tail", "full", "layer1", "layer5"):
        with pytest.raises(ValueError, match="backbone_grads"):
            FasterRCNNTrainer("train", 20, backbone="resnet50", backbone_grads=bad)
    for kw in (dict(backbone_grads="layer4"), dict()):
        with pytest.raises(ValueError, match="bn_batch_stats"):
            FasterRCNNTrainer("train", 20, backbone="resnet50", bn_batch_stats=True, **kw)
    with pytest.raises(ValueError, match="backbone_grads"):
        FasterRCNNTrainer("train", 20, backbone="hardnet39", backbone_grads="layer4")


def _projection_bottleneck(stride):
    from two_stage_object_detection_amd.models.resnet import Bottleneck, _conv
    torch.manual_seed(40 + stride)
    ds = torch.nn.Sequential(_conv(16, 32, 1, stride), torch.nn.BatchNorm2d(32))
    torch.nn.init.kaiming_normal_(ds[0].weight, mode="fan_out", nonlinearity="relu")
    blk = Bottleneck(16, 8, stride=stride, downsample=ds).double().eval()
    assert blk.conv2.weight.shape == (8, 8, 3, 3) and blk.conv2.stride == (stride, stride)
    for bn in (blk.bn1, blk.bn2, blk.bn3, ds[1]):
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.normal_(0, 0.3)
    return blk


@pytest.mark.parametrize("stride,H,W", [(2, 5, 7), (2, 4, 6), (1, 3, 3)])
def test_restatement_against_plain_autograd_of_a_small_projection_bottleneck(stride, H, W):
    """projection_block_reference, fed the plain float64 forward's own outputs as the 'saved' ones, is plain autograd of
    F.conv2d / F.batch_norm(training=False) / F.prelu."""
    from two_stage_object_detection_amd.models import resnet_grads
    blk = _projection_bottleneck(stride)
    assert resnet_grads.eligible_stage(blk) and not resnet_grads.eligible(blk)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(2, 16, H, W, dtype=torch.float64, generator=gen).requires_grad_()
    gy = torch.randn(2, 32, OH, OW, dtype=torch.float64, generator=gen)
    names, params = zip(*blk.named_parameters())
    y1, y2, y3 = projection_forward_plain(blk, x)
    assert y1.shape == (2, 8, H, W) and y2.shape == (2, 8, OH, OW) and y3.shape == (2, 32, OH, OW)
    plain = torch.autograd.grad(y3, list(params) + [x], gy)
    assert all(bool((y < 0).any()) and bool((y > 0).any()) for y in (y1, y2, y3))
    ref, (dx, dxT, n_dx) = projection_block_reference(blk, dict(x=x.detach(), y1=y1.detach(), y2=y2.detach(), y3=y3.detach()), gy)
    assert set(ref) == set(names) and len(names) == 13 and list(names) == THIRTEEN
    for name, p, g in zip(names, params, plain):
        got, T, n = ref[name]
        assert got.shape == p.shape and T.shape == p.shape and n > 0 and bool((T >= got.abs() * (1 - 1e-12)).all()), name
        assert float((got - g).abs().max()) <= 1e-12, name
    assert float((dx - plain[-1]).abs().max()) <= 1e-12 and bool((dxT >= dx.abs() * (1 - 1e-12)).all())
    assert ref["relu.weight"][2] == sum(int((y < 0).sum()) for y in (y1, y2, y3)) + 1
