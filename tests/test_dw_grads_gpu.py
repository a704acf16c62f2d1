"""tsod_dwconv3x3_grad_f32 / tsod_gconv1x1_pair_grad_f32 and the autograd operators over them,
against torch's float64 autograd on the CPU with the derived bar of tests/dw_grads_restated.py:
|err| <= (n + 8) 2^-24 T elementwise, T = sum of |products| of the element, n = their number."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dw_grads_restated import assert_within, dw_reference, pack33, pair_reference, unpack33  # noqa: E402

pytestmark = pytest.mark.gpu

# (N, H, W, C), pixel pitch, channel offset
SHAPES = [((1, 1, 1, 4), 4, 0),          # degenerate map: every tap but the centre in the padding
          ((2, 7, 9, 12), 20, 4),        # odd extents at stride 2, a slice inside a wider pixel, batch boundary
          ((2, 8, 6, 260), 260, 0),      # even extents; more channel quads (65) than one wave holds
          ((2, 33, 31, 8), 8, 0)]        # 2 046 pixels: the reduction spans several workgroups


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def draw(shape, stride, relu, with_scale, with_shift, c_real=None, seed0=0):
    """Inputs of one case (CPU f32, NHWC) such that no pre-ReLU value lies within 1e-4 of zero: the first seed that does."""
    N, H, W, C = shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    for seed in range(seed0, seed0 + 64):
        g = torch.Generator().manual_seed(1000 + seed)
        x = torch.randn(N, H, W, C, generator=g)
        w = torch.randn(C, 1, 3, 3, generator=g)
        scale = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1) if with_scale else None
        shift = torch.randn(C, generator=g) if with_shift else None
        dy = torch.randn(N, OH, OW, C, generator=g)
        if c_real is not None:                                   # pad channels: exact zeros everywhere
            x[..., c_real:] = 0
            w[c_real:] = 0
            dy[..., c_real:] = 0
            if scale is not None:
                scale[c_real:] = 0
            if shift is not None:
                shift[c_real:] = 0
        ref = dw_reference(nchw(x), w, scale, shift, stride, relu, nchw(dy))
        if c_real is not None and relu:                          # (the pad channels' pre-ReLU value IS zero: judge the real ones)
            ref["clear"] = bool((ref["y"][:, :c_real].abs() > 1e-4).all())
        if ref["clear"]:
            return x, w, scale, shift, dy, ref
    raise AssertionError("no seed keeps the pre-ReLU values away from zero")


def run_grad(dev, x, w, scale, shift, stride, relu, dy, pitch, off, *, want_dx=True, want_dscale=True, dx0=None,
             short_ws=0):
    """One raw tsod_dwconv3x3_grad_f32 call on pitched buffers -> (rc, dx [N,H,W,C] or None, dw [3,3,C], dscale, dshift)."""
    from two_stage_object_detection_amd import _ffi
    L = _ffi.lib()
    N, H, W, C = x.shape
    fill = torch.Generator().manual_seed(7)
    xb = torch.randn(N, H, W, pitch, generator=fill)
    xb[..., off:off + C] = x
    dyb = torch.randn(tuple(dy.shape[:3]) + (pitch,), generator=fill)
    dyb[..., off:off + C] = dy
    xb, dyb = xb.to(dev), dyb.to(dev)
    dxb = None
    if want_dx:
        dxb = torch.full((N, H, W, pitch), 7.0)
        if dx0 is not None:
            dxb[..., off:off + C] = dx0
        dxb = dxb.to(dev)
    w33 = pack33(w).to(dev)
    sc = None if scale is None else scale.to(dev)
    sh = None if shift is None else shift.to(dev)
    dw = torch.full((3, 3, C), 9.0, device=dev)
    dscale = torch.full((C,), 9.0, device=dev) if (sc is not None and want_dscale) else None
    dshift = torch.full((C,), 9.0, device=dev)
    ws_bytes = L.tsod_dwconv3x3_grad_workspace_bytes(N, H, W, C, stride, int(relu and want_dx))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rc = L.tsod_dwconv3x3_grad_f32(xb.data_ptr(), N, H, W, C, pitch, off, w33.data_ptr(), _ffi.ptr(sc), _ffi.ptr(sh), stride,
                                   int(relu), dyb.data_ptr(), pitch, off, _ffi.ptr(dxb), pitch, off, 1 if dx0 is not None else 0,
                                   dw.data_ptr(), _ffi.ptr(dscale), dshift.data_ptr(), ws.data_ptr(), ws_bytes - short_ws,
                                   _ffi.stream_ptr())
    torch.cuda.synchronize()
    if dxb is not None and rc == 0:                              # nothing outside the slice was touched
        keep = torch.ones(pitch, dtype=torch.bool)
        keep[off:off + C] = False
        assert bool((dxb.cpu()[..., keep] == 7.0).all())
    return rc, None if dxb is None else dxb[..., off:off + C].cpu(), dw.cpu(), None if dscale is None else dscale.cpu(), dshift.cpu()


def check_case(dev, shape, pitch, off, stride, relu, with_scale, with_shift, c_real=None):
    x, w, scale, shift, dy, ref = draw(shape, stride, relu, with_scale, with_shift, c_real)
    assert ref["clear"]
    rc, dx, dw, dscale, dshift = run_grad(dev, x, w, scale, shift, stride, relu, dy, pitch, off)
    assert rc == 0
    tag = f"{shape} s{stride} relu={relu} scale={with_scale} shift={with_shift}"
    assert_within(nchw(dx), *ref["dx"], f"dx {tag}")
    assert_within(unpack33(dw), *ref["dw"], f"dw {tag}")
    assert_within(dshift, *ref["dshift"], f"dshift {tag}")
    if with_scale:
        assert_within(dscale, *ref["dscale"], f"dscale {tag}")
    # accumulate = 1 onto a non-zero dx: one more addition per element
    dx0 = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    rc, dx_acc, dw2, _, _ = run_grad(dev, x, w, scale, shift, stride, relu, dy, pitch, off, dx0=dx0)
    assert rc == 0 and torch.equal(dw2, dw)
    g, T, n = ref["dx"]
    assert_within(nchw(dx_acc), g + nchw(dx0).double(), T + nchw(dx0).double().abs(), n + 1, f"dx accumulate {tag}")
    return x, w, scale, shift, dy, (dx, dw, dscale, dshift)


@pytest.mark.parametrize("shape,pitch,off", SHAPES, ids=[str(s[0]) for s in SHAPES])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("relu,with_scale,with_shift", [(False, False, False), (True, False, True), (False, True, True),
                                                        (True, True, True)])
def test_dwconv3x3_grad(dev, shape, pitch, off, stride, relu, with_scale, with_shift):
    check_case(dev, shape, pitch, off, stride, relu, with_scale, with_shift)


@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv3x3_grad_pad_channels_stay_zero(dev, stride):
    """C real = 10 in a pad of 12: zero pad channels of w, dy, x give exactly zero gradients there."""
    _, _, _, _, _, (dx, dw, dscale, dshift) = check_case(dev, (2, 7, 9, 12), 12, 0, stride, True, True, True, c_real=10)
    assert bool((dx[..., 10:] == 0).all()) and bool((dw[..., 10:] == 0).all())
    assert bool((dscale[10:] == 0).all()) and bool((dshift[10:] == 0).all())


def test_dwconv3x3_grad_null_outputs_and_bit_identical_runs(dev):
    """dx = NULL and dscale = NULL leave the other outputs unchanged; two runs of the largest case are bit-identical."""
    shape, pitch, off = SHAPES[3]
    x, w, scale, shift, dy, _ = draw(shape, 1, True, True, True)
    full = run_grad(dev, x, w, scale, shift, 1, True, dy, pitch, off)
    again = run_grad(dev, x, w, scale, shift, 1, True, dy, pitch, off)
    assert full[0] == 0 and all(torch.equal(a, b) for a, b in zip(full[1:], again[1:]))
    rc, dx, dw, dscale, dshift = run_grad(dev, x, w, scale, shift, 1, True, dy, pitch, off, want_dx=False, want_dscale=False)
    assert rc == 0 and dx is None and dscale is None
    assert torch.equal(dw, full[2]) and torch.equal(dshift, full[4])


def test_dwconv3x3_grad_refuses_bad_arguments(dev):
    """C % 4 != 0, stride 3, a short workspace, dscale without scale: an error status, nothing launched (outputs untouched)."""
    from two_stage_object_detection_amd import _ffi
    L = _ffi.lib()
    x, w, scale, shift, dy, _ = draw((2, 7, 9, 12), 1, False, True, True)
    rc, dx, dw, _, dshift = run_grad(dev, x, w, scale, shift, 1, False, dy, 12, 0, short_ws=16)
    assert rc == -4 and bool((dx == 7.0).all()) and bool((dw == 9.0).all()) and bool((dshift == 9.0).all())
    P = torch.zeros(4096, device=dev)
    p, n = P.data_ptr(), P.numel() * 4
    s = _ffi.stream_ptr()
    assert L.tsod_dwconv3x3_grad_f32(p, 1, 4, 4, 6, 8, 0, p, None, None, 1, 0, p, 8, 0, p, 8, 0, 0, p, None, p, p, n, s) == -3   # C % 4
    assert L.tsod_dwconv3x3_grad_f32(p, 1, 4, 4, 8, 8, 0, p, None, None, 3, 0, p, 8, 0, p, 8, 0, 0, p, None, p, p, n, s) == -1   # stride 3
    assert L.tsod_dwconv3x3_grad_f32(p, 1, 4, 4, 8, 8, 0, p, None, None, 1, 0, p, 8, 0, p, 8, 0, 0, p, p, p, p, n, s) == -1      # dscale, no scale
    assert L.tsod_dwconv3x3_grad_f32(p, 1, 4, 4, 8, 8, 4, p, None, None, 1, 0, p, 8, 0, p, 8, 0, 0, p, None, p, p, n, s) == -1   # slice past the pitch
    assert L.tsod_dwconv3x3_grad_workspace_bytes(1, 4, 4, 6, 1, 0) == 0 and L.tsod_dwconv3x3_grad_workspace_bytes(1, 4, 4, 8, 3, 0) == 0
    assert L.tsod_gconv1x1_pair_grad_f32(p, 16, 8, 12, p, p, 8, p, 16, p, p, p, n, s) == -1                                     # in_pitch < 2G
    assert L.tsod_gconv1x1_pair_grad_f32(p, 16, 8, 16, p, p, 8, p, 16, p, p, p, 16, s) == -4                                    # short workspace
    torch.cuda.synchronize()
    assert bool((P == 0).all())


@pytest.mark.parametrize("relu", [False, True])
def test_dwconv3x3_grad_dx_alone(dev, relu):
    """No parameter gradient asked for (dw = dshift = NULL): dx is bit-equal to the full call's; without a ReLU no workspace is
    needed.  dw without dshift, or nothing at all, is refused."""
    from two_stage_object_detection_amd import _ffi, hip_ops
    x, w, scale, shift, dy, _ = draw((2, 7, 9, 12), 2, relu, True, True)
    xd, w33, sc, sh, dyd = x.to(dev), pack33(w).to(dev), scale.to(dev), shift.to(dev), dy.to(dev)
    full = hip_ops.dwconv3x3_grad(xd, w33, sc, sh, 2, relu, dyd)
    alone = hip_ops.dwconv3x3_grad(xd, w33, sc, sh, 2, relu, dyd, want_params=False)
    assert alone[1] is None and alone[2] is None and alone[3] is None and torch.equal(alone[0], full[0])
    L, s = _ffi.lib(), _ffi.stream_ptr()
    dx = torch.full_like(xd, 7.0)
    args = (xd.data_ptr(), 2, 7, 9, 12, 12, 0, w33.data_ptr(), sc.data_ptr(), sh.data_ptr(), 2, int(relu), dyd.data_ptr(), 12, 0)
    rc = L.tsod_dwconv3x3_grad_f32(*args, dx.data_ptr(), 12, 0, 0, None, None, None, None, 0, s)
    torch.cuda.synchronize()
    if relu:
        assert rc == -4 and bool((dx == 7.0).all())              # (g has to be made: the workspace is needed)
    else:
        assert rc == 0 and torch.equal(dx, full[0])
    dw = torch.zeros(3, 3, 12, device=dev)
    assert L.tsod_dwconv3x3_grad_f32(*args, dx.data_ptr(), 12, 0, 0, dw.data_ptr(), None, None, None, 0, s) == -1
    assert L.tsod_dwconv3x3_grad_f32(*args, None, 12, 0, 0, None, None, None, None, 0, s) == -1


def test_slices_and_output_buffers_keep_the_plain_path(dev):
    """A call with C / in_off / out on tensors that require grad runs as before: no node, no error."""
    from two_stage_object_detection_amd import hip_ops
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 5, 6, 16, generator=g).to(dev).requires_grad_()
    w33 = torch.randn(3, 3, 8, generator=g).to(dev).requires_grad_()
    y = hip_ops.dwconv3x3_nhwc(x, w33, None, None, 1, False, C=8, in_off=8)
    assert not y.requires_grad
    assert torch.equal(y, hip_ops.dwconv3x3_nhwc(x.detach()[..., 8:].contiguous(), w33.detach(), None, None, 1, False))
    wp = torch.randn(4, 2, generator=g).to(dev).requires_grad_()
    assert not hip_ops.gconv1x1_pair_nhwc(x, wp).requires_grad    # (x wider than 2G)


# ------------------------------------------------------------------------------------------------------- the pair conv
def run_pair(dev, x, w, dy, in_pitch, **want):
    from two_stage_object_detection_amd import hip_ops
    P, G = dy.shape
    xb = torch.randn(P, in_pitch, generator=torch.Generator().manual_seed(5))
    xb[:, :2 * G] = x
    return [None if v is None else v.cpu() for v in hip_ops.gconv1x1_pair_grad(xb.to(dev), w.to(dev), dy.to(dev), **want)]


@pytest.mark.parametrize("pixels,G,in_pitch", [(1, 4, 8), (35, 6, 16), (2046, 512, 1024)])
def test_gconv1x1_pair_grad(dev, pixels, G, in_pitch):
    g = torch.Generator().manual_seed(pixels)
    x, w, dy = torch.randn(pixels, 2 * G, generator=g), torch.randn(G, 2, generator=g), torch.randn(pixels, G, generator=g)
    ref = pair_reference(x, w, dy)
    dx, dw, db = run_pair(dev, x, w, dy, in_pitch)
    assert_within(dx, *ref["dx"], f"pair d_in {pixels}x{G}")
    assert_within(dw, *ref["dw"], f"pair dw {pixels}x{G}")
    assert_within(db, *ref["dbias"], f"pair dbias {pixels}x{G}")
    again = run_pair(dev, x, w, dy, in_pitch)
    assert all(torch.equal(a, b) for a, b in zip((dx, dw, db), again))                # bit-identical from run to run
    only_dw = run_pair(dev, x, w, dy, in_pitch, want_dx=False, want_dbias=False)
    assert only_dw[0] is None and only_dw[2] is None and torch.equal(only_dw[1], dw)


# --------------------------------------------------------------------------------------------------- autograd operators
@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_layer_through_autograd(dev, stride):
    """hip_ops.dwconv3x3_nhwc with BN folded by torch ops under autograd = the f64 autograd of a DWConvLayer in eval mode:
    d gamma, d beta, d w, d x."""
    from two_stage_object_detection_amd import hip_ops
    N, H, W, C = 2, 9, 7, 24
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn(N, H, W, C, generator=g), torch.randn(C, 1, 3, 3, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    mean, var = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    dy = torch.randn(N, (H - 1) // stride + 1, (W - 1) // stride + 1, C, generator=g)
    eps = 1e-5
    # float64 autograd of conv2d(groups=C) + eval-mode batch_norm
    xs, ws, gs, bs = (v.double().requires_grad_() for v in (nchw(x), w, gamma, beta))
    y = F.batch_norm(F.conv2d(xs, ws, None, stride, 1, groups=C), mean.double(), var.double(), gs, bs, False, 0.0, eps)
    want = torch.autograd.grad(y, [xs, ws, gs, bs], nchw(dy).double())
    inv = 1.0 / torch.sqrt(var.double() + eps)
    ref = dw_reference(nchw(x), w, (gamma.double() * inv).float(), None, stride, False, nchw(dy))
    # the HIP operator, BN folded by torch ops on the device
    xd, gd, bd = (v.to(dev).requires_grad_() for v in (x, gamma, beta))
    w33 = pack33(w).to(dev).requires_grad_()
    scale = gd / torch.sqrt(var.to(dev) + eps)
    shift = bd - mean.to(dev) * scale
    out = hip_ops.dwconv3x3_nhwc(xd, w33, scale, shift, stride, False)
    assert out.requires_grad
    dx, dw, dgamma, dbeta = torch.autograd.grad(out, [xd, w33, gd, bd], dy.to(dev))
    pixels = ref["dw"][2]
    assert_within(nchw(dx.cpu()), want[0], ref["dx"][1], 9 + 2, "layer dx")              # (+2: the f32 fold of scale)
    assert_within(unpack33(dw.cpu()), want[1], ref["dw"][1], pixels + 2, "layer dw")
    # d gamma = inv * (dscale - mean * dshift): two products, a subtraction and the fold on top of the two reductions
    T_gamma = inv * (ref["dscale"][1] + mean.double().abs() * ref["dshift"][1])
    assert_within(dgamma.cpu(), want[2], T_gamma, pixels + 4, "layer d gamma")
    assert_within(dbeta.cpu(), want[3], ref["dshift"][1], pixels, "layer d beta")


def test_operators_honour_needs_input_grad(dev):
    from two_stage_object_detection_amd import hip_ops
    g = torch.Generator().manual_seed(2)
    x, w33 = torch.randn(1, 5, 6, 8, generator=g).to(dev), torch.randn(3, 3, 8, generator=g).to(dev)
    sc, sh = torch.randn(8, generator=g).to(dev), torch.randn(8, generator=g).to(dev)
    plain = hip_ops.dwconv3x3_nhwc(x, w33, sc, sh, 2, True)
    assert not plain.requires_grad
    with torch.no_grad():
        assert not hip_ops.dwconv3x3_nhwc(x, w33.clone().requires_grad_(), sc, sh, 2, True).requires_grad
    full = [v.clone().requires_grad_() for v in (x, w33, sc, sh)]
    out = hip_ops.dwconv3x3_nhwc(*full, 2, True)
    assert torch.equal(out.detach(), plain)
    dy = torch.randn(out.shape, generator=g).to(dev)
    all4 = torch.autograd.grad(out, full, dy)
    for keep in ([1], [0, 3], [2]):
        args = [v.clone().requires_grad_(i in keep) for i, v in enumerate((x, w33, sc, sh))]
        o = hip_ops.dwconv3x3_nhwc(*args, 2, True)
        got = torch.autograd.grad(o, [args[i] for i in keep], dy)
        assert all(torch.equal(a, all4[i]) for a, i in zip(got, keep))
        o = hip_ops.dwconv3x3_nhwc(*args, 2, True)
        o.backward(dy)
        assert all((args[i].grad is not None) == (i in keep) for i in range(4))
    # the pair conv
    xp, wp, bp = torch.randn(1, 3, 4, 12, generator=g).to(dev), torch.randn(6, 2, generator=g).to(dev), torch.randn(6, generator=g).to(dev)
    plain = hip_ops.gconv1x1_pair_nhwc(xp, wp, bp)
    args = [xp.clone().requires_grad_(False), wp.clone().requires_grad_(), bp.clone().requires_grad_()]
    o = hip_ops.gconv1x1_pair_nhwc(*args)
    assert torch.equal(o.detach(), plain)
    dyp = torch.randn(o.shape, generator=g).to(dev)
    o.backward(dyp)
    assert args[0].grad is None
    ref = pair_reference(xp.cpu().view(-1, 12), wp.cpu(), dyp.cpu().view(-1, 6))
    assert_within(args[1].grad.cpu(), *ref["dw"], "pair op dw")
    assert_within(args[2].grad.cpu(), *ref["dbias"], "pair op dbias")
