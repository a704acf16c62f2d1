"""tsod_conv3x3_strided_wgrad_f32, tsod_prelu_grad_d2s_f32 with the stride-2 3x3 dgrad through the forward conv library, and the
two strided pixel-row kernels against the float64 restatement of tests/resnet_stage_grads_restated.py.
The bar is section 4.17's: |err| <= (n + 8) 2^-24 T."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resnet_stage_grads_restated import assert_within, strided_stage_reference  # noqa: E402

SLOPE = 0.25


def _away_from_zero(y):
    """test data stays out of a 1e-4 band around y = 0 (the mask must not hang on a rounding)"""
    y[y.abs() < 1e-4] = 0.5
    return y


def _nhwc(t, pitch=None, fill=None):
    """NCHW -> contiguous NHWC, optionally into the first columns of a wider pixel whose other columns hold ``fill``."""
    t = t.permute(0, 2, 3, 1).contiguous()
    if pitch is None:
        return t
    wide = torch.full(t.shape[:3] + (pitch,), float("nan") if fill is None else fill)
    wide[..., :t.shape[3]] = t
    return wide


def _wgrad_case(N, H, W, C, Cout, stride, seed):
    gen = torch.Generator().manual_seed(seed)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(N, C, H, W, generator=gen)
    w = torch.randn(Cout, C, 3, 3, generator=gen) * 0.2
    scale = torch.rand(Cout, generator=gen) + 0.5
    g = torch.randn(N, Cout, OH, OW, generator=gen)
    return x, w, scale, g


# odd sizes with two images and channels below a tile; even sizes (the last tap column leaves the image); single pixels; four M
# slices; several K and N tiles
WGRAD_S2 = [(2, 5, 7, 8, 12, False), (2, 5, 7, 8, 12, True), (2, 4, 6, 8, 12, False), (1, 1, 1, 4, 4, False), (1, 2, 2, 4, 4, False),
            (2, 25, 33, 8, 4, False), (1, 5, 7, 48, 68, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,C,Cout,wide", WGRAD_S2)
def test_strided_wgrad_stride_2(dev, N, H, W, C, Cout, wide):
    from two_stage_object_detection_amd import hip_ops
    x, w, scale, g = _wgrad_case(N, H, W, C, Cout, 2, 50 + H * W + C)
    ref = strided_stage_reference(x, w, scale, g, 2, 1)
    xd = _nhwc(x, C + 8 if wide else None).to(dev)                 # (NaN beyond C: a read past the channels would show)
    gd = _nhwc(g, Cout + 4 if wide else None).to(dev)
    wp = w.permute(0, 2, 3, 1).contiguous().to(dev)
    runs = [hip_ops.conv3x3_strided_wgrad(gd, xd, wp, scale.to(dev), stride=2) for _ in range(2)]
    dw, dscale, dshift = runs[0]
    what = f"strided wgrad {N}x{H}x{W}x{C}->{Cout}" + (" wide" if wide else "")
    assert_within(dw.permute(0, 3, 1, 2), *ref["dw"], what + " dw")
    assert_within(dscale, *ref["dscale"], what + " dscale")
    assert_within(dshift, *ref["dshift"], what + " dshift")
    assert all(torch.equal(a, b) for a, b in zip(*runs))           # two runs, the same bits
    only_shift = hip_ops.conv3x3_strided_wgrad(gd, xd, wp, scale.to(dev), stride=2, want_dw=False, want_dscale=False)
    assert only_shift[0] is None and only_shift[1] is None and torch.equal(only_shift[2], dshift)


@pytest.mark.gpu
def test_strided_wgrad_stride_1_has_the_dense_entry_points_bits(dev):
    from two_stage_object_detection_amd import hip_ops
    x, w, scale, g = _wgrad_case(2, 5, 7, 8, 12, 1, 61)
    args = (_nhwc(g).to(dev), _nhwc(x).to(dev), w.permute(0, 2, 3, 1).contiguous().to(dev), scale.to(dev))
    old = hip_ops.conv3x3_dense_wgrad(*args)
    new = hip_ops.conv3x3_strided_wgrad(*args, stride=1)
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    ref = strided_stage_reference(x, w, scale, g, 1, 1)
    assert_within(new[0].permute(0, 3, 1, 2), *ref["dw"], "strided wgrad stride 1 dw")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [8, 68])
@pytest.mark.parametrize("H,W", [(5, 7), (4, 6), (1, 1), (2, 2), (25, 33)])
def test_stride_2_dgrad_through_the_phase_pack_and_prelu_grad_d2s(dev, H, W, C):
    """g1 = d1 m(y1) and sum d1 y1 [y1 < 0] with d1 the stride-2 3x3's input gradient: the forward conv library on the 2x2 phase
    pack, then the gathering mask pass; d1 itself is never written."""
    from two_stage_object_detection_amd import _ffi, hip_ops
    N, Cout = 2, 12
    x, w, scale, g2 = _wgrad_case(N, H, W, C, Cout, 2, 70 + H * W + C)
    gen = torch.Generator().manual_seed(71)
    y1 = _away_from_zero(torch.randn(N, C, H, W, generator=gen))
    y1[0, 1, 0, 0] = -0.7                                          # (a negative value for sure)
    du, duT, n_du = strided_stage_reference(x, w, scale, g2, 2, 1)["du"]
    m = torch.where(y1.double() > 0, 1.0, SLOPE)
    neg = (y1 < 0).double()
    pack = hip_ops.s2d_conv3x3_weight(w.permute(0, 2, 3, 1).contiguous().to(dev), scale.to(dev))
    assert tuple(pack.shape) == (4 * C, 2, 2, Cout)
    P = hip_ops.conv2d_nhwc(_nhwc(g2).to(dev), pack, pad=1, precision=_ffi.PREC_F32)
    assert tuple(P.shape) == (N, (H - 1) // 2 + 2, (W - 1) // 2 + 2, 4 * C)
    yd = _nhwc(y1).to(dev)
    g1, num = hip_ops.prelu_grad_d2s(yd, P, SLOPE)
    what = f"s2 dgrad {N}x{H}x{W}x{C}"
    assert_within(g1.permute(0, 3, 1, 2), du * m, duT * m, n_du + 1, what + " g1")
    terms = du * y1.double() * neg
    assert_within(num, terms.sum().reshape(1), (duT * y1.double().abs() * neg).sum().reshape(1), n_du + 1 + int(neg.sum()) + 1,
                  what + " slope sum")
    g1b, numb = hip_ops.prelu_grad_d2s(yd, P, SLOPE)
    assert torch.equal(g1, g1b) and torch.equal(num, numb)         # two runs, the same bits
    g1c, none = hip_ops.prelu_grad_d2s(yd, P, SLOPE, want_dslope=False)
    assert none is None and torch.equal(g1c, g1)                   # with and without the slope sum: the same g
    # the gathered d1 written out by the plain mask pass at slope 1 is what the d2s pass read: the same sum order, the same bits
    d1, _ = hip_ops.prelu_grad_d2s(yd, P, 1.0, want_dslope=False)
    g1d, numd = hip_ops.prelu_grad(yd, d1, SLOPE)
    assert torch.equal(g1d, g1) and torch.equal(numd, num)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("H,W", [(5, 7), (4, 6)])
def test_pixel_subsample_and_upsample_add(dev, H, W, stride):
    from two_stage_object_detection_amd import hip_ops
    gen = torch.Generator().manual_seed(80 + H + stride)
    N, C, P = 2, 8, 20
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(N, H, W, P, generator=gen)
    xs = hip_ops.pixel_subsample(x.to(dev), stride, C=C)
    assert tuple(xs.shape) == (N, OH, OW, C) and torch.equal(xs.cpu(), x[:, ::stride, ::stride, :C])
    full = hip_ops.pixel_subsample(x.to(dev), stride)
    assert torch.equal(full.cpu(), x[:, ::stride, ::stride, :].contiguous())
    d = torch.randn(N, OH, OW, C + 4, generator=gen)
    dx = hip_ops.pixel_upsample_add(x.to(dev), d.to(dev), stride, C=C)
    want = x.clone()
    want[:, ::stride, ::stride, :C] += d[..., :C]                  # one f32 add per touched element, dx the first operand
    assert torch.equal(dx.cpu(), want)                             # (every untouched pixel and column keeps its bits)
    touched = torch.zeros(N, H, W, P, dtype=torch.bool)
    touched[:, ::stride, ::stride, :C] = True
    assert int(touched.sum()) == N * OH * OW * C and torch.equal(dx.cpu()[~touched], x[~touched])
