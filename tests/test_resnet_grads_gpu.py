"""tsod_prelu_grad_f32 / tsod_conv3x3_dense_wgrad_f32 and the 3x3 dgrad through the forward conv library
against the float64 restatement of tests/resnet_grads_restated.py.  The bar is section 4.17's: |err| <= (n + 8) 2^-24 T."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resnet_grads_restated import assert_within, conv_stage_reference, prelu_reference  # noqa: E402
from test_resnet_grads_abi import _plan_bytes  # noqa: E402

SLOPE = 0.25


def _away_from_zero(y):
    """test data stays out of a 1e-4 band around y = 0 (the mask must not hang on a rounding)"""
    y[y.abs() < 1e-4] = 0.5
    return y


# ----------------------------------------------------------------------------------------------------------------- PReLU
@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", [(1, 4), (70, 12), (257, 68)])
def test_prelu_grad(dev, rows, C):
    from two_stage_object_detection_amd import hip_ops
    gen = torch.Generator().manual_seed(21 + rows)
    y = _away_from_zero(torch.randn(rows, C, generator=gen))
    if rows == 1:
        y[0, 1] = -0.7                                             # (a negative value for sure)
    dy = torch.randn(rows, C, generator=gen)
    ref = prelu_reference(y, dy, SLOPE)
    g, num = hip_ops.prelu_grad(y.to(dev), dy.to(dev), SLOPE)
    assert_within(g, *ref["g"], f"prelu g {rows}x{C}")
    assert_within(num, ref["dslope_num"][0].reshape(1), ref["dslope_num"][1].reshape(1), ref["dslope_num"][2], f"prelu sum {rows}x{C}")
    g2, num2 = hip_ops.prelu_grad(y.to(dev), dy.to(dev), SLOPE)
    assert torch.equal(g, g2) and torch.equal(num, num2)           # two runs, the same bits
    # no slope sum wanted: the same g, no workspace
    g3, none = hip_ops.prelu_grad(y.to(dev), dy.to(dev), SLOPE, want_dslope=False)
    assert none is None and torch.equal(g3, g)


@pytest.mark.gpu
def test_prelu_grad_offset_pitch_and_planted_zeros(dev):
    """dy is a channel slice of a wider buffer, g goes into the first columns of a wider buffer whose other columns keep their
    bits; an exact y == 0 takes the slope branch and adds nothing to the sum."""
    from two_stage_object_detection_amd import hip_ops
    gen = torch.Generator().manual_seed(22)
    rows, C = 70, 12
    y = _away_from_zero(torch.randn(rows, C, generator=gen))
    y[::3, 1], y[1::5, 7] = 0.0, -0.0
    wide = torch.randn(rows, C + 12, generator=gen)
    dy = wide[:, 8:8 + C].clone()
    pre = torch.randn(rows, C + 8, generator=gen)
    gbuf = pre.clone().to(dev)
    g, num = hip_ops.prelu_grad(y.to(dev), wide.to(dev), SLOPE, dy_off=8, g=gbuf)
    assert g is gbuf
    got = gbuf.cpu()
    assert torch.equal(got[:, C:], pre[:, C:]), "columns beyond C must keep their bits"
    ref = prelu_reference(y, dy, SLOPE)
    assert_within(got[:, :C], *ref["g"], "prelu g (slice)")
    zero = y == 0
    assert torch.equal(got[:, :C][zero], (SLOPE * dy)[zero])       # the slope branch, exactly
    assert_within(num, ref["dslope_num"][0].reshape(1), ref["dslope_num"][1].reshape(1), ref["dslope_num"][2], "prelu sum (slice)")
    # only zeros and positives: the sum is an exact zero
    y2 = y.abs()
    _, num0 = hip_ops.prelu_grad(y2.to(dev), wide.to(dev), SLOPE, dy_off=8)
    assert float(num0) == 0.0
    plain, _ = hip_ops.prelu_grad(y.to(dev), dy.to(dev), SLOPE)
    assert torch.equal(plain.cpu(), got[:, :C])


@pytest.mark.gpu
def test_prelu_grad_refuses_tensors_that_do_not_match(dev):
    """dy and g must hold y's rows and the asked columns: refused on the host, before any launch."""
    from two_stage_object_detection_amd import hip_ops
    y, dy = torch.ones(6, 8, device=dev), torch.ones(6, 12, device=dev)
    for bad in (dict(dy=dy[:5].contiguous()), dict(dy=dy, dy_off=8), dict(dy=dy, dy_off=-4), dict(dy=dy, g=torch.empty(5, 8, device=dev)),
                dict(dy=dy, g=torch.empty(6, 4, device=dev)), dict(dy=dy.double())):
        with pytest.raises(ValueError, match="prelu_grad"):
            hip_ops.prelu_grad(y, bad.pop("dy"), SLOPE, **bad)


# ------------------------------------------------------------------------------------------------------------- 3x3 wgrad
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _wgrad_case(dev, shape, seed, x=None):
    """random g, x, w, scale (both signs) -> the kernel's (dw, dscale, dshift) in torch's layouts and the reference"""
    from two_stage_object_detection_amd import hip_ops
    N, H, W, C, Cout = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen) if x is None else x
    g = torch.randn(N, Cout, H, W, generator=gen)
    w = torch.randn(Cout, C, 3, 3, generator=gen) / (9 * C) ** 0.5
    scale = (torch.rand(Cout, generator=gen) + 0.5) * (torch.randint(0, 2, (Cout,), generator=gen) * 2 - 1)
    ref = conv_stage_reference(x, w, scale, g, 1)
    args = (_nhwc(g).to(dev), _nhwc(x).to(dev), _nhwc(w).to(dev), scale.to(dev))

    def run(**kw):
        dw, dscale, dshift = hip_ops.conv3x3_dense_wgrad(*args, **kw)
        return (None if dw is None else dw.permute(0, 3, 1, 2).contiguous()), dscale, dshift
    return run, ref, args


WGRAD_SHAPES = [
    ((1, 1, 1, 8, 4), (1, 1, 1)),          # only the centre tap is live; M = 1
    ((1, 1, 4, 8, 4), (1, 1, 1)),          # a single row
    ((2, 3, 5, 8, 4), (1, 1, 1)),          # odd W: a row pair straddles image rows and the two images
    ((2, 3, 5, 48, 68), (2, 4, 1)),        # 4 k-tiles whose borders fall inside taps; 2 n-tiles, the second partial
    ((2, 5, 7, 128, 64), (1, 9, 1)),       # one tap per k-tile
    ((2, 13, 17, 8, 4), (1, 1, 4)),        # 4 slices, the last short
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,plan", WGRAD_SHAPES)
def test_conv3x3_dense_wgrad(dev, shape, plan):
    from two_stage_object_detection_amd._ffi import lib
    N, H, W, C, Cout = shape
    want_plan, nbytes = _plan_bytes(N * H * W, Cout, 9 * C)
    assert want_plan == plan and lib().tsod_conv3x3_dense_wgrad_workspace_bytes(N, H, W, C, Cout) == nbytes
    if plan[2] > 1:
        pairs = (N * H * W + 1) // 2
        assert pairs % -(-pairs // plan[2]) != 0                   # the last slice is short
    run, ref, _ = _wgrad_case(dev, shape, seed=31)
    dw, dscale, dshift = run()
    name = "x".join(str(v) for v in shape)
    assert_within(dw, *ref["dw"], f"3x3 wgrad {name} dW")
    assert_within(dscale, *ref["dscale"], f"3x3 wgrad {name} dscale")
    assert_within(dshift, *ref["dshift"], f"3x3 wgrad {name} dshift")
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((dw, dscale, dshift), again))          # two runs, the same bits
    for i, k in enumerate(("want_dw", "want_dscale", "want_dshift")):
        only = run(**{n: n == k for n in ("want_dw", "want_dscale", "want_dshift")})
        assert [t is not None for t in only] == [j == i for j in range(3)] and torch.equal(only[i], (dw, dscale, dshift)[i]), k


@pytest.mark.gpu
def test_conv3x3_dense_wgrad_does_not_read_across_the_batch_border(dev):
    """Image 0 holds 1, image 1 holds 1000, the gradient is nonzero in image 0 only: a tap that leaks from image 0's last rows
    into image 1 (or wraps from a row's end to the next row's start) shows as a value of the wrong size, and exactly: every sum
    here is a sum of g's entries over the pixels whose tap lies inside the image."""
    shape = (2, 3, 5, 8, 4)
    N, H, W, C, Cout = shape
    x = torch.ones(N, C, H, W)
    x[1] = 1000.0
    run, ref, args = _wgrad_case(dev, shape, seed=32, x=x)
    dw, _, _ = run()
    assert_within(dw, *ref["dw"], "3x3 wgrad, constant images")
    from two_stage_object_detection_amd import hip_ops
    g = args[0].clone()
    g[1] = 0.0
    dw0 = hip_ops.conv3x3_dense_wgrad(g, args[1], args[2], torch.ones(Cout, device=dev), want_dscale=False, want_dshift=False)[0]
    g64 = g[0].double().cpu()                                       # [H,W,Cout]
    for kh in range(3):
        for kw in range(3):
            oh = slice(max(0, 1 - kh), min(H, H + 1 - kh))
            ow = slice(max(0, 1 - kw), min(W, W + 1 - kw))
            want = g64[oh, ow].sum((0, 1))                          # image 0's x is 1 everywhere
            got = dw0[:, kh, kw, :].double().cpu()
            assert float((got - want[:, None]).abs().max()) <= 24 * 2.0 ** -24 * float(g64.abs().sum((0, 1)).max()), (kh, kw)


# ------------------------------------------------------------------------------------------------------------- 3x3 dgrad
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 5, 8, 4), (2, 5, 7, 128, 64)])
def test_conv3x3_dgrad_through_the_forward_library(dev, shape):
    from two_stage_object_detection_amd import _ffi, hip_ops
    run, ref, (g, x, w, scale) = _wgrad_case(dev, shape, seed=33)
    assert bool((scale > 0).any()) and bool((scale < 0).any())
    rot = hip_ops.rotate_conv3x3_weight(w, scale)
    N, H, W, C, Cout = shape
    assert tuple(rot.shape) == (C, 3, 3, Cout)
    dx = hip_ops.conv2d_nhwc(g, rot, pad=1, precision=_ffi.PREC_F32)
    assert tuple(dx.shape) == (N, H, W, C)
    assert_within(dx.permute(0, 3, 1, 2), *ref["du"], "3x3 dgrad " + "x".join(str(v) for v in shape))
    assert torch.equal(dx, hip_ops.conv2d_nhwc(g, rot, pad=1, precision=_ffi.PREC_F32))
