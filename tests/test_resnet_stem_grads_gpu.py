"""tsod_prelu_grad_pool_f32 and tsod_conv7x7s2_wgrad_f32 against the float64 restatement of
tests/resnet_stem_grads_restated.py, from the same f32 inputs.  The bar is section 4.17's: |err| <= (n + 8) 2^-24 T."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resnet_stem_grads_restated import assert_within, prelu_pool_reference, strided_stage_reference  # noqa: E402
from test_resnet_stem_grads_abi import stem7_slices  # noqa: E402

SLOPE = 0.25

# single pixels and windows, odd and even sizes (the last window clipped or not), channels below and at the stem's 64, and a shape
# whose slope sum has more than one partial (280 workgroups) and more than 256 of them (the finish's second round)
POOL_SHAPES = [(1, 1, 1, 4), (2, 2, 2, 8), (1, 5, 7, 64), (2, 4, 6, 64), (1, 31, 47, 64), (1, 33, 9, 12), (2, 40, 56, 64)]


def _nhwc(t, pitch=None):
    """NCHW -> contiguous NHWC, optionally into the first columns of a wider pixel whose other columns hold NaN."""
    t = t.permute(0, 2, 3, 1).contiguous()
    if pitch is None:
        return t
    wide = torch.full(t.shape[:3] + (pitch,), float("nan"))
    wide[..., :t.shape[3]] = t
    return wide


def _pool_case(N, OH, OW, C, seed, integer=False):
    gen = torch.Generator().manual_seed(seed)
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    if integer:
        return (torch.randint(-2, 3, (N, C, OH, OW), generator=gen).float(), torch.randint(-3, 4, (N, C, PH, PW), generator=gen).float())
    y = torch.randn(N, C, OH, OW, generator=gen)
    y[y.abs() < 1e-4] = 0.5                                        # (the mask must not hang on a rounding)
    y.view(-1)[0] = -0.7                                           # (a negative value for sure)
    return y, torch.randn(N, C, PH, PW, generator=gen)


@pytest.mark.gpu
@pytest.mark.parametrize("N,OH,OW,C", POOL_SHAPES)
def test_prelu_grad_pool_random(dev, N, OH, OW, C):
    from two_stage_object_detection_amd import hip_ops
    y, dp = _pool_case(N, OH, OW, C, 100 + OH * OW + C)
    ref = prelu_pool_reference(y, dp, SLOPE)
    what = f"prelu_grad_pool {N}x{OH}x{OW}x{C}"
    yd, dpd = _nhwc(y).to(dev), _nhwc(dp).to(dev)
    g, num = hip_ops.prelu_grad_pool(yd, dpd, SLOPE)
    assert_within(g.permute(0, 3, 1, 2), *ref["g"], what + " g")
    assert_within(num, ref["dslope_num"][0].reshape(1), ref["dslope_num"][1].reshape(1), ref["dslope_num"][2], what + " slope sum")
    g2, num2 = hip_ops.prelu_grad_pool(yd, dpd, SLOPE)
    assert torch.equal(g, g2) and torch.equal(num, num2)           # two runs, the same bits
    g3, none = hip_ops.prelu_grad_pool(yd, dpd, SLOPE, want_dslope=False)
    assert none is None and torch.equal(g3, g)                     # without the slope sum: the same g
    # every operand in a wider pixel (NaN beyond C: a read past the channels would show; g's other columns are not written)
    gw = torch.full((N, OH, OW, C + 4), float("nan"), device=dev)
    g4, num4 = hip_ops.prelu_grad_pool(_nhwc(y, C + 4).to(dev), _nhwc(dp, C + 8).to(dev), SLOPE, C=C, g=gw)
    assert g4 is gw and torch.equal(gw[..., :C], g) and bool(torch.isnan(gw[..., C:]).all()) and torch.equal(num4, num)
    # the gathered dy written out by this pass at slope 1, then the plain mask pass: the same grid rule and sum order, the same bits
    dy, _ = hip_ops.prelu_grad_pool(yd, dpd, 1.0, want_dslope=False)
    g5, num5 = hip_ops.prelu_grad(yd, dy, SLOPE)
    assert torch.equal(g5, g) and torch.equal(num5, num)


@pytest.mark.gpu
@pytest.mark.parametrize("N,OH,OW,C", POOL_SHAPES)
def test_prelu_grad_pool_gives_every_tie_to_the_first_maximum_exactly(dev, N, OH, OW, C):
    """Integer y in -2 .. 2 (ties in nearly every window, exact zeros among them), integer dp, slope 0.25: every sum is exact in
    f32, so the result must equal the float64 restatement - which tests/test_resnet_stem_grads_abi.py holds to autograd's own tie
    handling - bit for bit."""
    from two_stage_object_detection_amd import hip_ops
    y, dp = _pool_case(N, OH, OW, C, 200 + OH * OW + C, integer=True)
    ref = prelu_pool_reference(y, dp, SLOPE)
    g, num = hip_ops.prelu_grad_pool(_nhwc(y).to(dev), _nhwc(dp).to(dev), SLOPE)
    assert torch.equal(g.permute(0, 3, 1, 2).double().cpu(), ref["g"][0])
    assert float(num) == float(ref["dslope_num"][0])


# images smaller than the kernel, odd and even sizes, clipped taps on all four sides; by the shipped slice rule (1, 64, 96) has 12
# full slices, (2, 61, 93) 24 with a short last one, (2, 16, 12) and the smaller ones a single slice
WGRAD_SHAPES = [(1, 1, 1), (1, 2, 3), (1, 7, 9), (2, 16, 12), (3, 33, 25), (1, 64, 96), (2, 61, 93)]


def _wgrad_case(N, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.randn(N, 3, H, W, generator=gen)
    w = torch.randn(64, 3, 7, 7, generator=gen) * 0.1
    scale = torch.rand(64, generator=gen) + 0.5
    g = torch.randn(N, 64, OH, OW, generator=gen)
    wp = torch.zeros(64, 7, 8, 4)
    wp[:, :, :7, :3] = w.permute(0, 2, 3, 1)                       # the forward's f32 pack
    x4 = torch.zeros(N, H, W, 4)
    x4[..., :3] = x.permute(0, 2, 3, 1)
    return x, w, scale, g, wp, x4


def test_the_wgrad_shapes_cover_the_slice_rule():
    assert stem7_slices(2, 61, 93) == (24, 64, 16) and stem7_slices(1, 64, 96) == (12, 64, 64)
    assert [stem7_slices(*s)[0] for s in WGRAD_SHAPES[:4]] == [1, 1, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", WGRAD_SHAPES)
def test_conv7x7s2_wgrad(dev, N, H, W):
    from two_stage_object_detection_amd import hip_ops
    x, w, scale, g, wp, x4 = _wgrad_case(N, H, W, 300 + H * W)
    ref = strided_stage_reference(x, w, scale, g, 2, 3)
    what = f"conv7x7s2 wgrad {N}x{H}x{W}"
    gd, xd, wd, sd = _nhwc(g).to(dev), x4.to(dev), wp.to(dev), scale.to(dev)
    runs = [hip_ops.conv7x7s2_wgrad(gd, xd, wd, sd) for _ in range(2)]
    dw, dscale, dshift = runs[0]
    assert tuple(dw.shape) == (64, 3, 7, 7)
    assert_within(dw, *ref["dw"], what + " dw")
    assert_within(dscale, *ref["dscale"], what + " dscale")
    assert_within(dshift, *ref["dshift"], what + " dshift")
    assert all(torch.equal(a, b) for a, b in zip(*runs))           # two runs, the same bits
    # each output asked for alone: the bits it has when all three are asked for
    for i, kw in enumerate((dict(want_dscale=False, want_dshift=False), dict(want_dw=False, want_dshift=False),
                            dict(want_dw=False, want_dscale=False))):
        alone = hip_ops.conv7x7s2_wgrad(gd, xd, wd, sd, **kw)
        assert [a is None for a in alone] == [j != i for j in range(3)] and torch.equal(alone[i], runs[0][i])
    # the kernel's own layout: the pack's, with exact zeros in the padding
    raw = hip_ops.conv7x7s2_wgrad(gd, xd, wd, sd, raw=True)[0]
    assert tuple(raw.shape) == (64, 7, 8, 4) and torch.equal(raw[:, :, :7, :3].permute(0, 3, 1, 2), dw)
    assert not bool(raw[:, :, 7, :].any()) and not bool(raw[..., 3].any())
    # NaN in the image's pad channel and g in a wider pixel (NaN beyond 64) change nothing
    xn = xd.clone()
    xn[..., 3] = float("nan")
    again = hip_ops.conv7x7s2_wgrad(_nhwc(g, 72).to(dev), xn, wd, sd)
    assert all(torch.equal(a, b) for a, b in zip(again, runs[0]))


@pytest.mark.gpu
def test_conv7x7s2_wgrad_refuses_other_channel_counts(dev):
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd._ffi import TsodError
    x, w, scale, g, wp, x4 = _wgrad_case(1, 7, 9, 400)
    with pytest.raises(TsodError):
        hip_ops.conv7x7s2_wgrad(_nhwc(g[:, :32]).to(dev), x4.to(dev), wp[:32].contiguous().to(dev), scale[:32].to(dev))
