"""tsod_conv3x3_wgrad_f32 against float64 autograd on the CPU from the same f32 inputs
(tests/stem_grads_restated.py).  The bar: |err| <= (n + 8) 2^-24 T elementwise, n = the number of summed products, T = the
same graph on absolute values.  Inputs are drawn so that no pre-activation lies within 1e-4 of 0 or 6."""
import functools
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stem_grads_restated import assert_within, conv3x3_layer_reference  # noqa: E402

#        N, H,   W,   cout_pad, cout_real, stride
CASES = {"2x13x18": (2, 13, 18, 24, 24, 2),            # odd H, even W: the bottom pad row is used, the right one is not
         "1x8x7": (1, 8, 7, 32, 32, 2),
         "2x9x9_s1": (2, 9, 9, 48, 48, 1),
         "2x151x201": (2, 151, 201, 24, 24, 2),        # 152 output rows, 6 per slice: 26 slices, the last one of 2 rows
         "2x13x18_pad": (2, 13, 18, 24, 22, 2)}        # two pad rows in the weight
SLICES = {"2x13x18": 1, "1x8x7": 1, "2x9x9_s1": 1, "2x151x201": 26, "2x13x18_pad": 1}


@functools.lru_cache(maxsize=None)
def case(name):
    """The CPU side of a case, made once: f32 inputs in torch's layouts, the saved output, and the float64 reference."""
    N, H, W, cp, cr, s = CASES[name]
    g = torch.Generator().manual_seed(len(name) * 1000 + H)
    x = torch.randn(N, 3, H, W, generator=g) * 1.5
    w = torch.randn(cr, 3, 3, 3, generator=g) * 0.4
    scale = torch.rand(cr, generator=g) + 0.5
    shift = torch.randn(cr, generator=g) * 0.5 + 1.5
    for _ in range(100):                                       # redraw the centre pixel of every patch too close to 0 or 6
        z = F.conv2d(x.double(), w.double(), None, s, 1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        bad = ((z.abs() < 1e-4) | ((z - 6).abs() < 1e-4)).any(1).nonzero()
        if not len(bad):
            break
        x[bad[:, 0], :, bad[:, 1] * s, bad[:, 2] * s] = torch.randn(len(bad), 3, generator=g) * 1.5
    else:
        raise AssertionError("could not keep the pre-activations away from 0 and 6")
    y = z.clamp(0, 6).float()
    assert int((y == 0).sum()) > 0 and int((y == 6).sum()) > 0 and int(((y > 0) & (y < 6)).sum()) > 0
    dy = torch.randn(y.shape, generator=g)
    ref = conv3x3_layer_reference(x, w, scale, shift, y, dy, s)
    return dict(x=x, w=w, scale=scale, shift=shift, y=y, dy=dy, ref=ref, junk=torch.randn(N, y.shape[2], y.shape[3], cp, generator=g))


def device_inputs(name, dev, pad_value=0.0):
    N, H, W, cp, cr, s = CASES[name]
    c = case(name)
    x4 = torch.full((N, H, W, 4), pad_value)
    x4[..., :3] = c["x"].permute(0, 2, 3, 1)
    w4 = torch.zeros(cp, 3, 3, 4)
    w4[:cr, :, :, :3] = c["w"].permute(0, 2, 3, 1)
    sc = torch.ones(cp)
    sc[:cr] = c["scale"]
    y, dy = c["junk"].clone() + 2.0, c["junk"].clone()         # the pad channels hold something: they must not matter
    y[..., :cr], dy[..., :cr] = c["y"].permute(0, 2, 3, 1), c["dy"].permute(0, 2, 3, 1)
    return [t.contiguous().to(dev) for t in (x4, w4, sc, y, dy)]


def run(name, dev, tensors=None, **kw):
    from two_stage_object_detection_amd import hip_ops
    N, H, W, cp, cr, s = CASES[name]
    x4, w4, sc, y, dy = device_inputs(name, dev) if tensors is None else tensors
    return hip_ops.conv3x3_bn_relu6_grad(x4, w4, sc, y, dy, stride=s, cout=cr, **kw)


def check_against_reference(name, outs):
    worst = {}
    for key, got in zip(("dw", "dscale", "dshift"), outs):
        g, T, n = case(name)["ref"][key]
        assert_within(got, g, T, n, f"{name} {key}")
        worst[key] = float(((got.double().cpu() - g).abs() / ((n + 8) * 2.0 ** -24 * T).clamp_min(1e-300)).max())
    print(f"conv3x3_wgrad {name}: largest err / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gradients_match_f64_pad_is_zero_and_runs_are_bit_equal(dev, name):
    from two_stage_object_detection_amd import _ffi
    N, H, W, cp, cr, s = CASES[name]
    tiles = (cp + 31) // 32
    assert _ffi.lib().tsod_conv3x3_wgrad_workspace_bytes(N, H, W, cp, s) == SLICES[name] * tiles * 32 * 33 * 4
    outs = run(name, dev)
    assert outs[0].shape == (cr, 3, 3, 3) and outs[1].shape == (cr,) and outs[2].shape == (cr,)
    check_against_reference(name, outs)
    raw = run(name, dev, raw=True)
    assert raw[0].shape == (cp, 3, 3, 4) and not bool(raw[0][..., 3].any()) and not bool(raw[0][cr:].any())
    assert not bool(raw[1][cr:].any()) and not bool(raw[2][cr:].any())
    assert torch.equal(raw[0][:cr, :, :, :3].permute(0, 3, 1, 2), outs[0]) and torch.equal(raw[1][:cr], outs[1])
    again = run(name, dev)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["2x13x18", "2x151x201"])
def test_dy_with_a_wider_pitch_and_a_channel_offset(dev, name):
    from two_stage_object_detection_amd import hip_ops
    N, H, W, cp, cr, s = CASES[name]
    x4, w4, sc, y, dy = device_inputs(name, dev)
    wide = torch.randn(dy.shape[:3] + (cp + 12,), generator=torch.Generator().manual_seed(1)).to(dev)
    wide[..., 8:8 + cp] = dy
    got = hip_ops.conv3x3_bn_relu6_grad(x4, w4, sc, y, wide, stride=s, cout=cr, dy_off=8)
    assert all(torch.equal(a, b) for a, b in zip(got, run(name, dev)))


@pytest.mark.gpu
def test_nan_in_the_pad_channel_of_x4_reaches_nothing(dev):
    name = "2x13x18_pad"
    outs = run(name, dev, device_inputs(name, dev, pad_value=float("nan")), raw=True)
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    assert all(torch.equal(a, b) for a, b in zip(outs, run(name, dev, raw=True)))
    cr = CASES[name][4]
    check_against_reference(name, (outs[0][:cr, :, :, :3].permute(0, 3, 1, 2), outs[1][:cr], outs[2][:cr]))


@pytest.mark.gpu
def test_outputs_of_exactly_0_and_exactly_6_contribute_nothing(dev):
    """Pixels whose saved output is set to exactly 0 or 6 drop out: the result is bit-equal to the one with dy zeroed there, and
    within the bar of the reference fed the same saved output."""
    name = "2x13x18"
    x4, w4, sc, y, dy = device_inputs(name, dev)
    c = case(name)
    open_ = ((c["y"] > 0) & (c["y"] < 6)).permute(0, 2, 3, 1).nonzero()
    pick = open_[:: max(1, len(open_) // 40)]
    n, oh, ow, o = pick.t().to(dev)
    y2, dy2 = y.clone(), dy.clone()
    y2[n[0::2], oh[0::2], ow[0::2], o[0::2]] = 0.0
    y2[n[1::2], oh[1::2], ow[1::2], o[1::2]] = 6.0
    dy2[n, oh, ow, o] = 1000.0                                  # would be seen at once
    got = run(name, dev, (x4, w4, sc, y2, dy2))
    dy3 = dy2.clone()
    dy3[n, oh, ow, o] = 0.0
    assert all(torch.equal(a, b) for a, b in zip(got, run(name, dev, (x4, w4, sc, y2, dy3))))
    ref = conv3x3_layer_reference(c["x"], c["w"], c["scale"], c["shift"], y2.cpu().permute(0, 3, 1, 2), dy2.cpu().permute(0, 3, 1, 2), 2)
    for key, t in zip(("dw", "dscale", "dshift"), got):
        assert_within(t, *ref[key], f"saturated {key}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["2x9x9_s1", "2x151x201"])
def test_every_want_combination_is_bit_equal_to_the_all_wanted_run(dev, name):
    tensors = device_inputs(name, dev)
    full = run(name, dev, tensors)
    for want in itertools.product((False, True), repeat=3):
        if not any(want):
            with pytest.raises(ValueError):
                run(name, dev, tensors, want_dw=False, want_dscale=False, want_dshift=False)
            continue
        got = run(name, dev, tensors, want_dw=want[0], want_dscale=want[1], want_dshift=want[2])
        for wanted, a, b in zip(want, got, full):
            assert (a is None) if not wanted else torch.equal(a, b), want
