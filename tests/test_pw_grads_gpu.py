"""tsod_relu6_grad_mask_f32 / tsod_pw_wgrad_f32 / tsod_pw_dgrad_f32 / tsod_dwconv3x3_grad_act_f32
against the float64 restatement of tests/pw_grads_restated.py.  The bar is section 4.17's: |err| <= (n + 8) 2^-24 T elementwise."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_grads_restated import assert_within, conv_layer_reference  # noqa: E402


def _pad4(c):
    return (c + 3) // 4 * 4


class Case:
    """One ConvLayer on an NHWC buffer: x [N,H,W,pitch] with real-width segments at ``offs`` (pad channels zero, like a block
    buffer), w gathered to the padded segments, y = the layer's output in f32 (computed on the CPU), moved out of the 1e-4 bands
    next to 0 and 6 so that the mask does not hang on a rounding."""

    def __init__(self, dev, shape, reals, offs, pitch, cout, seed):
        g = torch.Generator().manual_seed(seed)
        N, H, W = shape
        self.M, self.reals, self.offs, self.pitch, self.cout, self.cp = N * H * W, reals, offs, pitch, cout, _pad4(cout)
        self.segs = [(o, _pad4(r)) for o, r in zip(offs, reals)]
        x = torch.randn(N, H, W, pitch, generator=g)
        keep = torch.zeros(pitch, dtype=torch.bool)
        for o, r in zip(offs, reals):
            keep[o:o + r] = True
        for o, ln in self.segs:                                  # pad channels of a slice hold zeros; the rest is foreign data
            x[..., o:o + ln] *= keep[o:o + ln]
        K = sum(reals)
        self.w = torch.randn(cout, K, generator=g) / K ** 0.5
        self.scale = (torch.rand(cout, generator=g) + 0.5) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1)
        self.shift = torch.randn(cout, generator=g) + 1.5
        self.xg = torch.cat([x[..., o:o + r] for o, r in zip(offs, reals)], -1).reshape(self.M, K)
        y = torch.clamp((self.xg @ self.w.t()) * self.scale + self.shift, 0, 6)
        near = ((y > 0) & (y < 1e-4)) | ((y < 6) & (y > 6 - 1e-4))
        y[near] = 0.5
        self.y = y
        self.dy = torch.randn(self.M, cout, generator=g)
        wg = torch.zeros(self.cp, sum(ln for _, ln in self.segs))
        k0 = c0 = 0
        for (o, ln), r in zip(self.segs, reals):
            wg[:cout, k0:k0 + r] = self.w[:, c0:c0 + r]
            k0, c0 = k0 + ln, c0 + r
        pad = lambda t, fill=0.0: torch.cat([t, torch.full((self.M, self.cp - cout), fill)], 1) if t.dim() == 2 else \
            torch.cat([t, torch.zeros(self.cp - cout)])
        self.d = dict(x=x.to(dev), w=wg.to(dev), scale=pad(self.scale).to(dev), y=pad(y).view(N, H, W, self.cp).to(dev),
                      dy=pad(self.dy, 1.0).view(N, H, W, self.cp).to(dev))   # (pad columns of dy: anything - y is 0 there)
        self.prefill = torch.randn(N, H, W, pitch, generator=g)

    def run(self, y=None, dy=None, **kw):
        from two_stage_object_detection_amd import hip_ops
        d = self.d
        dx = self.prefill.to(d["x"].device) if kw.get("want_dx", True) else None
        out = hip_ops.conv1x1_bn_relu6_grad(d["x"], self.segs, d["w"], d["scale"], d["y"] if y is None else y,
                                            d["dy"] if dy is None else dy, seg_real=self.reals, cout=self.cout, dx=dx,
                                            accumulate=True, **kw)
        return [None if t is None else t.cpu() for t in out]

    def check(self, name):
        dx, dw, dscale, dshift = self.run()
        ref = conv_layer_reference(self.xg, self.w, self.scale, self.shift, self.y, self.dy)
        assert_within(dw, ref["dw"][0], ref["dw"][1], ref["dw"][2], f"{name} dW")
        assert_within(dscale, *ref["dscale"], f"{name} dscale")
        assert_within(dshift, *ref["dshift"], f"{name} dshift")
        g, T, n = ref["dx"]
        flat, pre = dx.reshape(self.M, self.pitch), self.prefill.reshape(self.M, self.pitch)
        touched = torch.zeros(self.pitch, dtype=torch.bool)
        c0 = 0
        for (o, ln), r in zip(self.segs, self.reals):
            assert_within(flat[:, o:o + r], pre[:, o:o + r].double() + g[:, c0:c0 + r], pre[:, o:o + r].abs().double() + T[:, c0:c0 + r],
                          n + 1, f"{name} dx segment at {o}")
            assert bool((flat[:, o + r:o + ln] == 0).all()), "pad channels of dx must be exact zeros"
            touched[o:o + ln] = True
            c0 += r
        assert torch.equal(flat[:, ~touched], pre[:, ~touched]), "columns between the segments must keep their bits"
        return dx, dw, dscale, dshift


@pytest.fixture(scope="module")
def small(dev):
    return Case(dev, (2, 5, 7), [10, 6], [0, 20], 40, 6, seed=11)


@pytest.mark.gpu
def test_small_with_padding_and_a_hole(small):
    assert small.segs == [(0, 12), (20, 8)] and small.cp == 8 and small.M == 70
    small.check("small")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["layer4", "transition"])
def test_last_block_extremes_at_few_pixels(dev, which):
    """HarDNet-39's last HarDBlock (slices 640 | 160 | 256 | 160 | 410) at 2 x 19 x 23 pixels, in a pitch-1668 buffer."""
    from two_stage_object_detection_amd.models.hardnet import HarDBlock
    blk = HarDBlock(640, 160, 1.6, 4, dwconv=True)
    real, offs, P = blk.slice_table()
    assert real == [640, 160, 256, 160, 410] and P <= 1668
    slices, cout = (blk.links[3], 410) if which == "layer4" else (blk.output_slices(), 1024)
    assert [real[k] for k in slices] == ([160, 256, 640] if which == "layer4" else [160, 160, 410])
    Case(dev, (2, 19, 23), [real[k] for k in slices], [offs[k] for k in slices], 1668, cout, seed=12).check(which)


@pytest.mark.gpu
def test_mask_edges_give_zero_gradient(small):
    """Exact 0.0 and exact 6.0 in the saved output: nothing flows (strict comparisons), whatever dy holds there."""
    y = small.d["y"].clone().view(small.M, small.cp)
    planted = torch.zeros_like(y, dtype=torch.bool)
    planted[::3, 1], planted[1::5, 4] = True, True
    y[::3, 1], y[1::5, 4] = 0.0, 6.0
    dy = torch.where(planted, small.d["dy"].view(small.M, small.cp), torch.zeros_like(y))
    dx, dw, dscale, dshift = small.run(y=y.view_as(small.d["y"]), dy=dy.view_as(small.d["dy"]))
    assert not dw.any() and not dscale.any() and not dshift.any()
    flat, pre = dx.reshape(small.M, -1), small.prefill.reshape(small.M, -1)
    for (o, ln), r in zip(small.segs, small.reals):
        assert torch.equal(flat[:, o:o + r], pre[:, o:o + r])
    # and planted among live values: the f64 statement with the same saved output agrees
    y2 = small.d["y"].clone().view(small.M, small.cp)
    y2[::3, 1], y2[1::5, 4] = 0.0, 6.0
    got = small.run(y=y2.view_as(small.d["y"]))
    ref = conv_layer_reference(small.xg, small.w, small.scale, small.shift, y2[:, :small.cout].cpu(), small.dy)
    assert_within(got[1], *ref["dw"], "planted dW")
    assert_within(got[3], *ref["dshift"], "planted dshift")


@pytest.mark.gpu
def test_want_switches_and_determinism(small):
    full = small.run()
    again = small.run()
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    names = ("want_dx", "want_dw", "want_dscale", "want_dshift")
    for i, name in enumerate(names):
        only = small.run(**{k: k == name for k in names})
        assert [t is not None for t in only] == [k == name for k in names]
        assert torch.equal(only[i], full[i]), name
    # a segment nobody needs is skipped: its columns keep their bits, the other segment's are the all-on call's
    from two_stage_object_detection_amd import hip_ops
    d = small.d
    dx = small.prefill.to(d["x"].device)
    hip_ops.conv1x1_bn_relu6_grad(d["x"], small.segs, d["w"], d["scale"], d["y"], d["dy"], seg_real=small.reals, seg_want=[True, False],
                                  cout=small.cout, dx=dx, accumulate=True, want_dw=False, want_dscale=False, want_dshift=False)
    dx = dx.cpu()
    assert torch.equal(dx[..., 12:], small.prefill[..., 12:]) and torch.equal(dx[..., :12], full[0][..., :12])


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
def test_fused_mask_of_the_depthwise_backward(dev, stride):
    """tsod_dwconv3x3_grad_act_f32: dx = tsod_dwconv3x3_grad_f32's dx times [0 < x < 6], the parameter gradients bit for bit."""
    from two_stage_object_detection_amd import hip_ops
    g = torch.Generator().manual_seed(13)
    N, H, W, C = 2, 9, 11, 12
    x = torch.clamp(torch.randn(N, H, W, C, generator=g) * 3 + 3, 0, 6).to(dev)        # a ReLU6 output: exact 0 and 6 occur
    assert bool((x == 0).any()) and bool((x == 6).any())
    w = torch.randn(3, 3, C, generator=g).to(dev)
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn(N, OH, OW, C, generator=g).to(dev)
    plain = hip_ops.dwconv3x3_grad(x, w, sc, sh, stride, False, dy)
    fused = hip_ops.dwconv3x3_grad(x, w, sc, sh, stride, False, dy, act_dx=True)
    mask = ((x > 0) & (x < 6)).float()
    assert torch.equal(fused[0], plain[0] * mask)
    assert all(torch.equal(a, b) for a, b in zip(fused[1:], plain[1:]))
    # dy read as a channel slice of a wider buffer, and the standalone mask pass says the same
    wide = torch.randn(N, OH, OW, C + 8, generator=g).to(dev)
    wide[..., 4:4 + C] = dy
    sliced = hip_ops.dwconv3x3_grad(x, w, sc, sh, stride, False, wide, dy_off=4, act_dx=True)
    assert all(torch.equal(a, b) for a, b in zip(sliced, fused))
    if stride == 1:
        assert torch.equal(hip_ops.relu6_grad_mask(x, wide, 4), dy * mask)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,segs,pitch,slices", [
    (999, 40, [(0, 72)], 72, 8),                       # one tile, a ragged last row pair, N and K short of the tile
    (2001, 100, [(0, 100), (160, 132)], 296, 16),      # 2 x 2 tiles, a k-tile that straddles the hole (the operand cap: 20)
])
def test_wgrad_tile_is_one_tile_for_both_entry_points(dev, M, N, segs, pitch, slices):
    """tsod_pw_wgrad_f32 (scale = 1, an already masked gradient) and tsod_wgrad_f32 on the contiguous gathered X run the same
    tile (csrc/grad_reduce.h) over the same slices: dW and dshift / db are equal bit for bit.  Columns outside the segments
    hold NaN: they are never read."""
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd._ffi import lib
    gen = torch.Generator().manual_seed(14)
    K = sum(ln for _, ln in segs)
    x = torch.full((M, pitch), float("nan"))
    for o, ln in segs:
        x[:, o:o + ln] = torch.randn(M, ln, generator=gen)
    xg = torch.cat([x[:, o:o + ln] for o, ln in segs], 1).contiguous()
    g = torch.randn(M, N, generator=gen)
    w = torch.randn(N, K, generator=gen)
    n_pad, k_pad = -(-N // 64) * 64, -(-K // 128) * 128
    assert lib().tsod_pw_wgrad_workspace_bytes(M, N, K) == lib().tsod_wgrad_workspace_bytes(M, N, K) \
        == slices * n_pad * (k_pad + 1) * 4, "both entry points must cut M into the same slices"
    _, dw, _, dshift = hip_ops.conv1x1_bn_relu6_grad(x.to(dev), segs, w.to(dev), torch.ones(N, device=dev), None, g.to(dev),
                                                     want_dx=False)
    dw0, db0 = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
    hip_ops.wgrad(g.to(dev), xg.to(dev), dw0, db0)
    assert torch.isfinite(dw).all() and torch.isfinite(dshift).all()
    assert torch.equal(dw, dw0), "dW"
    assert torch.equal(dshift, db0), "dshift / db0"
