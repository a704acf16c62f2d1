"""Every size-selected variant of the streaming layer kernels (csrc/pool_layout.hip) against the float64 restatements of
tests/layer_kernels_restated.py, with the derived bars stated there: the seven depthwise patch shapes at ragged edges and
in the channel-slice form the HarDNet plan uses, the grid-stride trips of the pair conv, the grouped 3x3 and absmax, the
max pool on both sides of its banded switch, and the layout kernels' offsets and pads.

The largest err / bar of each kernel and variant is printed; with TSOD_LAYER_KERNELS_JSONL=<path> the same figures are
appended to that file, one JSON line each (TSOD_LAYER_KERNELS_COMMIT names the commit in them)."""
import functools
import json
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_kernels_restated as R  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25          # what the channels around an output slice hold before a launch, and must hold after it
FAR = 1.0e6               # what the channels around an input slice hold: one wrong channel read cannot stay inside a bar
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -2     # include/tsod.h


@pytest.fixture(scope="module")
def ops():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def ffi():
    from two_stage_object_detection_amd import _ffi
    return _ffi


def record(kernel, variant, shape, ratio):
    """Print one kernel's largest err / bar at one shape, and append it to the JSON lines file when one is asked for."""
    line = {"kernel": kernel, "variant": variant, "shape": shape, "max_err_over_bar": round(float(ratio), 4),
            "commit": os.environ.get("TSOD_LAYER_KERNELS_COMMIT", "unknown")}
    print("layer_kernels:", json.dumps(line))
    path = os.environ.get("TSOD_LAYER_KERNELS_JSONL")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def within(got, y, T, bar):
    """(every |got - y| <= bar T, the largest |got - y| / (bar T)) for a device or host f32 result against f64 y, T."""
    err = (got.detach().cpu().double() - y).abs()
    lim = bar * T
    ok = bool((err <= lim).all())
    ratio = float((err / lim.clamp_min(1e-300)).max())
    return ok, ratio


def signed(g, n):
    """[n] scales of magnitude 0.5 .. 1.5 and mixed sign."""
    return (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()


# ----------------------------------------------------------------------------- the restatements, on the CPU
def test_restatements_match_torch_conv_in_f64():
    """The f64 restatements against F.conv2d in f64 (and T against the same conv on absolute values) on small, odd shapes -
    a CPU-only check, so the references the GPU tests use are themselves verified without a GPU."""
    from two_stage_object_detection_amd import _ffi
    assert (R.ACT_NONE, R.ACT_PRELU, R.ACT_RELU6, R.ACT_RELU) == (_ffi.ACT_NONE, _ffi.ACT_PRELU, _ffi.ACT_RELU6, _ffi.ACT_RELU)
    g = torch.Generator().manual_seed(1)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    tight = dict(rtol=1e-13, atol=1e-13)
    for (N, H, W, C), stride in [((2, 7, 9, 8), 1), ((2, 7, 9, 8), 2), ((1, 8, 6, 4), 2), ((3, 1, 1, 4), 1), ((1, 2, 2, 4), 2),
                                 ((1, 5, 3, 12), 1)]:
        x = torch.randn(N, H, W, C, generator=g).double()
        w = torch.randn(3, 3, C, generator=g).double()
        scale, shift = signed(g, C).double(), torch.randn(C, generator=g).double()
        wt = w.permute(2, 0, 1).unsqueeze(1)                               # [C,1,3,3]
        for sc, sh in ((scale, shift), (None, None), (None, shift)):
            y, T = R.dwconv_ref(x, w, sc, sh, stride, False)
            ref = nhwc(F.conv2d(nchw(x), wt, None, stride, 1, 1, C))
            refT = nhwc(F.conv2d(nchw(x).abs(), wt.abs(), None, stride, 1, 1, C))
            if sc is not None:
                ref, refT = ref * sc, refT * sc.abs()
            if sh is not None:
                ref, refT = ref + sh, refT + sh.abs()
            torch.testing.assert_close(y, ref, **tight)
            torch.testing.assert_close(T, refT, **tight)
            assert bool((T >= y.abs() * (1 - 1e-12)).all())
            yr, Tr = R.dwconv_ref(x, w, sc, sh, stride, True)
            assert torch.equal(yr, y.clamp_min(0.0)) and torch.equal(Tr, T)
    for pixels, G in [(13, 6), (1, 1), (5, 1)]:
        x = torch.randn(pixels, 2 * G + 2, generator=g).double()            # two channels past 2G that must be ignored
        w, b = torch.randn(G, 2, generator=g).double(), torch.randn(G, generator=g).double()
        x4 = x[:, :2 * G].t().reshape(1, 2 * G, pixels, 1)
        for bias in (b, None):
            y, T = R.gconv_pair_ref(x, w, bias)
            ref = F.conv2d(x4, w.view(G, 2, 1, 1), bias, 1, 0, 1, G).view(G, pixels).t()
            refT = F.conv2d(x4.abs(), w.abs().view(G, 2, 1, 1), None if bias is None else bias.abs(), 1, 0, 1, G).view(G, pixels).t()
            torch.testing.assert_close(y, ref, **tight)
            torch.testing.assert_close(T, refT, **tight)
    for (N, H, W), groups, cpg in [((2, 5, 7), 3, 4), ((1, 6, 4), 2, 8), ((1, 1, 1), 1, 4), ((1, 9, 9), 2, 4)]:
        C = groups * cpg
        x = torch.randn(N, H, W, C, generator=g).double()
        w = torch.randn(C, 3, 3, cpg, generator=g).double()
        scale, shift = signed(g, C).double(), torch.randn(C, generator=g).double()
        y1 = None
        for stride in (1, 2):
            pre = nhwc(F.conv2d(nchw(x), w.permute(0, 3, 1, 2), None, stride, 1, 1, groups)) * scale + shift
            refT = nhwc(F.conv2d(nchw(x).abs(), w.abs().permute(0, 3, 1, 2), None, stride, 1, 1, groups)) * scale.abs() + shift.abs()
            for act, slope, fn in ((R.ACT_NONE, 0.0, lambda v: v), (R.ACT_PRELU, 0.25, lambda v: F.prelu(v, torch.tensor([0.25]).double())),
                                   (R.ACT_RELU6, 0.0, F.relu6), (R.ACT_RELU, 0.0, F.relu)):
                y, T = R.gconv3x3_ref(x, w, groups, scale, shift, stride, act, slope)
                torch.testing.assert_close(y, fn(pre), **tight)
                torch.testing.assert_close(T, refT, **tight)
            y, T = R.gconv3x3_ref(x, w, groups, None, None, stride)
            torch.testing.assert_close(y, (pre - shift) / scale, **tight)
            if stride == 1:
                y1 = R.gconv3x3_ref(x, w, groups, scale, shift, 1, R.ACT_PRELU, 0.25)
            else:        # pad 1, kernel 3: the stride-2 output IS every other stride-1 output (the GPU test shares one reference)
                y2 = R.gconv3x3_ref(x, w, groups, scale, shift, 2, R.ACT_PRELU, 0.25)
                assert torch.equal(y2[0], y1[0][:, ::2, ::2]) and torch.equal(y2[1], y1[1][:, ::2, ::2])


def test_dw_variant_restates_the_kernels_selection():
    """dw_variant against the text of tsod_dwconv3x3_amax_f32: the same thread target and the same ladders in the same order
    (a changed rule must change the restatement, or the GPU cases below silently stop reaching their variants)."""
    with open(os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "pool_layout.hip")) as f:
        src = f.read()
    want = re.search(r"const long want = ([0-9L* ]+);", src).group(1)
    assert math.prod(int(f.strip().rstrip("L")) for f in want.split("*")) == R.DW_WANT
    rungs = re.findall(r"if \(threads_for\((\d), (\d)\) >= want\) TSOD_DW\((\d), (\d), (\d)\);", src)
    last = re.findall(r"else TSOD_DW\((\d), (\d), (\d)\);", src)
    ladder = {1: [], 2: []}
    for r, outs, s, o2, r2 in rungs:
        assert (r, outs) == (r2, o2)
        ladder[int(s)].append((int(r), int(outs)))
    for s, outs, r in last:
        ladder[int(s)].append((int(r), int(outs)))
    assert {s: tuple(v) for s, v in ladder.items()} == R.DW_LADDER
    assert len(R.DW_VARIANTS) == 7
    # the rule at its thresholds: one thread short of the target falls to the next rung
    assert R.dw_threads(1, 9, 1021, 1024, 1, 8, 4) == R.DW_WANT and R.dw_variant(1, 9, 1021, 1024, 1) == (1, 4, 8)
    assert R.dw_variant(1, 9, 1017, 1024, 1) == (1, 4, 4)


# ----------------------------------------------------------------------------- depthwise 3x3
# (N, H, W, C, stride) -> (STRIDE, OUTS, R); every patch shape with OH no multiple of R and OW no multiple of OUTS
DW_CASES = [
    ((1, 9, 1021, 1024, 1), (1, 4, 8)),       # OH = 8 + 1, OW = 4 * 255 + 1
    ((1, 13, 517, 1024, 1), (1, 4, 4)),       # OH = 4 * 3 + 1, OW = 4 * 129 + 1
    ((1, 11, 341, 1024, 1), (1, 4, 2)),       # OH = 2 * 5 + 1, OW = 4 * 85 + 1
    ((2, 21, 30, 24, 1), (1, 2, 2)),
    ((1, 5, 3, 8, 1), (1, 2, 2)),
    ((3, 1, 1, 4, 1), (1, 2, 2)),             # 1 x 1 map: W < OUTS, H < R
    ((1, 10, 1025, 1024, 2), (2, 2, 4)),      # even H, odd W: OH = 5, OW = 513
    ((1, 13, 1037, 512, 2), (2, 2, 2)),       # OH = 7, OW = 519
    ((2, 21, 30, 24, 2), (2, 2, 1)),
    ((1, 2, 2, 4, 2), (2, 2, 1)),
    ((3, 1, 1, 4, 2), (2, 2, 1)),
]
DW_IDS = ["x".join(map(str, c[:4])) + f"s{c[4]}" for c, _ in DW_CASES]


def dw_draw(case, with_affine=True):
    N, H, W, C, stride = case
    g = torch.Generator().manual_seed(5000 + 7 * H + W + C + stride)
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(3, 3, C, generator=g)
    scale, shift = (signed(g, C), torch.randn(C, generator=g)) if with_affine else (None, None)
    return x, w, scale, shift


@functools.lru_cache(maxsize=2)
def dw_case(case):
    """Inputs and the pre-ReLU f64 reference of one case, computed once for its relu = False and relu = True runs."""
    x, w, scale, shift = dw_draw(case)
    y, T = R.dwconv_ref(x, w, scale, shift, case[4], False)
    return x, w, scale, shift, y, T


def dw_slice_buffers(x, OH, OW, dev):
    """The HarDBlock form: input channels [4, 4 + C) of a pitch C + 8 buffer, output channels [8, 8 + C) of a pitch C + 12 one.
    -> (input, output [N,OH,OW,C+12], guard): the guard is one more output row of sentinels right behind the last image, where
    a patch row stored at oh == OH would land."""
    N, H, W, C = x.shape
    xb = torch.full((N, H, W, C + 8), FAR)
    xb[..., 4:4 + C] = x
    rows = torch.full((N * OH + 1, OW, C + 12), SENTINEL, device=dev)
    return xb.to(dev), rows[:N * OH].view(N, OH, OW, C + 12), rows[N * OH:]


def sentinels_intact(out, off, C, guard):
    return bool((out[..., :off] == SENTINEL).all()) and bool((out[..., off + C:] == SENTINEL).all()) and bool((guard == SENTINEL).all())


@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case,variant", DW_CASES, ids=DW_IDS)
def test_dwconv_every_variant_whole_and_slice(ops, dev, case, variant, relu):
    N, H, W, C, stride = case
    assert R.dw_variant(*case) == variant and {v for _, v in DW_CASES} == R.DW_VARIANTS and len(R.DW_VARIANTS) == 7
    x, w, scale, shift, y, T = dw_case(case)
    if relu:
        y = y.clamp_min(0.0)
    OH, OW = y.shape[1:3]
    wg, sg, bg = w.to(dev), scale.to(dev), shift.to(dev)
    whole = ops.dwconv3x3_nhwc(x.to(dev), wg, sg, bg, stride, relu)
    ok, ratio = within(whole, y, T, R.DW_BAR)
    record("dwconv3x3", "S%d_OUTS%d_R%d" % variant, "x".join(map(str, case[:4])) + f" stride {stride} relu {int(relu)}", ratio)
    assert ok, f"whole form: largest err / bar = {ratio}"
    xb, out, guard = dw_slice_buffers(x, OH, OW, dev)
    ret = ops.dwconv3x3_nhwc(xb, wg, sg, bg, stride, relu, C=C, in_off=4, out=out, out_off=8)
    assert ret is out
    assert torch.equal(out[..., 8:8 + C], whole), "the slice form differs from the whole form"
    assert sentinels_intact(out, 8, C, guard), "a store outside [out_off, out_off + C) or past the last row"


def test_dwconv_cases_reach_all_seven_variants():
    assert {R.dw_variant(*case) for case, _ in DW_CASES} == {v for _, v in DW_CASES} == R.DW_VARIANTS
    assert len(R.DW_VARIANTS) == 7


@gpu
@pytest.mark.parametrize("with_affine", [True, False])
@pytest.mark.parametrize("case", [(1, 11, 341, 1024, 1), (1, 13, 1037, 512, 2)], ids=["s1", "s2"])
def test_dwconv_range_word_is_the_slice_abs_max(ops, ffi, dev, case, with_affine):
    """tsod_dwconv3x3_amax_f32 in the slice form, with and without scale / shift: the range word is exactly the abs-max of
    the channels it stored - not of the sentinels around them, nor of the patch rows and columns past OH and OW."""
    N, H, W, C, stride = case
    x, w, scale, shift = dw_draw(case, with_affine)
    y, T = R.dwconv_ref(x, w, scale, shift, stride, True)
    OH, OW = y.shape[1:3]
    xb, out, guard = dw_slice_buffers(x, OH, OW, dev)
    words = ops.new_amax_words(dev, 1)
    wg = w.to(dev)
    sg, bg = (scale.to(dev), shift.to(dev)) if with_affine else (None, None)
    ffi.check(ffi.lib().tsod_dwconv3x3_amax_f32(ffi.ptr(xb), N, H, W, C, C + 8, 4, ffi.ptr(wg), ffi.ptr(sg) or None, ffi.ptr(bg) or None,
                                                stride, 1, ffi.ptr(out), C + 12, 8, words.data_ptr(), ffi.stream_ptr()))
    got = out[..., 8:8 + C]
    ok, ratio = within(got, y, T, R.DW_BAR)
    record("dwconv3x3_amax", "S%d_OUTS%d_R%d" % R.dw_variant(*case), "x".join(map(str, case[:4])) + f" affine {int(with_affine)}", ratio)
    assert ok, f"largest err / bar = {ratio}"
    assert sentinels_intact(out, 8, C, guard)
    assert ops.amax_value(words) == float(got.abs().max()) > 0


@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", [(1, 9, 1021, 1024, 1), (1, 10, 1025, 1024, 2)], ids=["s1", "s2"])
def test_dwconv_value_does_not_depend_on_the_patch_shape(ops, dev, case, relu):
    """'(R, OUTS) only changes which thread computes an output, never its value': channels [16, 24) computed alone select
    the smallest patch and must equal, bit for bit, the same channels of the full run on the tallest patch."""
    N, H, W, C, stride = case
    small = R.DW_LADDER[stride][-1]
    assert R.dw_variant(*case) == (stride, R.DW_LADDER[stride][0][1], R.DW_LADDER[stride][0][0])
    assert R.dw_variant(N, H, W, 8, stride) == (stride, small[1], small[0])
    x, w, scale, shift = dw_draw(case)
    xg = x.to(dev)
    full = ops.dwconv3x3_nhwc(xg, w.to(dev), scale.to(dev), shift.to(dev), stride, relu)
    part = ops.dwconv3x3_nhwc(xg, w[..., 16:24].contiguous().to(dev), scale[16:24].clone().to(dev), shift[16:24].clone().to(dev),
                              stride, relu, C=8, in_off=16)
    assert part.shape == full.shape[:3] + (8,)
    diff = (part - full[..., 16:24]).abs().max().item()
    assert torch.equal(part, full[..., 16:24]), f"patch shapes disagree by up to {diff}"


# ----------------------------------------------------------------------------- grouped-pair 1x1
@gpu
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("pixels,G", [(4100, 512), (4100, 1), (1, 512), (1, 1)])
def test_gconv_pair_stride_loop_and_pitches(ops, ffi, dev, pixels, G, with_bias):
    """4100 x 512 is 2 099 200 threads against a grid capped at 8192 x 256: a second, ragged trip of the stride loop."""
    if (pixels, G) == (4100, 512):
        assert pixels * G > 8192 * 256 and pixels * G % (8192 * 256) != 0
    g = torch.Generator().manual_seed(6000 + G + pixels)
    x = torch.randn(pixels, 2 * G, generator=g)
    w = torch.randn(G, 2, generator=g)
    bias = torch.randn(G, generator=g) if with_bias else None
    y, T = R.gconv_pair_ref(x, w, bias)
    in_pitch, out_pitch = 2 * G + 8, G + 4
    xb = torch.full((pixels, in_pitch), FAR)
    xb[:, :2 * G] = x
    xb, wg = xb.to(dev), w.to(dev)
    bg = bias.to(dev) if with_bias else None
    out = torch.full((pixels, out_pitch), SENTINEL, device=dev)
    words = ops.new_amax_words(dev, 1)
    ffi.check(ffi.lib().tsod_gconv1x1_pair_amax_f32(ffi.ptr(xb), pixels, G, in_pitch, ffi.ptr(wg), ffi.ptr(bg) or None, ffi.ptr(out),
                                                    out_pitch, words.data_ptr(), ffi.stream_ptr()))
    got = out[:, :G]
    ok, ratio = within(got, y, T, R.PAIR_BAR)
    record("gconv1x1_pair", "grid-stride" if pixels * G > 8192 * 256 else "one trip", f"{pixels}x{G} bias {int(with_bias)}", ratio)
    assert ok, f"largest err / bar = {ratio}"
    assert bool((out[:, G:] == SENTINEL).all())
    assert ops.amax_value(words) == float(got.abs().max()) > 0


# ----------------------------------------------------------------------------- grouped 3x3
def gconv_draw(N, H, W, C, groups, seed):
    g = torch.Generator().manual_seed(seed)
    cpg = C // groups
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(C, 3, 3, cpg, generator=g) / (9 * cpg) ** 0.5
    return x, w, signed(g, C), torch.randn(C, generator=g) * 0.1


@functools.lru_cache(maxsize=1)
def gconv_large():
    """The 1 x 129 x 129 x 1024 case (4 260 096 threads against a grid capped at 16384 x 256) and its stride-1 reference; the
    stride-2 reference is every other output of it (checked on the CPU in test_restatements_match_torch_conv_in_f64)."""
    x, w, scale, shift = gconv_draw(1, 129, 129, 1024, 32, 7000)
    y, T = R.gconv3x3_ref(x, w, 32, scale, shift, 1, R.ACT_PRELU, 0.25)
    return x, w, scale, shift, y, T


@gpu
@pytest.mark.parametrize("stride", [1, 2])
def test_gconv3x3_past_the_grid_cap(ops, dev, stride):
    assert 129 * 129 * (1024 // 4) > 16384 * 256
    x, w, scale, shift, y, T = gconv_large()
    if stride == 2:
        y, T = y[:, ::2, ::2], T[:, ::2, ::2]
    got = ops.gconv3x3_nhwc(x.to(dev), w.to(dev), 32, scale.to(dev), shift.to(dev), stride, R.ACT_PRELU, 0.25)
    assert got.shape == y.shape
    ok, ratio = within(got, y, T, R.gconv3x3_bar(32))
    record("gconv3x3", "grid-stride" if stride == 1 else "one trip", f"1x129x129x1024 groups 32 stride {stride} prelu", ratio)
    assert ok, f"largest err / bar = {ratio}"


@gpu
@pytest.mark.parametrize("act,slope", [(R.ACT_NONE, 0.0), (R.ACT_PRELU, 0.2), (R.ACT_RELU6, 0.0), (R.ACT_RELU, 0.0)],
                         ids=["none", "prelu", "relu6", "relu"])
@pytest.mark.parametrize("cpg", [4, 8, 16, 32])
def test_gconv3x3_activations_pitches_and_null_affine(ops, ffi, dev, cpg, act, slope):
    """All four activations at every ResNeXt group width, through pitched buffers (in_pitch = out_pitch = C + 4, the pad
    channels far away on the input side and sentinels on the output side), with and without scale / shift, both strides.
    The inputs are scaled so that RELU6's upper clamp is reached as well as its lower one."""
    groups, N, H, W = 8, 2, 13, 17
    C = groups * cpg
    x, w, scale, shift = gconv_draw(N, H, W, C, groups, 7100 + cpg)
    x, shift = x * 4.0, shift + 1.0
    xb = torch.full((N, H, W, C + 4), FAR)
    xb[..., :C] = x
    xb, wg = xb.to(dev), w.to(dev)
    worst = 0.0
    for stride in (1, 2):
        for sc, sh in ((scale, shift), (None, None)):
            y, T = R.gconv3x3_ref(x, w, groups, sc, sh, stride, act, slope)
            if act == R.ACT_RELU6 and sc is not None:
                assert bool((y == 6.0).any()) and bool((y == 0.0).any())
            out = torch.full(tuple(y.shape[:3]) + (C + 4,), SENTINEL, device=dev)
            sg, bg = (sc.to(dev), sh.to(dev)) if sc is not None else (None, None)
            words = ops.new_amax_words(dev, 1)
            ffi.check(ffi.lib().tsod_gconv3x3_amax_f32(ffi.ptr(xb), N, H, W, C, C + 4, groups, ffi.ptr(wg), ffi.ptr(sg) or None,
                                                       ffi.ptr(bg) or None, stride, act, slope, ffi.ptr(out), C + 4, words.data_ptr(),
                                                       ffi.stream_ptr()))
            got = out[..., :C]
            ok, ratio = within(got, y, T, R.gconv3x3_bar(cpg))
            worst = max(worst, ratio)
            assert ok, f"stride {stride} affine {sc is not None}: largest err / bar = {ratio}"
            assert bool((out[..., C:] == SENTINEL).all())
            assert ops.amax_value(words) == float(got.abs().max())
    record("gconv3x3", f"cpg{cpg}", f"2x13x17x{C} act {act} pitched", worst)


@gpu
def test_gconv3x3_refusals(ops, ffi, dev):
    x = torch.zeros(1, 5, 5, 24, device=dev)
    out = torch.zeros(1, 5, 5, 24, device=dev)
    w = torch.zeros(24 * 9 * 6, device=dev)
    call = lambda groups: ffi.lib().tsod_gconv3x3_f32(ffi.ptr(x), 1, 5, 5, 24, 24, groups, ffi.ptr(w), None, None, 1, R.ACT_NONE, 0.0,
                                                      ffi.ptr(out), 24, ffi.stream_ptr())
    assert call(4) == ERR_UNSUPPORTED          # cpg = 6: no whole float4s per group
    assert call(5) == ERR_INVALID_ARG          # 24 channels do not divide into 5 groups
    assert call(6) == 0                        # cpg = 4


# ----------------------------------------------------------------------------- 3x3 / s2 max pool
def pool(ffi, dev, x, in_pad=0, out_pad=0):
    """tsod_maxpool3x3s2_f32 on x [N,C,H,W] (CPU) through buffers of pitch C + in_pad / C + out_pad -> ([N,C,OH,OW] on the CPU, the
    output buffer): the input's pad channels hold +FAR (a read there would win every max), the output's the sentinel."""
    N, C, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xb = torch.full((N, H, W, C + in_pad), FAR)
    xb[..., :C] = x.permute(0, 2, 3, 1)
    xb = xb.to(dev)
    out = torch.full((N, OH, OW, C + out_pad), SENTINEL, device=dev)
    ffi.check(ffi.lib().tsod_maxpool3x3s2_f32(ffi.ptr(xb), N, H, W, C, C + in_pad, ffi.ptr(out), C + out_pad, ffi.stream_ptr()))
    return out[..., :C].cpu().permute(0, 3, 1, 2), out


def pool_blocks(shape):
    N, C, H, W = shape
    return (N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * (C // 4) + 255) // 256


@gpu
@pytest.mark.parametrize("shape,blocks", [((1, 64, 49, 80), 63),       # the last plain grid, its last block ragged
                                          ((1, 64, 63, 63), 64),       # the first banded grid
                                          ((1, 64, 65, 65), 69),       # banded, rounded up to 72 blocks: three whole idle blocks
                                          ((2, 8, 1, 9), 1), ((2, 8, 9, 1), 1), ((1, 4, 2, 2), 1), ((1, 4, 1, 1), 1)])
@pytest.mark.parametrize("pads", [(0, 0), (4, 8)], ids=["dense", "pitched"])
def test_maxpool_around_the_banded_switch(ffi, dev, shape, blocks, pads):
    assert pool_blocks(shape) == blocks
    x = torch.randn(shape, generator=torch.Generator().manual_seed(8000 + blocks))
    got, out = pool(ffi, dev, x, *pads)
    assert torch.equal(got, F.max_pool2d(x, 3, 2, 1))
    assert bool((out[..., shape[1]:] == SENTINEL).all())


@gpu
@pytest.mark.parametrize("shape", [(1, 64, 49, 80), (1, 64, 65, 65), (1, 4, 2, 2)])
def test_maxpool_negative_and_infinite_inputs(ffi, dev, shape):
    """An all-negative map (a running max that starts at 0 instead of -inf would return zeros) and a map with -inf entries,
    one output window holding nothing else."""
    g = torch.Generator().manual_seed(8100)
    neg = -torch.rand(shape, generator=g) - 0.5
    got, _ = pool(ffi, dev, neg)
    assert torch.equal(got, F.max_pool2d(neg, 3, 2, 1)) and bool((got < 0).all())
    x = torch.randn(shape, generator=g)
    x[torch.rand(shape, generator=g) < 0.3] = float("-inf")
    x[:, :, :2, :2] = float("-inf")                                    # output (0, 0) sees rows and columns 0..1 only
    got, _ = pool(ffi, dev, x, 4, 4)
    ref = F.max_pool2d(x, 3, 2, 1)
    assert bool((ref[:, :, 0, 0] == float("-inf")).all())
    assert torch.equal(got, ref)


# ----------------------------------------------------------------------------- layout changes and absmax
@gpu
def test_nhwc_to_nchw_channel_offset_and_ragged_width(ops, dev):
    x = torch.randn(2, 33, 31, 64, generator=torch.Generator().manual_seed(9000))
    got = ops.nhwc_to_nchw(x.to(dev), C=37, c_off=5)
    assert torch.equal(got.cpu(), x[..., 5:42].permute(0, 3, 1, 2))


@gpu
def test_nchw_to_nhwc_pads_to_c_pad_and_stops_there(ops, ffi, dev):
    """C = 70 into C_pad = 72 of a pitch-80 pixel: channels 70 and 71 are zeroed, channels 72..79 are someone else's."""
    N, C, H, W, c_pad, pitch = 2, 70, 9, 11, 72, 80
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(9001))
    out = torch.full((N, H, W, pitch), SENTINEL, device=dev)
    words = ops.new_amax_words(dev, 1)
    ffi.check(ffi.lib().tsod_nchw_to_nhwc_amax_f32(ffi.ptr(x.to(dev)), N, C, H, W, ffi.ptr(out), pitch, c_pad, words.data_ptr(),
                                                   ffi.stream_ptr()))
    out = out.cpu()
    assert torch.equal(out[..., :C], x.permute(0, 2, 3, 1))
    assert bool((out[..., C:c_pad] == 0).all()) and bool((out[..., c_pad:] == SENTINEL).all())
    assert ops.amax_value(words) == float(x.abs().max())


@gpu
def test_nchw_to_nhwc_single_channel_small_path(ops, ffi, dev):
    """C = 1, C_pad = 4 (the one-thread-per-pixel kernel), whole and into a pitch-8 pixel; 2 x 300 x 7 pixels: several blocks."""
    x = torch.randn(2, 1, 300, 7, generator=torch.Generator().manual_seed(9002))
    got = ops.nchw_to_nhwc(x.to(dev), 4).cpu()
    assert torch.equal(got[..., :1], x.permute(0, 2, 3, 1)) and bool((got[..., 1:] == 0).all())
    out = torch.full((2, 300, 7, 8), SENTINEL, device=dev)
    ffi.check(ffi.lib().tsod_nchw_to_nhwc_f32(ffi.ptr(x.to(dev)), 2, 1, 300, 7, ffi.ptr(out), 8, 4, ffi.stream_ptr()))
    out = out.cpu()
    assert torch.equal(out[..., :4], got) and bool((out[..., 4:] == SENTINEL).all())


@gpu
@pytest.mark.parametrize("extra,lead", [(0, 0), (1, 0), (0, 1)], ids=["float4-second-trip", "scalar-by-length", "scalar-by-pointer"])
def test_absmax_past_the_grid_cap(ops, dev, extra, lead):
    """n = 2048 * 256 * 4 + 4 floats is one float4 more than one trip of the capped grid; n + 1 and a pointer 4 bytes off a
    16-byte boundary take the scalar loop.  The maximum sits in the last element each time."""
    n = 2048 * 256 * 4 + 4 + extra
    base = torch.randn(n + 4, generator=torch.Generator().manual_seed(9100)).to(dev)
    assert base.data_ptr() % 16 == 0
    x = base[lead:lead + n]
    assert x.data_ptr() % 16 == 4 * lead and (n % 4 == 0) == (extra == 0)
    x[-1] = -123.5
    words = ops.new_amax_words(dev, 1)
    ops.absmax(x, words)
    assert ops.amax_value(words) == 123.5
    x[-1] = 0.0
    words = ops.new_amax_words(dev, 1)
    ops.absmax(x, words)
    assert ops.amax_value(words) == float(x.abs().max()) < 123.5
