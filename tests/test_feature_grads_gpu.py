"""The backward of the RoI pooling (csrc/feature_grads.hip: roi_pool_argmax_kernel, roi_pool_gather_kernel,
roi_align_extent_kernel, roi_align_gather_kernel, gather_grid) at every launch and geometry switch, through the C ABI, against
the float64 restatements of tests/feature_grads_restated.py with the per-element bars derived there: strip width and ragged row
ends, strip counts that do not fill the last block, channel groups with dead lanes, bin shapes, spatial_scale, roi_indices,
sampling_ratio x aligned, the culling of align_span, ties / NaN / infinities in the map, the limits of the u16 arg-max record and
of the grid, the refusals, the adjoint identity against the forward kernels, and channel independence.

Every case runs twice (same bits), with accumulate = 0 and with accumulate = 1 onto a random base, with pitches wider than C
(FAR in the input pads, SENTINEL around the output).  Every case with a tolerance prints its largest err / bar; with
TSOD_FEATURE_GRADS_JSONL=<path> the same figures are appended to that file, one JSON line each (TSOD_FEATURE_GRADS_COMMIT names
the commit in them).  The tests without the gpu mark hold the restatements to oracle.roi_pool / oracle.roi_align by the adjoint
identity, an f32 sum in the kernels' order to the bars, and every case to what it is named for."""
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_grads_restated as G  # noqa: E402
import proposal_tail_restated as R  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "feature_grads.hip")
SENTINEL = -7.25          # what d_feat holds around the written channels and behind the last image, before and after
FAR = 1.0e6               # what the pad channels of the map and of d_out hold: one read there wins every maximum
FEAT_PAD, DOUT_PAD, DFEAT_PAD, DFEAT_LEAD = 8, 4, 12, 4
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_ALIGNMENT, ERR_WORKSPACE = 0, -1, -2, -3, -4

# image sides that are no multiple of the map's, chosen so that the .5 RoIs of geometry_rois come back to .5 exactly at
# spatial_scale 1, 0.5 and 2 (test_case_conditions_geometry).  The 16 x 8 map's sides are powers of two: there every dyadic
# coordinate comes back exactly, which the RoIs with samples exactly on an edge need (no sides of the 13 x 11 map give them all).
IMG_OF = {(13, 11): (200, 168), (5, 3): (76, 47), (6, 4): (91, 62), (7, 5): (107, 77), (3, 1): (46, 17), (1, 3): (16, 47),
          (4, 4): (61, 62), (16, 8): (256, 128), (255, 257): (1020, 1028), (50, 84): (800, 1333)}
MAPS = [(13, 11), (5, 3), (6, 4), (7, 5), (3, 1)]
BINS = [(7, 7), (1, 1), (1, 3), (9, 5), (17, 3), (3, 16)]
ALIGN_MODES = [(sr, al) for sr in (0, 1, 2, 3) for al in (False, True)]
CHANNELS = [4, 252, 256, 260, 516]
STRIP_CASES = [(13, 11, 2), (5, 3, 1), (1, 3, 1)]                   # 78, 5 and 1 strips
INDEX_CASES = [(0, 1), (1, 0), (0, 0), (1, 1), (-1, 0), (2, 1), (2, 0, 2)]


def source_text():
    return open(SOURCE).read()


def source_const(name):
    return int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, source_text()).group(1))


# ------------------------------------------------------------------------------------------------- the launch rule, restated
def strips_of(B, Hf, Wf, kStrip=4):
    return B * Hf * ((Wf + kStrip - 1) // kStrip)


def channel_groups(C, kQuadsPerWave=64):
    """(blocks in the grid's y, live lanes of the last group's wave)."""
    quads = C // 4
    groups = (quads + kQuadsPerWave - 1) // kQuadsPerWave
    return groups, quads - (groups - 1) * kQuadsPerWave


# --------------------------------------------------------------------------------------------------------------- the cases
def culling_rois(Hf, Wf, PH, PW, sampling_ratio, aligned):
    """Map-coordinate RoIs for align_span's culling: far outside on every side, between the +-4 clamp and the skip edge,
    three times the map, negative sizes (bins < 0 under aligned), and RoIs of bin size exactly 2 whose samples fall exactly
    on -1, 0, n - 1 and n of each axis (EXACT_ROWS: the last 12 rows)."""
    H, W = float(Hf), float(Wf)
    rows = [[-7, 2, 3, 5], [W - 3, 2, W + 7, 5], [2, -8, 5, 3], [2, H - 3, 5, H + 9], [-6, -7, W + 6, H + 8],
            [-9, -9, -4.5, -4.5], [W + 4.5, H + 4.5, W + 9, H + 9], [-9, -9, -0.5, -0.5], [W - 0.5, H - 0.5, W + 9, H + 9],
            [-W, -H, 2 * W, 2 * H], [6, 2, 1.5, 7], [2, 7, 6, 1.5], [8, 8, 2, 3], [2.75, 3, 3.875, 9]]
    off = 0.5 if aligned else 0.0
    grid = sampling_ratio if sampling_ratio > 0 else 2                   # adaptive: ceil of the bin size 2
    delta = 0.5 if grid == 2 else 1.0                                    # a sample of bin p lies at start + 2 p + delta
    for n, P, axis in ((Hf, PH, 1), (Wf, PW, 0)):
        for target, p in ((-1, 0), (0, 0), (n - 1, 0), (n, 0), (n - 1, P - 1), (n, P - 1)):
            start = target - delta - 2 * p + off
            r = [1.5 + off, 1.5 + off, 1.5 + off + 2 * PW, 1.5 + off + 2 * PH]
            r[axis], r[axis + 2] = start, start + 2 * P
            rows.append(r)
    return torch.tensor(rows, dtype=torch.float32)


EXACT_ROWS = 12


@functools.lru_cache(maxsize=None)
def rois_of(kind, Hf, Wf, B=2, scale=1.0):
    """-> (rois [B,R,4] in image coordinates, fm [B,R,4] the map coordinates they are meant to reach after the scale, img_h,
    img_w).  ``kind``: "geometry" = proposal_tail_restated.geometry_rois (8 random + the 18 named shapes), or ("culling", PH,
    PW, sampling_ratio, aligned).  Every second group is flipped."""
    if kind == "geometry":
        base = R.geometry_rois(torch.Generator().manual_seed(100 * Hf + Wf), Hf, Wf)
    else:
        base = culling_rois(Hf, Wf, *kind[1:])
    fm = torch.stack([base if i % 2 == 0 else base.flip(0) for i in range(B)])
    img_h, img_w = IMG_OF[(Hf, Wf)]
    return R.map_to_image(fm / scale, img_h, img_w, Hf, Wf), fm, img_h, img_w


@functools.lru_cache(maxsize=None)
def feat_of(kind, B, C, Hf, Wf):
    g = torch.Generator().manual_seed(7 * C + Hf + 1000 * B)
    if kind == "marked":
        return R.marked_map(g, B, C, Hf, Wf)
    if kind == "ties":
        feat = torch.randint(0, 3, (B, C, Hf, Wf), generator=g).float()
        feat[:, 0] = 1.0                                                   # channel 0: all tied
        return feat
    assert kind == "no_winner" and C >= 8
    feat = torch.randn(B, C, Hf, Wf, generator=g)
    feat[:, 0] = float("-inf")
    feat[:, 1] = float("nan")
    feat[:, 2] = -G.FLT_MAX
    feat[:, 3] = float("nan")
    feat[:, 3, ::2, ::2] = torch.randn(B, (Hf + 1) // 2, (Wf + 1) // 2, generator=g)    # finite pixels among the NaN
    feat[:, 4][torch.rand(B, Hf, Wf, generator=g) < 0.5] = float("inf")    # several +inf: the first of a bin wins
    feat[:, 5, :3, :3] = float("-inf")                                     # -inf beside finite values
    feat[:, 6, 2:, 1:] = float("nan")
    return feat


def d_out_of(K, C, seed=0):
    return torch.randn(K, C, generator=torch.Generator().manual_seed(31 * K + C + seed))


def base_of(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(9 + shape[1]))


@functools.lru_cache(maxsize=None)
def align_maps_of(kind, Hf, Wf, B, scale, idx, PH, PW, sr, aligned):
    """The RoIAlign walk of one geometry as matrices: shared by every channel count and by both accumulate modes."""
    rois, _, img_h, img_w = rois_of(kind, Hf, Wf, B, scale)
    walk = G.align_walk((B, 1, Hf, Wf), rois, idx, img_h, img_w, PH, PW, sr, aligned, scale)
    return G.align_maps(walk, (B, 1, Hf, Wf), rois.shape[0] * rois.shape[1])


@functools.lru_cache(maxsize=None)
def reference(op, kind, fkind, Hf, Wf, B, C, scale, idx, PH, PW, sr=2, aligned=False):
    """-> (feat, rois, img_h, img_w, d_out, (want, T, N)) of one case, computed once."""
    rois, _, img_h, img_w = rois_of(kind, Hf, Wf, B, scale)
    feat = feat_of(fkind, B, C, Hf, Wf)
    d_out = d_out_of(rois.shape[0] * rois.shape[1], C)
    if op == "pool":
        ref = G.pool_grad_ref(feat, rois, idx, img_h, img_w, d_out, PH, PW, scale)
    else:
        ref = G.align_grad_ref(tuple(feat.shape), rois, idx, img_h, img_w, d_out, PH, PW, sr, aligned, scale,
                               maps=align_maps_of(kind, Hf, Wf, B, scale, idx, PH, PW, sr, aligned))
    return feat, rois, img_h, img_w, d_out, ref


def bar_of(op, T, N):
    return G.pool_bar(T, N) if op == "pool" else G.align_bar(T, N)


def ratio_of(got, want, bar):
    """The largest |got - want| / bar over the elements with a bar (where the bar is 0 the caller asserts equality)."""
    err = (got.double() - want).abs()
    has = bar > 0
    return float((err[has] / bar[has]).max()) if bool(has.any()) else 0.0


def record(kernel, variant, shape, ratio):
    """Print one kernel's largest err / bar at one case, and append it to the JSON lines file when one is asked for."""
    line = {"kernel": kernel, "variant": variant, "shape": shape, "max_err_over_bar": round(float(ratio), 4),
            "commit": os.environ.get("TSOD_FEATURE_GRADS_COMMIT", "unknown")}
    print("feature_grads:", json.dumps(line))
    path = os.environ.get("TSOD_FEATURE_GRADS_JSONL")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ============================================================================= the restatements, on the CPU
ADJOINT_BINS = [(7, 7), (9, 5), (1, 1), (3, 16)]


def adjoint_case(scale, C=4):
    Hf, Wf, idx = 13, 11, (1, 0)
    rois, _, img_h, img_w = rois_of("geometry", Hf, Wf, 2, scale)
    feat = torch.randn(2, C, Hf, Wf, generator=torch.Generator().manual_seed(17))
    rois5 = R.rois5_of(R.roi_to_map(rois, img_h, img_w, Hf, Wf), torch.tensor(idx), rois.shape[1])
    return feat, rois, rois5, idx, img_h, img_w, d_out_of(rois5.shape[0], C)


@pytest.mark.parametrize("PH,PW", ADJOINT_BINS)
def test_pool_restatement_is_the_adjoint_of_the_oracle(PH, PW):
    """RoIPool + mean is linear in the map once the arg-max is fixed (empty bins give 0 on both sides), so
    <oracle.roi_pool(x).mean, d> = <x, pool_avg_grad_f64(d)>: both sides are float64 sums of the same f32 maxima times d.  The
    plain scatter (pool_grad_ref) must be the autograd restatement."""
    worst = 0.0
    for scale in (1.0, 0.5):
        feat, rois, rois5, idx, img_h, img_w, d = adjoint_case(scale)
        m = oracle.roi_pool(feat, rois5, (PH, PW), scale).double().mean(dim=(2, 3))
        grad = G.pool_avg_grad_f64(feat, rois, idx, img_h, img_w, d, PH, PW, scale)
        lhs, rhs = float((m * d.double()).sum()), float((feat.double() * grad).sum())
        size = float((m.abs() * d.double().abs()).sum())
        assert size > 1.0
        worst = max(worst, abs(lhs - rhs) / size)
        assert abs(lhs - rhs) <= 1e-12 * size, (scale, lhs, rhs)
        want, T, N = G.pool_grad_ref(feat, rois, idx, img_h, img_w, d, PH, PW, scale)
        assert float((want - grad).abs().max()) <= 1e-14 * float(T.max())
        assert bool((T >= want.abs() - 1e-15).all()) and bool(((N == 0) == (T == 0)).all())
    print("feature_grads: pool adjoint, largest |lhs - rhs| / sum|m||d| =", worst)


@pytest.mark.parametrize("PH,PW", ADJOINT_BINS)
def test_align_restatement_is_the_adjoint_of_the_oracle(PH, PW):
    """RoIAlign + mean is linear in the map: <oracle.roi_align(x).mean, d> = <x, align_avg_grad_f64(d)> to the oracle's own f32
    rounding: it sums 4 count products per bin in f32, so (4 count_max + 4) u of sum |a| |d| with a the oracle on |x|."""
    worst = 0.0
    for scale in (1.0, 0.5):
        feat, rois, rois5, idx, img_h, img_w, d = adjoint_case(scale)
        for sr, aligned in ALIGN_MODES:
            a = oracle.roi_align(feat, rois5, (PH, PW), scale, sr, aligned).double().mean(dim=(2, 3))
            a_abs = oracle.roi_align(feat.abs(), rois5, (PH, PW), scale, sr, aligned).double().mean(dim=(2, 3))
            grad = G.align_avg_grad_f64(tuple(feat.shape), rois, idx, img_h, img_w, d, PH, PW, sr, aligned, scale)
            count_max = max(G.align_geom(tuple(fm), PH, PW, sr, aligned, scale)[6] for fm in rois5[:, 1:].tolist())
            lhs, rhs = float((a * d.double()).sum()), float((feat.double() * grad).sum())
            size = float((a_abs * d.double().abs()).sum())
            assert size > 1.0
            bound = (4 * count_max + 4) * G.U * size
            worst = max(worst, abs(lhs - rhs) / bound)
            assert abs(lhs - rhs) <= bound, (scale, sr, aligned, lhs, rhs, bound)
    print("feature_grads: align adjoint, largest |lhs - rhs| / bound =", worst)


@pytest.mark.parametrize("PH,PW", ADJOINT_BINS)
def test_bars_bound_an_f32_sum_in_the_kernels_order(PH, PW):
    """kernel_order_f32 - the same terms, f32 operations, the kernel's order - stays within the derived bars on the adjoint
    cases, with and without a base, and is exactly 0 (exactly the base) where nothing arrives."""
    worst = {"pool": 0.0, "align": 0.0}
    for scale in (1.0, 0.5):
        feat, rois, rois5, idx, img_h, img_w, d = adjoint_case(scale)
        shape = tuple(feat.shape)
        base = base_of(shape)
        am = G.pool_argmax(feat, rois, idx, img_h, img_w, PH, PW, scale)
        runs = [("pool", G.pool_grad_ref(feat, rois, idx, img_h, img_w, d, PH, PW, scale, argmax=am), dict(argmax=am))]
        for sr, aligned in ALIGN_MODES:
            walk = G.align_walk(shape, rois, idx, img_h, img_w, PH, PW, sr, aligned, scale)
            maps = G.align_maps(walk, shape, rois5.shape[0])
            runs.append(("align", G.align_grad_ref(shape, rois, idx, img_h, img_w, d, PH, PW, sr, aligned, scale, maps=maps),
                         dict(walk=walk)))
        for op, (want, T, N), how in runs:
            for b in (None, base):
                got = G.kernel_order_f32(op, shape, d, PH, PW, base=b, **how)
                w, t, n = (want, T, N) if b is None else G.with_base(want, T, N, b)
                bar = bar_of(op, t, n)
                assert bool(((got.double() - w).abs() <= bar).all()), (op, scale, ratio_of(got, w, bar))
                assert torch.equal(bits(got[N == 0]), bits((torch.zeros(shape) if b is None else b)[N == 0]))
                worst[op] = max(worst[op], ratio_of(got, w, bar))
    print("feature_grads: f32 in the kernel's order, largest err / bar =", worst)
    assert 0.0 < worst["pool"] <= 1.0 and 0.0 < worst["align"] <= 1.0


def plain_first_max(feat, b, c, hs, he, ws, we, Wf):
    """The kernel's loop in plain Python: from -FLT_MAX, strict '>', h outer, w inner -> map index or -1."""
    m, at = -G.FLT_MAX, -1
    for h in range(hs, he):
        for w in range(ws, we):
            v = float(feat[b, c, h, w])
            if v > m:
                m, at = v, h * Wf + w
    return at


def plain_last_max(feat, b, c, hs, he, ws, we, Wf):
    m, at = -G.FLT_MAX, -1
    for h in range(hs, he):
        for w in range(ws, we):
            v = float(feat[b, c, h, w])
            if v >= m and v > -G.FLT_MAX:
                m, at = v, h * Wf + w
    return at


def bins_of_case(rois, idx, img_h, img_w, Hf, Wf, PH, PW, scale=1.0):
    """[(k, b, bin index, hs, he, ws, we)] of every non-empty bin of every RoI of a valid group."""
    out = []
    Rn = rois.shape[1]
    for k, r in enumerate(rois.reshape(-1, 4).tolist()):
        b = idx[k // Rn]
        if 0 <= b < rois.shape[0]:
            for ph, pw, hs, he, ws, we in G.pool_bins(G.roi_to_map(r, img_h, img_w, Hf, Wf), Hf, Wf, PH, PW, scale):
                if he > hs and we > ws:
                    out.append((k, b, ph * PW + pw, hs, he, ws, we))
    return out


def test_case_conditions_pool_maps():
    """The tie map has bins whose first and last maximum differ (and channel 0 sends every bin to its first pixel); the
    no-winner map has non-empty bins without a winner in the -inf, NaN and -FLT_MAX channels, a finite winner in every
    non-empty bin of the NaN-but-finite channel that holds a finite pixel, and a first +inf; pool_argmax follows the plain
    loop on all of it."""
    Hf, Wf, B, PH, PW, idx = 13, 11, 2, 7, 7, (0, 1)
    rois, _, img_h, img_w = rois_of("geometry", Hf, Wf, B, 1.0)
    bins = bins_of_case(rois, idx, img_h, img_w, Hf, Wf, PH, PW)
    assert len(bins) > 500
    for fkind in ("ties", "no_winner"):
        feat = feat_of(fkind, B, 8, Hf, Wf)
        am = {k: rec for k, _, rec in G.pool_argmax(feat, rois, idx, img_h, img_w, PH, PW)}
        differ = none = finite_wins = inf_wins = 0
        for k, b, bin_, hs, he, ws, we in bins:
            for c in range(8):
                first = plain_first_max(feat, b, c, hs, he, ws, we, Wf)
                assert int(am[k][bin_, c]) == first, (fkind, k, bin_, c)
                if fkind == "ties":
                    differ += first != plain_last_max(feat, b, c, hs, he, ws, we, Wf)
                    if c == 0:
                        assert first == hs * Wf + ws
                else:
                    if c in (0, 1, 2):
                        assert first == -1
                        none += 1
                    window = feat[b, c, hs:he, ws:we]
                    if c == 3 and bool(torch.isfinite(window).any()) and bool(torch.isnan(window).any()):
                        assert first >= 0 and bool(torch.isfinite(feat[b, c].reshape(-1)[first]))
                        finite_wins += 1
                    if c == 4 and bool(torch.isinf(window).sum() >= 2):
                        h, w = torch.nonzero(torch.isinf(window))[0].tolist()
                        assert first == (hs + h) * Wf + ws + w
                        inf_wins += 1
        if fkind == "ties":
            assert differ > 100
        else:
            assert none > 1000 and finite_wins > 100 and inf_wins > 20


def test_case_conditions_geometry():
    """The .5 RoIs reach .5 exactly at every scale on every map; some RoI's RoIPool extent starts and ends inside a strip."""
    kStrip = source_const("kStrip")
    for (Hf, Wf, B) in [(h, w, 2) for h, w in MAPS] + [(1, 3, 1)]:
        for scale in (1.0, 0.5, 2.0):
            rois, fm, img_h, img_w = rois_of("geometry", Hf, Wf, B, scale)
            assert rois.shape[1] == 26 == 8 + R.GEOMETRY_NAMED
            back = R.roi_to_map(rois, img_h, img_w, Hf, Wf) * scale
            assert torch.equal(back[0, list(R.HALF_ROWS)], fm[0, list(R.HALF_ROWS)]), (Hf, Wf, scale)
            assert float((back - fm).abs().max()) < 1e-3
            assert (img_h % Hf or Hf == 1) and (img_w % Wf or Wf == 1)
    rois, _, img_h, img_w = rois_of("geometry", 13, 11, 2, 1.0)
    ext = [G.pool_extent(G.roi_to_map(r, img_h, img_w, 13, 11), 13, 11) for r in rois[0].tolist()]
    assert any(e[2] % kStrip and e[3] % kStrip and e[3] > e[2] for e in ext)
    assert any(e[1] <= e[0] or e[3] <= e[2] for e in ext)               # ... and some RoI covers nothing


CULLING_MAPS = [(13, 11), (16, 8)]


@pytest.mark.parametrize("Hf,Wf", CULLING_MAPS)
@pytest.mark.parametrize("PH,PW", [(7, 7), (1, 1), (17, 3), (3, 16)])
def test_case_conditions_culling(PH, PW, Hf, Wf):
    """The culling RoIs reach what they are named for, by the reference alone: a RoI cut by align_span's +-4 clamp, an extent
    that starts and ends inside a strip, a negative bin size under aligned = 1, an adaptive grid >= 5, and on the 16 x 8 map
    samples exactly on -1, 0, n - 1 and n of both axes (which the skip rule keeps)."""
    kStrip = source_const("kStrip")
    for sr, aligned in ALIGN_MODES:
        rois, fm, img_h, img_w = rois_of(("culling", PH, PW, sr, aligned), Hf, Wf, 2, 1.0)
        back = R.roi_to_map(rois, img_h, img_w, Hf, Wf)
        assert float((back - fm).abs().max()) < 1e-4
        clamped = inside = negative = big_grid = 0
        for r in rois[0].tolist():
            m = G.roi_to_map(r, img_h, img_w, Hf, Wf)
            sh_, sw_, bh, bw, gh, gw, count = G.align_geom(m, PH, PW, sr, aligned)
            y0, y1, cy = G.align_span(sh_, bh, PH, Hf)
            x0, x1, cx = G.align_span(sw_, bw, PW, Wf)
            clamped += cy or cx
            inside += bool(x0 % kStrip and x1 % kStrip and x1 > x0)
            negative += bool(bh < 0 or bw < 0)
            big_grid += bool(gh >= 5 or gw >= 5)
        assert clamped >= 4 and inside >= 1
        assert (negative >= 3) == aligned and (negative == 0) != aligned
        if sr == 0:
            assert big_grid >= 1                                                     # no RoI larger than four times the map
            assert float((fm[..., 2:] - fm[..., :2]).abs().max()) <= 4 * max(Hf, Wf)
        if (Hf, Wf) != (16, 8):
            continue
        assert torch.equal(back, fm), (sr, aligned)
        hit = {"y": set(), "x": set()}
        for r in rois[0, -EXACT_ROWS:].tolist():
            m = G.roi_to_map(r, img_h, img_w, Hf, Wf)
            sh_, sw_, bh, bw, gh, gw, count = G.align_geom(m, PH, PW, sr, aligned)
            assert float(bh) == 2.0 and float(bw) == 2.0
            cy, sky = G.align_axis(sh_, bh, gh, PH, Hf)[:2]
            cx, skx = G.align_axis(sw_, bw, gw, PW, Wf)[:2]
            for name, c, skip, n in (("y", cy, sky, Hf), ("x", cx, skx, Wf)):
                for v in (-1, 0, n - 1, n):
                    if bool(((c == v) & ~skip).any()):
                        hit[name].add(v)
        assert hit["y"] == {-1, 0, Hf - 1, Hf} and hit["x"] == {-1, 0, Wf - 1, Wf}, (sr, aligned, hit)


def test_extent_and_bin_culling_hold_every_sample():
    """align_span, restated: on every RoI of the sweep the extent of the RoI and the span of each bin row / column contain
    every pixel that a non-skipped sample of it touches - the property the kernel's three skips rely on."""
    for PH, PW in ((7, 7), (1, 1), (3, 16)):
        for sr, aligned in ALIGN_MODES:
            for kind, Hf, Wf in (("geometry", 13, 11), (("culling", PH, PW, sr, aligned), 13, 11),
                                 (("culling", PH, PW, sr, aligned), 16, 8)):
                rois, _, img_h, img_w = rois_of(kind, Hf, Wf, 2, 1.0)
                for r in rois[0].tolist():
                    m = G.roi_to_map(r, img_h, img_w, Hf, Wf)
                    sh_, sw_, bh, bw, gh, gw, count = G.align_geom(m, PH, PW, sr, aligned)
                    for start, bin_, grid, P, n in ((sh_, bh, gh, PH, Hf), (sw_, bw, gw, PW, Wf)):
                        c, skip, low, high, l = G.align_axis(start, bin_, grid, P, n)
                        lo, hi, _ = G.align_span(start, bin_, P, n)
                        assert bool(((low >= lo) & (high < hi))[~skip].all()), (kind, r)
                        for p in range(P):
                            lo, hi, _ = G.align_span(np.float32(start) + np.float32(p) * np.float32(bin_), bin_, 1, n)
                            assert bool(((low[p] >= lo) & (high[p] < hi))[~skip[p]].all()), (kind, r, p)


def test_launch_rule_restated_and_pinned_to_the_source():
    """kQuadsPerWave, kStrip and kWaves from the kernel text; the shapes of the sweep land where they are said to land."""
    text = source_text()
    kQ, kS, kW = source_const("kQuadsPerWave"), source_const("kStrip"), source_const("kWaves")
    assert (kQ, kS, kW) == (64, 4, 4)
    assert "tsod_cdiv(strips, kWaves)" in text and "tsod_cdiv(C / 4, kQuadsPerWave)" in text
    assert "(long)B * Hf * ((Wf + kStrip - 1) / kStrip)" in text
    assert "bin += kWaves" in text and "threadIdx.x >> 6" in text
    assert text.count("px0 + kStrip <= e.z || px0 >= e.w") == 2          # both gather kernels cull on the extent
    assert "(long)B * R <= 65535" in text and "(long)Hf * Wf <= 65535" in text and "kNoArgmax = 0xFFFFu" in text
    # strips: 78 and 5 leave the last block's waves 2 and 1.. idle, 1 is a single strip; every ragged row end
    assert [strips_of(B, Hf, Wf, kS) for Hf, Wf, B in STRIP_CASES] == [78, 5, 1]
    assert [strips_of(B, Hf, Wf, kS) % kW for Hf, Wf, B in STRIP_CASES] == [2, 1, 1]
    assert sorted(Wf % kS for Hf, Wf in MAPS) == [0, 1, 1, 3, 3] and min(Wf for Hf, Wf in MAPS) < kS
    # channel groups: one live lane, 63 live lanes, a full wave, a second group of one live lane, a third
    assert [channel_groups(C, kQ) for C in CHANNELS] == [(1, 1), (1, 63), (1, 64), (2, 1), (3, 1)]
    # bins: fewer bins than waves, ragged last trips, an even one
    assert [PH * PW for PH, PW in BINS] == [49, 1, 3, 45, 51, 48]
    assert [PH * PW % kW for PH, PW in BINS] == [1, 1, 3, 1, 3, 0]


# ============================================================================= through the C ABI
@pytest.fixture(scope="module")
def ffi():
    from two_stage_object_detection_amd import _ffi
    return _ffi


def nhwc_padded(t_nchw, lead, pad, fill):
    """[B,C,H,W] -> [B*H*W (+ guard), lead + C + pad] rows with ``fill`` around the channels."""
    B, C, H, W = t_nchw.shape
    buf = torch.full((B * H * W, lead + C + pad), fill)
    buf[:, lead:lead + C] = t_nchw.permute(0, 2, 3, 1).reshape(-1, C)
    return buf


def launch(ffi, dev, op, feat, rois, idx, img_h, img_w, d_out, PH, PW, sr=2, aligned=False, scale=1.0, base=None,
           channels=None, expect=OK, bad=None):
    """One call of tsod_roi_pool_avg_grad_f32 / tsod_roi_align_avg_grad_f32 with feat_pitch = C + 8 (FAR in the pads),
    d_out_pitch = C + 4 (FAR), d_feat_pitch = C + 12 with the written channels 4 floats in (SENTINEL before, behind, and in a
    guard row after the last image).  ``channels`` = (first, count): the same buffers, the pointers moved to that channel and
    C = count.  ``bad`` overrides one argument for the refusals.  Returns d_feat [B,count,Hf,Wf] on the CPU after checking
    that every float outside the written window is what it was."""
    B, C, Hf, Wf = feat.shape
    K = rois.shape[0] * rois.shape[1]
    c0, cn = channels or (0, C)
    fbuf = nhwc_padded(feat, 0, FEAT_PAD, FAR).to(dev)
    dbuf = torch.full((K, C + DOUT_PAD), FAR)
    dbuf[:, :C] = d_out
    dbuf = dbuf.to(dev)
    rows = B * Hf * Wf
    init = torch.full((rows + 1, C + DFEAT_PAD), SENTINEL)
    if base is not None:
        init[:rows, DFEAT_LEAD:DFEAT_LEAD + C] = base.permute(0, 2, 3, 1).reshape(-1, C)
    out = init.to(dev)
    r, i = rois.to(dev).contiguous(), torch.tensor(idx, dtype=torch.int32, device=dev)
    L = ffi.lib()
    if op == "pool":
        ws_bytes = L.tsod_roi_pool_avg_grad_workspace_bytes(B, rois.shape[1], cn, PH, PW)
    else:
        ws_bytes = L.tsod_roi_align_avg_grad_workspace_bytes(B, rois.shape[1])
    ws = torch.zeros(ws_bytes + 64, dtype=torch.uint8, device=dev)
    a = dict(feat_ptr=ffi.ptr(fbuf) + 4 * c0, C=cn, feat_pitch=C + FEAT_PAD, rois_ptr=ffi.ptr(r), img_h=float(img_h),
             img_w=float(img_w), sr=int(sr), d_out_ptr=ffi.ptr(dbuf) + 4 * c0, d_out_pitch=C + DOUT_PAD,
             d_feat_ptr=ffi.ptr(out) + 4 * (DFEAT_LEAD + c0),
             d_feat_pitch=C + DFEAT_PAD, ws=ffi.ptr(ws), ws_bytes=ws_bytes)
    assert set(bad or {}) <= set(a), bad
    a.update(bad or {})
    acc = 0 if base is None else 1
    if op == "pool":
        rc = L.tsod_roi_pool_avg_grad_f32(a["feat_ptr"], B, Hf, Wf, a["C"], a["feat_pitch"], a["rois_ptr"], ffi.ptr(i),
                                          rois.shape[1], a["img_h"], a["img_w"], float(scale), PH, PW, a["d_out_ptr"],
                                          a["d_out_pitch"], a["d_feat_ptr"], a["d_feat_pitch"], acc, a["ws"], a["ws_bytes"],
                                          ffi.stream_ptr())
    else:
        rc = L.tsod_roi_align_avg_grad_f32(B, Hf, Wf, a["C"], a["rois_ptr"], ffi.ptr(i), rois.shape[1], a["img_h"], a["img_w"],
                                           float(scale), PH, PW, a["sr"], int(aligned), a["d_out_ptr"], a["d_out_pitch"],
                                           a["d_feat_ptr"], a["d_feat_pitch"], acc, a["ws"], a["ws_bytes"], ffi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (op, rc, expect, bad)
    got = out.cpu()
    if rc != OK:
        assert torch.equal(bits(got), bits(init)), "a refused call wrote to d_feat"
        return None
    lo, hi = DFEAT_LEAD + c0, DFEAT_LEAD + c0 + cn
    keep = torch.ones_like(init, dtype=torch.bool)
    keep[:rows, lo:hi] = False
    assert torch.equal(bits(got[keep]), bits(init[keep])), "d_feat was written outside its channels / behind its last image"
    return got[:rows, lo:hi].reshape(B, Hf, Wf, cn).permute(0, 3, 1, 2).contiguous()


def check_against(ffi, dev, op, feat, rois, idx, img_h, img_w, d_out, ref, PH, PW, sr=2, aligned=False, scale=1.0, what=""):
    """Both accumulate modes, each twice: the same bits, within the bar of every element, exact where nothing arrives.
    -> the largest err / bar."""
    want, T, N = ref
    shape = tuple(feat.shape)
    worst = 0.0
    for base in (None, base_of(shape)):
        got = launch(ffi, dev, op, feat, rois, idx, img_h, img_w, d_out, PH, PW, sr, aligned, scale, base)
        again = launch(ffi, dev, op, feat, rois, idx, img_h, img_w, d_out, PH, PW, sr, aligned, scale, base)
        mode = (what, op, "accumulate" if base is not None else "write")
        assert torch.equal(bits(got), bits(again)), (mode, "two runs differ")
        assert not bool(torch.isnan(got).any()), mode
        w, t, n = (want, T, N) if base is None else G.with_base(want, T, N, base)
        untouched = torch.zeros(shape) if base is None else base
        assert torch.equal(bits(got[N == 0]), bits(untouched[N == 0])), (mode, "an element that no RoI reaches changed")
        bar = bar_of(op, t, n)
        ratio = ratio_of(got, w, bar)
        print("feature_grads: err / bar", mode, ratio)
        bad = (got.double() - w).abs() > bar
        assert not bool(bad.any()), (mode, ratio, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
        worst = max(worst, ratio)
    return worst


def sweep(ffi, dev, op, kind, fkind, Hf, Wf, B, C, scale, idx, PH, PW, modes=((2, False),)):
    worst = 0.0
    for sr, aligned in (modes if op == "align" else ((2, False),)):
        feat, rois, img_h, img_w, d_out, ref = reference(op, kind, fkind, Hf, Wf, B, C, scale, idx, PH, PW, sr, aligned)
        worst = max(worst, check_against(ffi, dev, op, feat, rois, idx, img_h, img_w, d_out, ref, PH, PW, sr, aligned, scale,
                                         what=(Hf, Wf, B, C, PH, PW, sr, aligned, scale, idx)))
    return worst


KERNEL = {"pool": "roi_pool_avg_grad", "align": "roi_align_avg_grad"}


@gpu
@pytest.mark.parametrize("op", ["pool", "align"])
@pytest.mark.parametrize("Hf,Wf,B", [(h, w, 2) for h, w in MAPS] + STRIP_CASES[1:])
def test_maps_strips_and_ragged_row_ends(ffi, dev, op, Hf, Wf, B):
    """Wf of 11, 3, 4, 5 and 1 (rows that end inside a strip, rows narrower than one), strip counts of 78, 5 and 1."""
    idx = (1, 0)[:B] if B == 2 else (0,)
    r = sweep(ffi, dev, op, "geometry", "marked", Hf, Wf, B, 8, 1.0, idx, 7, 7, modes=((2, False), (0, True)))
    record(KERNEL[op], "map", [Hf, Wf, B], r)


@gpu
@pytest.mark.parametrize("op", ["pool", "align"])
@pytest.mark.parametrize("C", CHANNELS)
def test_channel_groups(ffi, dev, op, C):
    """1, 63 and 64 live lanes in one group; a second and a third group whose wave has one live lane."""
    r = sweep(ffi, dev, op, "geometry", "marked", 13, 11, 2, C, 1.0, (1, 0), 7, 7, modes=((2, False), (3, True)))
    record(KERNEL[op], "channels", [C], r)


@gpu
@pytest.mark.parametrize("PH,PW", BINS)
def test_pool_bins(ffi, dev, PH, PW):
    """Fewer bins than waves, ragged last trips of the bin loop, bins wider than the map; on the marked map a wrong column
    moves the result by a whole d / (PH PW)."""
    record(KERNEL["pool"], "bins", [PH, PW], sweep(ffi, dev, "pool", "geometry", "marked", 13, 11, 2, 8, 1.0, (1, 0), PH, PW))


@gpu
@pytest.mark.parametrize("PH,PW", BINS)
def test_align_bins_sampling_ratio_aligned(ffi, dev, PH, PW):
    """sampling_ratio 0 (adaptive), 1, 2, 3 x aligned 0, 1 on every bin shape."""
    r = sweep(ffi, dev, "align", "geometry", "marked", 13, 11, 2, 8, 1.0, (1, 0), PH, PW, modes=ALIGN_MODES)
    record(KERNEL["align"], "bins x sampling_ratio x aligned", [PH, PW], r)


@gpu
@pytest.mark.parametrize("op", ["pool", "align"])
@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0])
def test_spatial_scale(ffi, dev, op, scale):
    r = sweep(ffi, dev, op, "geometry", "marked", 13, 11, 2, 8, scale, (1, 0), 7, 7, modes=((2, False), (0, True), (3, True)))
    record(KERNEL[op], "spatial_scale", [scale], r)


@gpu
@pytest.mark.parametrize("op", ["pool", "align"])
@pytest.mark.parametrize("idx", INDEX_CASES)
def test_roi_indices(ffi, dev, op, idx):
    """Two groups on one image (the other gets zeros, or keeps its base), a group that names no image of the batch (it adds
    nothing), three groups of which two share an image."""
    B = len(idx)
    feat, rois, img_h, img_w, d_out, ref = reference(op, "geometry", "marked", 13, 11, B, 8, 1.0, idx, 7, 7)
    N = ref[2]
    for b in range(B):
        assert bool((N[b] > 0).any()) == (b in idx)
    r = check_against(ffi, dev, op, feat, rois, idx, img_h, img_w, d_out, ref, 7, 7, what=idx)
    record(KERNEL[op], "roi_indices", list(idx), r)


@gpu
@pytest.mark.parametrize("Hf,Wf,C", [(13, 11, 8), (16, 8, 8), (13, 11, 260)])
@pytest.mark.parametrize("PH,PW", [(7, 7), (1, 1), (17, 3), (3, 16)])
def test_align_culling(ffi, dev, PH, PW, Hf, Wf, C):
    """align_span's extent, bin-row and bin-column skips on the RoIs of test_case_conditions_culling, every sampling_ratio x
    aligned; on the 16 x 8 map samples lie exactly on the skip edges; C = 260 walks the same RoIs in a wave with one live
    lane."""
    modes = ALIGN_MODES if C == 8 else ((2, False), (0, True))
    worst = 0.0
    for sr, aligned in modes:
        worst = max(worst, sweep(ffi, dev, "align", ("culling", PH, PW, sr, aligned), "marked", Hf, Wf, 2, C, 1.0, (1, 0), PH, PW,
                                 modes=((sr, aligned),)))
    record(KERNEL["align"], "culling", [PH, PW, Hf, Wf, C], worst)


@gpu
@pytest.mark.parametrize("fkind", ["ties", "no_winner", "marked"])
@pytest.mark.parametrize("PH,PW", [(7, 7), (3, 16)])
def test_pool_ties_and_values_without_a_winner(ffi, dev, fkind, PH, PW):
    """Ties (the first maximum wins), channels of -inf, NaN and -FLT_MAX (no winner: nothing arrives, exactly), NaN around
    finite pixels (the finite one wins), several +inf (the first wins)."""
    record(KERNEL["pool"], fkind, [PH, PW], sweep(ffi, dev, "pool", "geometry", fkind, 13, 11, 2, 8, 1.0, (0, 1), PH, PW))


@functools.lru_cache(maxsize=None)
def u16_case():
    Hf, Wf, C, PH, PW = 255, 257, 4, 2, 3
    img_h, img_w = IMG_OF[(Hf, Wf)]
    feat = torch.randn(1, C, Hf, Wf, generator=torch.Generator().manual_seed(41))
    feat[0, :, Hf - 1, Wf - 1] = 100.0                                     # the map's maximum at pixel index 65534
    fm = torch.tensor([[[0, 0, Wf - 1, Hf - 1], [Wf - 1, Hf - 1, Wf - 1, Hf - 1], [0, Hf - 1, Wf - 1, Hf - 1],
                        [Wf - 9, Hf - 7, Wf + 5, Hf + 5], [100.5, 90.5, 180.5, 200.5], [-3, 250, 20, 254]]], dtype=torch.float32)
    rois = R.map_to_image(fm, img_h, img_w, Hf, Wf)
    d_out = d_out_of(6, C)
    am = G.pool_argmax(feat, rois, (0,), img_h, img_w, PH, PW)
    return feat, rois, img_h, img_w, d_out, am, G.pool_grad_ref(feat, rois, (0,), img_h, img_w, d_out, PH, PW, argmax=am)


def test_case_conditions_u16_record():
    """Hf Wf = 65535, and the record of the whole-map, last-pixel and last-row RoIs holds 0xFFFE = 65534 beside none."""
    feat, rois, img_h, img_w, d_out, am, (want, T, N) = u16_case()
    assert feat.shape[2] * feat.shape[3] == 65535
    for k in (0, 1, 2):
        assert int(am[k][2].max()) == 65534 == 0xFFFE
    assert bool((am[1][2] == 65534).all()) and int(N[0, 0, -1, -1]) >= 6 + 2
    assert bool((am[3][2] == -1).any())


@gpu
def test_pool_u16_record_at_its_limit(ffi, dev):
    feat, rois, img_h, img_w, d_out, am, ref = u16_case()
    r = check_against(ffi, dev, "pool", feat, rois, (0,), img_h, img_w, d_out, ref, 2, 3, what="Hf Wf = 65535")
    record(KERNEL["pool"], "u16 record limit", [255, 257], r)


@functools.lru_cache(maxsize=None)
def grid_limit_case():
    """B R = 65535 (the limit of the grid's y) on a 4 x 4 map with one bin: five RoIs in a cycle, so the reference is the five
    RoIs' gradients times the float64 sums of their d_out rows."""
    Hf = Wf = C = 4
    Rn = 65535
    img_h, img_w = IMG_OF[(4, 4)]
    feat = torch.randn(1, C, Hf, Wf, generator=torch.Generator().manual_seed(43))
    five = R.map_to_image(torch.tensor([[0, 0, 3, 3], [1, 1, 2, 3], [2.5, 0.5, 3.5, 1.5], [-2, -2, 0, 1], [7, 7, 9, 9]],
                                       dtype=torch.float32), img_h, img_w, Hf, Wf)
    rois = five.repeat(Rn // 5, 1)[None]
    d_out = d_out_of(Rn, C)
    am = G.pool_argmax(feat, five[None], (0,), img_h, img_w, 1, 1)
    per = lambda rows: G.pool_grad_ref(feat, five[None], (0,), img_h, img_w, rows, 1, 1, argmax=am)[0]   # noqa: E731
    want = per(torch.stack([d_out[j::5].double().sum(0) for j in range(5)]))
    T = per(torch.stack([d_out[j::5].double().abs().sum(0) for j in range(5)]))
    N = per(torch.full((5, C), float(Rn // 5), dtype=torch.float64)).round().long()
    return feat, rois, img_h, img_w, d_out, (want, T, N)


def test_case_conditions_grid_limit():
    feat, rois, img_h, img_w, d_out, (want, T, N) = grid_limit_case()
    assert rois.shape[1] == 65535 and rois.shape[1] % 5 == 0
    assert int(N.max()) >= 13107 and int(N.sum()) == 4 * 4 * 13107       # four RoIs with a winner per channel, one without
    assert bool(torch.equal(rois[0, :5], rois[0, 65530:]))


@gpu
def test_pool_grid_limit(ffi, dev):
    feat, rois, img_h, img_w, d_out, ref = grid_limit_case()
    r = check_against(ffi, dev, "pool", feat, rois, (0,), img_h, img_w, d_out, ref, 1, 1, what="B R = 65535")
    record(KERNEL["pool"], "B R = 65535", [65535], r)


# ------------------------------------------------------------------------------------------------------------- refusals
def small_case(Hf=4, Wf=4, Rn=5, C=4):
    feat = torch.randn(1, C, Hf, Wf, generator=torch.Generator().manual_seed(3))
    rois = R.rand_boxes(torch.Generator().manual_seed(4), Rn, span=40.0, wh=20.0)[None]
    return feat, rois, d_out_of(Rn, C)


@gpu
def test_refusals_leave_d_feat_untouched(ffi, dev):
    """The status code of every refusal, and d_feat as it was: nothing was launched."""
    feat, rois, d_out = small_case()
    call = lambda op, expect, **bad: launch(ffi, dev, op, feat, rois, (0,), 61, 62, d_out, 2, 2, expect=expect, bad=bad)  # noqa: E731
    for op in ("pool", "align"):
        assert call(op, OK) is not None
        call(op, ERR_ALIGNMENT, C=3)
        call(op, ERR_ALIGNMENT, C=6)
        call(op, ERR_ALIGNMENT, d_out_pitch=10)
        call(op, ERR_ALIGNMENT, d_feat_pitch=18)
        call(op, ERR_ALIGNMENT, d_out_pitch=0)                              # a pitch < C
        call(op, ERR_ALIGNMENT, d_feat_pitch=0)
        for name in ("rois_ptr", "d_out_ptr", "d_feat_ptr"):             # 4 bytes off a 16-byte boundary, in a large buffer
            call(op, ERR_ALIGNMENT, **{name: ffi.ptr(torch.zeros(4096, device=dev)) + 4})
        call(op, ERR_INVALID_ARG, img_h=0.0)
        call(op, ERR_INVALID_ARG, img_h=-5.0)
        L = ffi.lib()
        need = (L.tsod_roi_pool_avg_grad_workspace_bytes(1, 5, 4, 2, 2) if op == "pool"
                else L.tsod_roi_align_avg_grad_workspace_bytes(1, 5))
        call(op, ERR_WORKSPACE, ws_bytes=need - 1)
        call(op, ERR_WORKSPACE, ws=0)
        spare = torch.zeros(need + 64, dtype=torch.uint8, device=dev)
        call(op, ERR_WORKSPACE, ws=ffi.ptr(spare) + 4)
    call("pool", ERR_ALIGNMENT, feat_pitch=10)
    call("pool", ERR_ALIGNMENT, feat_pitch=0)
    call("pool", ERR_ALIGNMENT, feat_ptr=ffi.ptr(torch.zeros(4096, device=dev)) + 4)
    call("align", ERR_INVALID_ARG, sr=-1)


@gpu
def test_pool_refuses_a_map_beyond_the_u16_record(ffi, dev):
    feat = torch.zeros(1, 4, 256, 256)
    rois = R.rand_boxes(torch.Generator().manual_seed(4), 3, span=40.0, wh=20.0)[None]
    launch(ffi, dev, "pool", feat, rois, (0,), 1024, 1024, d_out_of(3, 4), 2, 2, expect=ERR_UNSUPPORTED)
    assert launch(ffi, dev, "align", feat, rois, (0,), 1024, 1024, d_out_of(3, 4), 2, 2) is not None


@gpu
def test_pool_refuses_more_rois_than_the_grid_holds(ffi, dev):
    feat, _, _ = small_case()
    rois = R.rand_boxes(torch.Generator().manual_seed(4), 65536, span=40.0, wh=20.0)[None]
    launch(ffi, dev, "pool", feat, rois, (0,), 61, 62, d_out_of(65536, 4), 1, 1, expect=ERR_INVALID_ARG)


# ------------------------------------------------------------------------------------------- against the forward kernels
def device_adjoint(dev, op, feat, rois, idx, img_h, img_w, d_out, PH, PW, sr, aligned, ref_T_N):
    """<forward kernel(feat), d> against <feat, backward kernel(d)>, both summed in float64 on the host -> |lhs - rhs| / bar
    with bar = sum of the forward's bar |d| + sum of the backward's bar |feat|."""
    from two_stage_object_detection_amd import hip_ops
    fd = feat.permute(0, 2, 3, 1).contiguous().to(dev)
    r, i = rois.to(dev), torch.tensor(idx, dtype=torch.int32, device=dev)
    rois5 = R.rois5_of(R.roi_to_map(rois, img_h, img_w, feat.shape[2], feat.shape[3]), torch.tensor(idx), rois.shape[1])
    if op == "pool":
        fwd = hip_ops.roi_pool_avg_nhwc(fd, r, i, img_h, img_w, (PH, PW))
        bwd = hip_ops.roi_pool_avg_grad_nhwc(fd, r, i, img_h, img_w, d_out.to(dev), (PH, PW))
        fwd_bar = R.roi_pool_avg_ref(feat, rois5, PH, PW)[1]
    else:
        fwd = hip_ops.roi_align_avg_nhwc(fd, r, i, img_h, img_w, (PH, PW), 1.0, sr, aligned)
        bwd = hip_ops.roi_align_avg_grad_nhwc(tuple(fd.shape), r, i, img_h, img_w, d_out.to(dev), (PH, PW), 1.0, sr, aligned)
        fwd_bar = R.roi_align_avg_ref(feat, rois5, PH, PW, sr, aligned)[1]
    T, N = ref_T_N
    bwd = bwd.cpu().permute(0, 3, 1, 2).double()
    lhs = float((fwd.cpu().double() * d_out.double()).sum())
    rhs = float((feat.double() * bwd).sum())
    bar = float((fwd_bar * d_out.double().abs()).sum()) + float((bar_of(op, T, N) * feat.double().abs()).sum())
    assert float((fwd.cpu().double().abs() * d_out.double().abs()).sum()) > 1.0      # the sums are not trivially small
    return abs(lhs - rhs) / bar, lhs, rhs


@gpu
@pytest.mark.parametrize("op", ["pool", "align"])
def test_backward_is_the_adjoint_of_the_forward_kernels(dev, op):
    """The 13 x 11, C = 260 case (a finite map), every sampling_ratio x aligned."""
    worst = 0.0
    for sr, aligned in (ALIGN_MODES if op == "align" else ((2, False),)):
        feat, rois, img_h, img_w, d_out, ref = reference(op, "geometry", "marked", 13, 11, 2, 260, 1.0, (1, 0), 7, 7, sr, aligned)
        ratio, lhs, rhs = device_adjoint(dev, op, feat, rois, (1, 0), img_h, img_w, d_out, 7, 7, sr, aligned, ref[1:])
        assert ratio <= 1.0, (sr, aligned, lhs, rhs, ratio)
        worst = max(worst, ratio)
    record(KERNEL[op], "adjoint of the forward kernel", [13, 11, 260], worst)


@gpu
@pytest.mark.parametrize("op", ["pool", "align"])
def test_backward_is_the_adjoint_of_the_forward_kernels_full_size(dev, op):
    """50 x 84 x 512, B = 2, R = 32, once: the adjoint needs no reference gradient (the walk only counts the addends)."""
    Hf, Wf, C, B, Rn = 50, 84, 512, 2, 32
    img_h, img_w = IMG_OF[(Hf, Wf)]
    g = torch.Generator().manual_seed(50)
    feat = torch.randn(B, C, Hf, Wf, generator=g)
    rois = torch.stack([R.rand_boxes(g, Rn, span=1200.0, wh=500.0) - 60.0 for _ in range(B)])
    d_out = d_out_of(B * Rn, C)
    if op == "pool":
        _, T, N = G.pool_grad_ref(feat, rois, (1, 0), img_h, img_w, d_out)
    else:
        _, T, N = G.align_grad_ref(tuple(feat.shape), rois, (1, 0), img_h, img_w, d_out)
    ratio, lhs, rhs = device_adjoint(dev, op, feat, rois, (1, 0), img_h, img_w, d_out, 7, 7, 2, False, (T, N))
    assert ratio <= 1.0, (lhs, rhs, ratio)
    record(KERNEL[op], "adjoint of the forward kernel", [Hf, Wf, C], ratio)


# ------------------------------------------------------------------------------------------------- channel independence
@gpu
@pytest.mark.parametrize("op", ["pool", "align"])
def test_channels_do_not_depend_on_their_neighbours(ffi, dev, op):
    """Channels [4, 12) computed alone (the pointers moved to channel 4 of the same buffers, C = 8) are, bit for bit, the same
    channels of the C = 260 run: the owner of an element never depends on the other lanes."""
    feat, rois, img_h, img_w, d_out, _ = reference(op, "geometry", "marked", 13, 11, 2, 260, 1.0, (1, 0), 7, 7)
    for base in (None, base_of(tuple(feat.shape))):
        whole = launch(ffi, dev, op, feat, rois, (1, 0), img_h, img_w, d_out, 7, 7, base=base)
        alone = launch(ffi, dev, op, feat, rois, (1, 0), img_h, img_w, d_out, 7, 7, base=base, channels=(4, 8))
        assert tuple(alone.shape) == (2, 8, 13, 11)
        assert torch.equal(bits(alone), bits(whole[:, 4:12]))
