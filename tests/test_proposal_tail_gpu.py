"""The proposal tail (RPN decode, top-k, NMS, RoI pool / align) and the detection tail (records, score filter, sort, gather,
class-aware NMS) at every point where their launch code changes behaviour, against the plain CPU references of
tests/proposal_tail_restated.py with the bars stated there: the second trip of the seven grid-stride loops, NMS at counts
of 0, 1 and multiples of 64, its conflict-free shortcut, chains across block edges and its upper caps, the pitch
arguments, the PH > 8 passes, the dead lanes, the grid switch and the column reuse of the RoI kernels, the top-k kernels on
both sides of each size switch, and the record kernel at class counts around a wave.

Exact results (indices, keys, gathers, maxima) are compared bit for bit.  Every case with a tolerance prints its largest
err / bar; with TSOD_PROPOSAL_TAIL_JSONL=<path> the same figures are appended to that file, one JSON line each
(TSOD_PROPOSAL_TAIL_COMMIT names the commit in them)."""
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle.box import nms_python, roi_pool_python

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proposal_tail_restated as R  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "two_stage_object_detection_amd", "csrc")
SENTINEL = -7.25          # what the columns around an output slice hold before a launch, and must hold after it
FAR = 1.0e6               # what the columns around an input slice hold: one wrong column read cannot stay inside a bar
GUARD = 64                # floats of SENTINEL behind a dense output
GRID_CAP = 4096 * 256     # elements one trip of a capped grid covers


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
            "commit": os.environ.get("TSOD_PROPOSAL_TAIL_COMMIT", "unknown")}
    print("proposal_tail:", json.dumps(line))
    path = os.environ.get("TSOD_PROPOSAL_TAIL_JSONL")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def ratio_of(got, ref, bar):
    """The largest |got - ref| / bar (bar a number or a tensor), in f64."""
    err = (got.detach().cpu().double() - ref.double()).abs()
    bar = torch.as_tensor(bar, dtype=torch.float64)
    return float((err / bar.clamp_min(1e-300)).max())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def big_rpn_case():
    return R.big_rpn_case()


def assert_keys(keys, score, keep_ref, side, min_size, what):
    """keys (device result) must be `score` bit for bit where the box is kept and -inf elsewhere, and the kept set may differ
    from the reference's only at the border boxes.  All 1-d CPU tensors."""
    kept = keys != R.NEG_INF
    assert not torch.isnan(keys).any(), what
    diff = kept != keep_ref
    assert bool(R.border_boxes(side, min_size)[diff].all()), f"{what}: {int(diff.sum())} min-size decisions differ off the border"
    assert torch.equal(bits(keys[kept]), bits(score[kept])), what
    assert bool((keys[~kept] == R.NEG_INF).all()), what


# ============================================================================= the restatements, on the CPU
def test_restatements_match_the_oracle_on_small_inputs():
    """Every restatement against oracle.* (or a plain loop) on small inputs, without a GPU."""
    g = torch.Generator().manual_seed(3)
    base = oracle.generate_basic_anchor()
    A, B, Hf, Wf, stride = base.shape[0], 2, 9, 11, 16
    locs = torch.randn(B * Hf * Wf, 4 * A, generator=g) * 0.4
    scores = torch.randn(B * Hf * Wf, 2 * A, generator=g) * 2
    H, W = Hf * stride, Wf * stride
    anchor, boxes, fg, keep, side = R.rpn_decode_ref(locs, scores, base, B, Hf, Wf, stride, H, W, 16.0)
    for b in range(B):                         # the proposal layer's own decode, clamp and min-size mask (img_size[1], [2])
        _, dbg = oracle.proposal_layer(locs.view(B, -1, 4)[b], fg[b], anchor, (3, H, W), return_debug=True)
        assert torch.equal(dbg["decoded"], boxes[b]) and torch.equal(dbg["valid"], keep[b])
    assert torch.equal(fg, F.softmax(scores.view(B, -1, 2), dim=-1)[:, :, 1])
    assert bool((side[keep] >= 16).all()) and bool((side[~keep] < 16).all())

    det = R.overlapping_records(5, B=1, R=40)[0]
    det[3, 4], det[4, 4], det[5, 4] = float("nan"), R.NEG_INF, 0.25
    for thr, bg in ((0.25, 0), (R.NEG_INF, -1), (0.0, 3)):
        keys = R.detection_keys_ref(det, thr, bg)
        want = oracle.postprocess(det.unsqueeze(0), 1.0, score_thresh=None if thr == R.NEG_INF else thr, background_class=bg)[0]
        kept = det[torch.isfinite(keys)]
        assert torch.equal(kept[torch.sort(kept[:, 4], descending=True, stable=True).indices], want)
        assert keys[3] == R.NEG_INF and keys[4] == R.NEG_INF and not torch.isnan(keys).any()
        assert torch.equal(bits(keys[torch.isfinite(keys)]), bits(det[torch.isfinite(keys), 4]))
    assert R.detection_keys_ref(det, 0.25, -1)[5] == 0.25           # exactly the threshold passes

    src = torch.randn(2, 5, 3, generator=g)
    idx = torch.tensor([[0, 4, -1, 5, 2, 2, -7], [4, 3, 99, 0, 1, -1, 2]], dtype=torch.int32)
    got = R.gather_rows_ref(src, idx)
    for b in range(2):
        for r in range(7):
            i = int(idx[b, r])
            assert torch.equal(got[b, r], src[b, i] if 0 <= i < 5 else torch.zeros(3))

    keys = torch.tensor([0.5, R.NEG_INF, 0.75, 0.5, 0.75, R.NEG_INF, 0.25])
    assert R.stable_topk_ref(keys, 4).tolist() == [2, 4, 0, 3] and R.stable_topk_ref(keys, 9).tolist() == [2, 4, 0, 3, 6]

    bx = (R.rand_boxes(g, 40, span=100.0, wh=60.0) / 10).round() * 10
    keep = R.nms_keep_ref(bx, 37, 0.5)
    assert keep.tolist() == nms_python(bx[:37].numpy(), np.arange(37, 0, -1, dtype=np.float32), 0.5)
    k = keep.numel()
    rc, out = R.nms_pad_ref(bx, 37, 0.5, k + 5)
    assert rc == k and out.tolist() == keep.tolist() + [0, 1, 2, 3, 4]
    assert R.nms_pad_ref(bx, 37, 0.5, k + 38)[0] == -2 and R.nms_pad_ref(bx, 0, 0.5, 1)[0] == -2
    assert R.nms_keep_ref(bx, 0, 0.5).numel() == 0 and R.nms_pad_ref(bx, 37, 0.5, 3)[1].tolist() == keep[:3].tolist()

    # the RoI geometry list goes through the C oracle as through the plain loop restatement, and the f64 mean of the bins
    # is the classifier's mean to within the sum bar
    for Hf, Wf in ((6, 6), (13, 17)):
        feat = R.marked_map(g, 2, 4, Hf, Wf)
        fm = R.geometry_rois(g, Hf, Wf)
        assert fm.shape[0] == 8 + R.GEOMETRY_NAMED
        rois5 = R.rois5_of(torch.cat([fm, fm]), torch.tensor([1, 0]), fm.shape[0])
        for PH, PW in ((7, 7), (9, 5), (17, 3), (1, 1)):
            m = oracle.roi_pool(feat, rois5, (PH, PW), 1.0)
            assert np.array_equal(m.numpy(), roi_pool_python(feat.numpy(), rois5.numpy(), (PH, PW), 1.0))
            mean, bar = R.roi_pool_avg_ref(feat, rois5, PH, PW)
            assert bool(((F.adaptive_avg_pool2d(m, 1).flatten(1).double() - mean).abs() <= bar).all())
            a = oracle.roi_align(feat, rois5, (PH, PW), 1.0, 2, False)
            mean, bar = R.roi_align_avg_ref(feat, rois5, PH, PW, 2, False)
            assert torch.equal(mean, a.double().mean(dim=(2, 3))) and bool((bar >= R.BIN_BAR).all())
        # image coordinates that come back to the map coordinates: the .5 RoIs land on .5 exactly
        img_h, img_w = IMG_OF[(Hf, Wf)]
        back = R.roi_to_map(R.map_to_image(fm, img_h, img_w, Hf, Wf), img_h, img_w, Hf, Wf)
        assert torch.equal(back[list(R.HALF_ROWS)], fm[list(R.HALF_ROWS)])
        assert float((back - fm).abs().max()) < 1e-4
        assert img_h % Hf and img_w % Wf


def test_sum_bar_bounds_an_f32_sum_in_the_kernels_order():
    """sum_bar on known values, and against an f32 sum taken in the kernels' order (bins of a row, then rows, then one divide)
    on values of mixed sign and scale."""
    assert R.SUM_ROUNDINGS(7, 7) == 15 and R.SUM_ROUNDINGS(17, 3) == 21
    ones = torch.ones(1, 1, 2, 3)
    assert float(R.sum_bar(ones, 2, 3)) == 6 * R.U
    assert float(R.sum_bar(-3 * ones, 2, 3)) == 18 * R.U
    g = torch.Generator().manual_seed(4)
    worst = 0.0
    for PH, PW in ((7, 7), (8, 3), (9, 5), (17, 3), (1, 1)):
        m = (torch.randn(64, 32, PH, PW, generator=g) * torch.exp(torch.randn(64, 32, PH, PW, generator=g) * 3)).float()
        rows = torch.zeros(64, 32, PH)
        for pw in range(PW):
            rows = rows + m[..., pw]
        total = torch.zeros(64, 32)
        for ph in range(PH):
            total = total + rows[..., ph]
        got = total / float(PH * PW)
        mean, bar = R.mean_and_bar(m)
        assert bool(((got.double() - mean).abs() <= bar).all())
        worst = max(worst, ratio_of(got, mean, bar))
    assert 0.0 < worst <= 1.0


def test_reference_side_conditions():
    """What the GPU cases rely on, on the reference's side: the border boxes of the big decode case stay under the cap, the
    200 disjoint boxes are all kept, and the chain keeps every other box (shifted by one leading box: the other parity)."""
    c = big_rpn_case()
    assert c["n"] == 1062882 and c["n"] > GRID_CAP
    border = R.border_boxes(c["side"], c["min_size"])
    print("border boxes of the reference:", int(border.sum()), "of", c["n"])
    assert int(border.sum()) <= R.BORDER_CAP * c["n"]
    assert 0.05 < float(c["keep"].float().mean()) < 0.999          # the mask is exercised on both sides
    d = R.disjoint_boxes(200)
    assert R.nms_keep_ref(d, 200, 0.7).tolist() == list(range(200))
    assert R.nms_keep_ref(R.chain_boxes(200), 200, 0.7).tolist() == list(range(0, 200, 2))
    assert R.nms_keep_ref(R.chain_boxes(200, lead=1), 200, 0.7).tolist() == [0] + list(range(1, 200, 2))


TOPK_SWITCHES = [  # (B, n, n_pre) below the switch, the same above it
    ((1, 17320, 3000), (1, 17321, 3000)),       # full rank | select + rank
    ((3, 10240, 3000), (3, 10241, 3000)),       # 10 | 20 keys per thread
    ((1, 20480, 6000), (1, 20481, 6000)),       # 20 | 40
    ((1, 40960, 3000), (1, 40961, 3000)),       # 40 | 80
    ((1, 81920, 3000), (1, 81921, 3000)),       # 80 keys per thread | streaming
]
TOPK_STRIPS = [((1, 20000, 1024), (1, 20000, 1025)),      # 16 | 17 64-blocks of candidates for the 16 waves
               ((1, 40000, 8192), (1, 40000, 8193))]      # a wave's strip fits its 512-entry window | needs a second pass


def test_topk_path_restates_the_launch_rule():
    """topk_path against the text of tsod_sort_topk_desc_ws_f32 (a changed rule must change the restatement, or the cases
    below silently stop straddling their switches), and every pair of cases on the two sides of its switch."""
    with open(os.path.join(CSRC, "sort_topk.hip")) as f:
        src = f.read()
    assert float(re.search(r"constexpr double kFullRankWork = ([0-9.e]+);", src).group(1)) == R.TOPK_FULL_RANK_WORK
    assert int(re.search(r"constexpr int kThreads = (\d+);", src).group(1)) == R.TOPK_THREADS
    assert re.search(r"\(double\)B \* n \* n <= kFullRankWork", src)
    ladder = [int(k) for k in re.findall(r"if \(n <= (\d+) \* kThreads\) TSOD_SORT\(\1\);", src)]
    last = int(re.search(r"else TSOD_SORT\((\d+)\);", src).group(1))
    assert tuple(ladder + [last]) == R.TOPK_KPT
    assert int(re.search(r"if \(n > (\d+) \* kThreads\) \{", src).group(1)) == R.TOPK_KPT[-1]
    assert int(re.search(r"constexpr int kRankParts = (\d+);", src).group(1)) == R.TOPK_RANK_PARTS
    assert int(re.search(r"constexpr int kRankMaxPer = (\d+);", src).group(1)) == R.TOPK_RANK_STRIP
    paths = [(R.topk_path(*lo), R.topk_path(*hi)) for lo, hi in TOPK_SWITCHES]
    assert paths == [(("full",), ("select", 20)), (("select", 10), ("select", 20)), (("select", 20), ("select", 40)),
                     (("select", 40), ("select", 80)), (("select", 80), ("stream",))]
    assert 17320 * 17320 == 299982400
    for lo, hi in TOPK_STRIPS:
        assert R.topk_path(*lo)[0] == R.topk_path(*hi)[0] == "select"
    assert [R.rank_strip(lo[2]) + R.rank_strip(hi[2]) for lo, hi in TOPK_STRIPS] == [(16, 1, 17, 1), (128, 1, 129, 2)]


# ============================================================================= 1. grid-stride trips
@gpu
def test_rpn_decode_second_grid_trip_pitched(ops, dev):
    """1 062 882 boxes (> 4096 blocks x 256 threads) with locs and scores as column slices of wider buffers."""
    c = big_rpn_case()
    A, B = c["A"], c["B"]
    rows = c["locs"].shape[0]
    lw = torch.full((rows, 4 * A + 8), FAR)
    sw = torch.full((rows, 2 * A + 6), FAR)
    lw[:, 4:4 + 4 * A] = c["locs"]
    sw[:, 3:3 + 2 * A] = c["scores"]
    lw, sw = lw.to(dev), sw.to(dev)
    boxes, fg, keys, anchors = ops.rpn_decode(lw[:, 4:4 + 4 * A], sw[:, 3:3 + 2 * A], c["base"].to(dev), B, c["Hf"], c["Wf"],
                                              c["stride"], c["clamp_x"], c["clamp_y"], c["min_size"], want_anchors=True)
    assert torch.equal(anchors.cpu(), c["anchor"])
    r_fg, r_box = ratio_of(fg, c["fg"], 1e-6), ratio_of(boxes, c["boxes"], 1e-3)
    record("rpn_decode", "pitched, two grid trips", [B, c["Hf"], c["Wf"], A], max(r_fg, r_box))
    assert r_fg < 1.0 and r_box < 1.0
    assert int(R.border_boxes(c["side"], c["min_size"]).sum()) <= R.BORDER_CAP * c["n"]
    assert_keys(keys.cpu().flatten(), fg.cpu().flatten(), c["keep"].flatten(), c["side"].flatten(), c["min_size"], "rpn_decode")


@gpu
def test_proposal_decode_second_grid_trip(ops, dev):
    c = big_rpn_case()
    n = c["n"]
    anchor = c["anchor"].repeat(c["B"], 1)
    loc = c["locs"].reshape(n, 4)
    score = torch.rand(n, generator=torch.Generator().manual_seed(21))
    ref, keep, side = c["boxes"].reshape(n, 4), c["keep"].flatten(), c["side"].flatten()
    for m in (n, 1):
        boxes, keys = ops.proposal_decode(anchor[:m].to(dev), loc[:m].to(dev), score[:m].to(dev), c["clamp_x"], c["clamp_y"],
                                          c["min_size"])
        r = ratio_of(boxes, ref[:m], 1e-3)
        record("proposal_decode", "two grid trips" if m > GRID_CAP else "one box", [m], r)
        assert r < 1.0
        assert_keys(keys.cpu(), score[:m], keep[:m], side[:m], c["min_size"], f"proposal_decode n={m}")


@gpu
def test_loc2bbox_bbox2loc_second_grid_trip(ops, dev):
    n = GRID_CAP + 3
    g = torch.Generator().manual_seed(22)
    src = R.rand_boxes(g, n, span=100.0, wh=60.0)
    loc = torch.randn(n, 4, generator=g) * 0.4
    r = ratio_of(ops.loc2bbox(src.to(dev), loc.to(dev)), oracle.loc2bbox(src, loc), 2e-4)
    record("loc2bbox", "two grid trips", [n], r)
    assert r <= 1.0
    xy, xy2 = torch.rand(n, 2, generator=g) * 700, torch.rand(n, 2, generator=g) * 700
    a = torch.cat([xy, xy + torch.rand(n, 2, generator=g) * 300 + 0.5], dim=1)
    b = torch.cat([xy2, xy2 + torch.rand(n, 2, generator=g) * 300 + 0.5], dim=1)
    a[7, 2], a[GRID_CAP + 1, 3] = a[7, 0], a[GRID_CAP + 1, 1]             # zero width / height: floored at eps like the reference
    ref = R.bbox2loc_ref(a, b)
    got = ops.bbox2loc(a.to(dev), b.to(dev)).cpu()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin)
    rel = ((got - ref).abs() / ref.abs().clamp_min(1.0))[fin]
    record("bbox2loc", "two grid trips", [n], float(rel.max()) / 2e-6)
    assert float(rel.max()) <= 2e-6


@gpu
def test_enumerate_anchors_second_grid_trip(ops, dev):
    base = oracle.generate_basic_anchor()
    # a thread writes one anchor: the 243 x 243 x 9 grid of the decode cases (531 441 anchors) stays inside one trip of the
    # 4096 x 256 threads, 342 x 342 x 9 = 1 052 676 is the smallest square grid that does not
    assert 243 * 243 * 9 < 341 * 341 * 9 < GRID_CAP < 342 * 342 * 9
    for Hf, Wf in ((243, 243), (342, 342)):
        got = ops.enumerate_anchors(base.to(dev), 16, Hf, Wf).cpu()
        assert torch.equal(got, oracle.enumerate_shifted_anchor(base, 16, Hf, Wf)), (Hf, Wf)


@gpu
def test_detection_keys_second_grid_trip(ffi, dev):
    n = GRID_CAP + 5
    g = torch.Generator().manual_seed(23)
    det = torch.cat([R.rand_boxes(g, n), (torch.randn(n, 1, generator=g) * 8).round() / 8,
                     torch.randint(0, 21, (n, 1), generator=g).float()], dim=1)
    thr = 0.25
    for at in (0, 1000, GRID_CAP - 1, GRID_CAP, n - 5):           # both trips get every special score
        det[at, 4], det[at + 1, 4], det[at + 2, 4], det[at + 3, 4] = float("nan"), R.NEG_INF, thr, 5.0
        det[at + 3, 5], det[at + 2, 5] = 0.0, 1.0                  # a background record above the threshold; one exactly at it
    d = det.to(dev)
    for background in (0, -1):
        keys = torch.full((n + GUARD,), SENTINEL, device=dev)
        ffi.check(ffi.lib().tsod_detection_keys_f32(ffi.ptr(d), n, thr, background, ffi.ptr(keys), ffi.stream_ptr()), "detection_keys")
        ref = R.detection_keys_ref(det, thr, background)
        assert torch.equal(bits(keys[:n]), bits(ref)), f"background_class={background}"
        assert bool((keys[n:] == SENTINEL).all())
        assert ref[GRID_CAP + 2] == thr and (ref[GRID_CAP + 3] == 5.0) == (background < 0)


@gpu
@pytest.mark.parametrize("B,n,m,C", [(3, 50000, 60000, 6), (3, 50000, 60000, 1), (2, 700, 1, 6)])
def test_gather_rows_second_grid_trip(ffi, dev, B, n, m, C):
    g = torch.Generator().manual_seed(24)
    src = torch.randn(B, n, C, generator=g)
    idx = torch.randint(-n // 8, n + n // 8, (B, m), generator=g, dtype=torch.int32)
    flat = idx.view(-1)
    flat[0], flat[-1] = -1, n                                       # the two edges of the valid range
    if flat.numel() > 4:
        flat[1], flat[2], flat[3] = 0, n - 1, -(2 ** 31)
    out = torch.full((B * m * C + GUARD,), SENTINEL, device=dev)
    sd, idev = src.to(dev), idx.to(dev)                             # (named: a temporary's memory is reused by the next one)
    ffi.check(ffi.lib().tsod_gather_rows_f32(ffi.ptr(sd), ffi.ptr(idev), B, n, m, C, ffi.ptr(out), ffi.stream_ptr()), "gather_rows")
    assert torch.equal(bits(out[:B * m * C].view(B, m, C)), bits(R.gather_rows_ref(src, idx)))
    assert bool((out[B * m * C:] == SENTINEL).all())
    assert (B * m * C > GRID_CAP) == (m == 60000 and C == 6)


# ============================================================================= 2. NMS
def check_nms(ops, dev, boxes, counts, thr, n_post, expect_clean=False):
    """tsod_nms_f32 on [B,n_max,4] against oracle_nms_pad, image by image; -> the status word."""
    keep, rois, n_kept, status = ops.nms_sorted(boxes.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), thr, n_post)
    keep, rois, n_kept, status = keep.cpu().long(), rois.cpu(), n_kept.cpu(), int(status.item())
    overflow = False
    for b, n in enumerate(counts):
        rc, ref = R.nms_pad_ref(boxes[b], n, thr, n_post)
        k = min(R.nms_keep_ref(boxes[b], n, thr).numel(), n_post)
        assert int(n_kept[b]) == k, f"image {b} (n = {n}, n_post = {n_post})"
        if rc == -2:                      # the reference raises here: status bit 0, and only the survivors are compared
            overflow = True
            assert torch.equal(keep[b, :k], ref[:k]) and torch.equal(rois[b, :k], boxes[b][ref[:k]]), f"image {b} (n = {n})"
        else:
            assert rc >= 0 and torch.equal(keep[b], ref), f"image {b} (n = {n}, n_post = {n_post})"
            assert torch.equal(rois[b], boxes[b][ref]), f"image {b} (n = {n})"
    assert (status & 1) == int(overflow) and status in (0, 1)
    assert not (expect_clean and overflow)
    return status


NMS_COUNTS = [0, 1, 63, 64, 65, 128, 199, 200]


@gpu
@pytest.mark.parametrize("n_post", [1, 64, 65, 150])
def test_nms_counts_and_padding(ops, dev, n_post):
    """Counts of 0, 1 and around the multiples of 64 beside each other in one batch; then the images of that batch whose pad
    does not overflow as a batch of their own, where the status word must stay 0."""
    g = torch.Generator().manual_seed(25)
    boxes = torch.stack([R.dense_boxes(g, 200) for _ in NMS_COUNTS])
    boxes[3] = (boxes[3] / 4).round() * 4                           # duplicates and IoUs exactly at the threshold
    assert check_nms(ops, dev, boxes, NMS_COUNTS, 0.7, n_post) == 1           # count 0 always overflows its pad
    clean = [b for b, n in enumerate(NMS_COUNTS) if R.nms_pad_ref(boxes[b], n, 0.7, n_post)[0] >= 0]
    assert len(clean) >= 2 and 200 in [NMS_COUNTS[b] for b in clean]
    assert check_nms(ops, dev, boxes[clean], [NMS_COUNTS[b] for b in clean], 0.7, n_post, expect_clean=True) == 0


@gpu
@pytest.mark.parametrize("n_post", [64, 65, 128, 130])
def test_nms_conflict_free_blocks_and_the_limit_at_a_block_edge(ops, dev, n_post):
    d = R.disjoint_boxes(200)
    keep, rois, n_kept, status = ops.nms_sorted(d.unsqueeze(0).to(dev), torch.tensor([200], dtype=torch.int32, device=dev), 0.7, n_post)
    assert keep.cpu().tolist() == [list(range(n_post))] and int(n_kept) == n_post and int(status) == 0
    assert torch.equal(rois.cpu()[0], d[:n_post])
    check_nms(ops, dev, torch.stack([d, d]), [200, n_post], 0.7, n_post, expect_clean=True)


@gpu
@pytest.mark.parametrize("lead", [0, 1])
def test_nms_chain_across_block_edges(ops, dev, lead):
    c = R.chain_boxes(200, lead)
    for n_post in (33, 100, 150):
        check_nms(ops, dev, torch.stack([c, c, c]), [200, 129, 128], 0.7, n_post, expect_clean=True)
    keep, _, n_kept, _ = ops.nms_sorted(c.unsqueeze(0).to(dev), torch.tensor([200], dtype=torch.int32, device=dev), 0.7, 100)
    assert int(n_kept) == 100
    assert keep.cpu()[0].tolist() == (list(range(0, 200, 2)) if lead == 0 else ([0] + list(range(1, 200, 2)))[:100])


@gpu
def test_nms_degenerate_sets(ops, dev):
    same = torch.tensor([[10.0, 20.0, 50.0, 80.0]]).repeat(200, 1)
    keep, _, n_kept, status = ops.nms_sorted(same.unsqueeze(0).to(dev), torch.tensor([200], dtype=torch.int32, device=dev), 0.7, 150)
    assert int(n_kept) == 1 and keep.cpu()[0].tolist() == [0] + list(range(149)) and int(status) == 0
    g = torch.Generator().manual_seed(26)
    pts = torch.rand(200, 2, generator=g) * 50
    pts[:70] = pts[0]                                               # identical points, distinct points ...
    zero = torch.cat([pts, pts], dim=1)
    zero[150:, 2] += 30.0                                           # ... and zero-height lines: 0 / 0 never suppresses
    assert R.nms_keep_ref(zero, 200, 0.7).tolist() == list(range(200))
    check_nms(ops, dev, torch.stack([same, zero, zero]), [200, 200, 77], 0.7, 150, expect_clean=True)
    check_nms(ops, dev, torch.stack([same, zero]), [200, 200], 0.7, 300)


@gpu
def test_nms_upper_cap(ops, dev):
    g = torch.Generator().manual_seed(27)
    boxes = R.rand_boxes(g, 16384, span=3000.0, wh=300.0)
    check_nms(ops, dev, boxes.unsqueeze(0), [16384], 0.7, 600, expect_clean=True)


DET_CASES = [(1, 300.0), (63, 300.0), (64, 300.0), (65, 300.0), (1000, 300.0), (8192, 300.0), (8192, 6000.0)]


@gpu
@pytest.mark.parametrize("per_class", [False, True])
@pytest.mark.parametrize("Rn,span", DET_CASES)
def test_detection_nms_through_filter_detections(ops, dev, Rn, span, per_class):
    """tsod_detection_nms_f32 (stride-6 records, label compare, no padding, n_post = R) at R around the 64-blocks and at its
    cap; image 1 is run a second time with every score under the threshold (counts = 0 beside a full image)."""
    det = R.overlapping_records(31 + Rn, B=2, R=Rn, span=span)
    empty = det.clone()
    empty[1, :, 4] -= 100.0
    for d, thr in ((det, None), (empty, -50.0)):
        ref = oracle.postprocess(d, 0.1, score_thresh=thr, per_class=per_class)
        det_sorted, keep, n_kept = ops.filter_detections(d.to(dev), 0.1, score_thresh=thr, per_class=per_class)
        det_sorted, keep, n_kept = det_sorted.cpu(), keep.cpu().long(), n_kept.cpu()
        for b in range(2):
            k = int(n_kept[b])
            assert k == ref[b].shape[0], f"image {b}: kept {k}, the reference {ref[b].shape[0]}"
            assert torch.equal(det_sorted[b][keep[b, :k]], ref[b]), f"image {b}"
            assert bool((keep[b, k:] == -1).all())
        assert thr is None or (int(n_kept[1]) == 0 and int(n_kept[0]) > 0)
        if Rn == 8192:                       # span 6000: thousands of survivors (dozens of gather rounds per lane); 300: few
            assert (int(n_kept[0]) > 2000) == (span > 1000), int(n_kept[0])


# ============================================================================= 3. RoI head
IMG_OF = {(6, 6): (101, 91), (13, 17): (203, 270)}                 # image sides that are no multiple of the map's
MAPS = [(6, 6), (13, 17)]


def nhwc_pitched(feat_nchw, pad, dev):
    """[B,C,H,W] -> device [B,H,W,C + pad] with FAR in the pad channels."""
    B, C, H, W = feat_nchw.shape
    buf = torch.full((B, H, W, C + pad), FAR)
    buf[..., :C] = feat_nchw.permute(0, 2, 3, 1)
    return buf.to(dev)


def plain_roi(ffi, dev, kind, buf, C, rois5, PH, PW, sampling_ratio=2, aligned=False):
    """tsod_roi_pool_f32 / tsod_roi_align_f32 through the ABI with feat_pitch = the buffer's width -> [K,C,PH,PW] on the CPU."""
    B, Hf, Wf, pitch = buf.shape
    K, n = rois5.shape[0], rois5.shape[0] * C * PH * PW
    out = torch.full((n + GUARD,), SENTINEL, device=dev)
    r = rois5.to(dev).contiguous()
    L = ffi.lib()
    if kind == "pool":
        rc = L.tsod_roi_pool_f32(ffi.ptr(buf), B, Hf, Wf, C, pitch, ffi.ptr(r), K, 1.0, PH, PW, ffi.ptr(out), ffi.stream_ptr())
    else:
        rc = L.tsod_roi_align_f32(ffi.ptr(buf), B, Hf, Wf, C, pitch, ffi.ptr(r), K, 1.0, PH, PW, sampling_ratio, int(aligned),
                                  ffi.ptr(out), ffi.stream_ptr())
    ffi.check(rc, "roi_" + kind)
    assert bool((out[n:] == SENTINEL).all())
    return out[:n].view(K, C, PH, PW).cpu()


def fused_roi(ffi, dev, kind, buf, C, rois, idx, img_h, img_w, PH, PW, sampling_ratio=2, aligned=False, out_pad=4):
    """tsod_roi_pool_avg_f32 / tsod_roi_align_avg_f32 through the ABI with both pitches wider than C -> [B*R,C] on the CPU."""
    B, Hf, Wf, pitch = buf.shape
    R_ = rois.shape[1]
    out = torch.full((B * R_, C + out_pad), SENTINEL, device=dev)
    r, i = rois.to(dev).contiguous(), idx.to(dev, torch.int32).contiguous()
    L = ffi.lib()
    if kind == "pool":
        rc = L.tsod_roi_pool_avg_f32(ffi.ptr(buf), B, Hf, Wf, C, pitch, ffi.ptr(r), ffi.ptr(i), R_, float(img_h), float(img_w), 1.0,
                                     PH, PW, ffi.ptr(out), C + out_pad, ffi.stream_ptr())
    else:
        rc = L.tsod_roi_align_avg_f32(ffi.ptr(buf), B, Hf, Wf, C, pitch, ffi.ptr(r), ffi.ptr(i), R_, float(img_h), float(img_w), 1.0,
                                      PH, PW, sampling_ratio, int(aligned), ffi.ptr(out), C + out_pad, ffi.stream_ptr())
    ffi.check(rc, f"roi_{kind}_avg")
    out = out.cpu()
    assert bool((out[:, C:] == SENTINEL).all()), "the pad columns of the output were written"
    return out[:, :C]


@functools.lru_cache(maxsize=None)
def roi_case(C, Hf, Wf):
    """One feature map and the geometry list for it, in both coordinate systems: B = 2, image indices permuted."""
    g = torch.Generator().manual_seed(1000 * C + Hf)
    feat = R.marked_map(g, 2, C, Hf, Wf)
    fm = torch.stack([R.geometry_rois(g, Hf, Wf), R.geometry_rois(g, Hf, Wf)])          # [2,K,4]
    img_h, img_w = IMG_OF[(Hf, Wf)]
    rois = R.map_to_image(fm, img_h, img_w, Hf, Wf)                                        # image coordinates
    idx = torch.tensor([1, 0], dtype=torch.int32)
    rois5 = R.rois5_of(R.roi_to_map(rois, img_h, img_w, Hf, Wf), idx, fm.shape[1])       # what the fused kernels derive
    return feat, rois, idx, rois5, img_h, img_w


@gpu
@pytest.mark.parametrize("Hf,Wf", MAPS)
@pytest.mark.parametrize("C", [4, 8, 132, 1028])
def test_roi_pool_and_align_plain_pitched(ffi, dev, C, Hf, Wf):
    """Quad counts 1, 2, 33 (dead lanes in a wave) and 257 (a second trip of the 256 threads), feat_pitch = C + 8."""
    feat, _, _, rois5, _, _ = roi_case(C, Hf, Wf)
    buf = nhwc_pitched(feat, 8, dev)
    worst = 0.0
    for PH, PW in ((7, 7), (1, 1), (9, 5)):
        assert torch.equal(plain_roi(ffi, dev, "pool", buf, C, rois5, PH, PW), oracle.roi_pool(feat, rois5, (PH, PW), 1.0)), (PH, PW)
        for sr in (0, 2, 3):
            for aligned in (False, True):
                got = plain_roi(ffi, dev, "align", buf, C, rois5, PH, PW, sr, aligned)
                r = ratio_of(got, oracle.roi_align(feat, rois5, (PH, PW), 1.0, sr, aligned), R.BIN_BAR)
                assert r <= 1.0, (PH, PW, sr, aligned, r)
                worst = max(worst, r)
    record("roi_align", "feat_pitch = C + 8", [C, Hf, Wf], worst)


FUSED_BINS = [(7, 7), (8, 3), (9, 5), (17, 3)]                     # the ph0 loop runs 1, 1, 2 and 3 passes (ragged last pass)


@gpu
@pytest.mark.parametrize("PH,PW", FUSED_BINS)
@pytest.mark.parametrize("C", [4, 132, 1028])
def test_roi_pool_avg_pitched(ffi, dev, C, PH, PW):
    """Channel groups 1, 2 (with dead lanes) and 9; feat_pitch = C + 8, out_pitch = C + 4."""
    worst = 0.0
    for Hf, Wf in MAPS:
        feat, rois, idx, rois5, img_h, img_w = roi_case(C, Hf, Wf)
        got = fused_roi(ffi, dev, "pool", nhwc_pitched(feat, 8, dev), C, rois, idx, img_h, img_w, PH, PW)
        mean, bar = R.roi_pool_avg_ref(feat, rois5, PH, PW)
        r = ratio_of(got, mean, bar)
        worst = max(worst, r)
        assert bool(((got.double() - mean).abs() <= bar).all()), (Hf, Wf, r)
    record("roi_pool_avg", "pitched", [C, PH, PW], worst)


@gpu
@pytest.mark.parametrize("PH,PW", FUSED_BINS)
@pytest.mark.parametrize("C", [4, 132, 1028])
def test_roi_align_avg_pitched(ffi, dev, C, PH, PW):
    worst = 0.0
    for Hf, Wf in MAPS:
        feat, rois, idx, rois5, img_h, img_w = roi_case(C, Hf, Wf)
        buf = nhwc_pitched(feat, 8, dev)
        for sr, aligned in ((2, False), (0, False), (3, True)):
            got = fused_roi(ffi, dev, "align", buf, C, rois, idx, img_h, img_w, PH, PW, sr, aligned)
            mean, bar = R.roi_align_avg_ref(feat, rois5, PH, PW, sr, aligned)
            r = ratio_of(got, mean, bar)
            worst = max(worst, r)
            assert bool(((got.double() - mean).abs() <= bar).all()), (Hf, Wf, sr, aligned, r)
    record("roi_align_avg", "pitched", [C, PH, PW], worst)


@gpu
@pytest.mark.parametrize("Rn", [65535, 65536])
def test_roi_avg_grid_switch(ops, dev, Rn):
    """B * R = 65535 keeps the RoI in the grid's y, 65536 moves it to x: the same RoIs on both sides of the switch."""
    g = torch.Generator().manual_seed(28)
    feat = torch.randn(1, 4, 4, 4, generator=g)
    rois = (R.rand_boxes(g, 65536, span=60.0, wh=30.0) - 4.0)[:Rn].unsqueeze(0)
    idx = torch.zeros(1, dtype=torch.int32)
    rois5 = R.rois5_of(R.roi_to_map(rois, 61, 67, 4, 4), idx, Rn)
    fd = feat.permute(0, 2, 3, 1).contiguous().to(dev)
    mean, bar = R.roi_pool_avg_ref(feat, rois5, 2, 2)
    got = ops.roi_pool_avg_nhwc(fd, rois.to(dev), idx.to(dev), 61, 67, (2, 2))
    assert tuple(got.shape) == (Rn, 4)
    r = ratio_of(got, mean, bar)
    assert bool(((got.cpu().double() - mean).abs() <= bar).all()), r
    mean, bar = R.roi_align_avg_ref(feat, rois5, 2, 2, 2, False)
    got = ops.roi_align_avg_nhwc(fd, rois.to(dev), idx.to(dev), 61, 67, (2, 2))
    r2 = ratio_of(got, mean, bar)
    assert bool(((got.cpu().double() - mean).abs() <= bar).all()), r2
    record("roi_pool_avg / roi_align_avg", "roi_in_y = %d" % (Rn <= 65535), [Rn], max(r, r2))


@gpu
@pytest.mark.parametrize("PH,PW", [(7, 7), (9, 5), (17, 3), (3, 16)])
def test_roi_pool_avg_column_reuse(ffi, dev, PH, PW):
    """The kept column of roi_pool_avg_kernel against the plain kernel, which reads every bin afresh: on a map whose rows
    each hold one large value, for every RoI of the geometry list, the fused mean must be the mean of the plain kernel's
    maxima to within the rounding of the sum."""
    worst = 0.0
    for C in (4, 132):
        for Hf, Wf in MAPS:
            feat, rois, idx, rois5, img_h, img_w = roi_case(C, Hf, Wf)
            buf = nhwc_pitched(feat, 8, dev)
            maxima = plain_roi(ffi, dev, "pool", buf, C, rois5, PH, PW)
            mean, bar = R.mean_and_bar(maxima)
            assert float(bar.max()) * 100 < 1.0 / (PH * PW)              # a wrong column costs >= 1 / (PH PW)
            got = fused_roi(ffi, dev, "pool", buf, C, rois, idx, img_h, img_w, PH, PW)
            r = ratio_of(got, mean, bar)
            worst = max(worst, r)
            assert bool(((got.double() - mean).abs() <= bar).all()), (C, Hf, Wf, r)
    record("roi_pool_avg", "column reuse against roi_pool", [PH, PW], worst)


# ============================================================================= 4. top-k switches
def check_topk(ops, ffi, dev, keys, boxes, n_pre):
    """Both entry points (the wrapper brings the scratch the library asks for, tsod_sort_topk_desc_f32 brings none) against
    torch's stable sort, and against each other."""
    B, n = keys.shape
    kd, bd = keys.to(dev), boxes.to(dev)
    got = ops.sort_topk_desc(kd, bd, n_pre)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    idx = torch.empty((B, n_pre), dtype=torch.int32, device=dev)
    bs = torch.empty((B, n_pre, 4), device=dev)
    ks = torch.empty((B, n_pre), device=dev)
    ffi.check(ffi.lib().tsod_sort_topk_desc_f32(ffi.ptr(kd), ffi.ptr(bd), B, n, n_pre, ffi.ptr(counts), ffi.ptr(idx), ffi.ptr(bs),
                                                ffi.ptr(ks), ffi.stream_ptr()), "sort_topk")
    for which, (c_, i_, b_, k_) in (("scratch", got), ("no scratch", (counts, idx, bs, ks))):
        c_, i_, b_, k_ = c_.cpu(), i_.cpu().long(), b_.cpu(), k_.cpu()
        for b in range(B):
            ref = R.stable_topk_ref(keys[b], n_pre)
            c = int(c_[b])
            assert c == ref.numel(), (which, b)
            assert torch.equal(i_[b, :c], ref), (which, b)
            assert bool((i_[b, c:] == -1).all()) and bool((b_[b, c:] == 0).all()) and bool((k_[b, c:] == R.NEG_INF).all()), (which, b)
            assert torch.equal(b_[b, :c], boxes[b][ref]) and torch.equal(k_[b, :c], keys[b][ref]), (which, b)
    for a, b_ in zip(got, (counts, idx, bs, ks)):
        assert torch.equal(a, b_)


@gpu
@pytest.mark.parametrize("B,n,n_pre", [t for pair in TOPK_SWITCHES + TOPK_STRIPS for t in pair])
def test_sort_topk_at_the_switches(ops, ffi, dev, B, n, n_pre):
    keys, boxes = R.topk_keys(B, n)
    check_topk(ops, ffi, dev, keys, boxes, n_pre)


@gpu
def test_sort_topk_ties_across_the_strip_edge(ops, ffi, dev):
    """Every finite key of the row equal: the whole order is the index rule, across the second pass of a wave's strip."""
    keys, boxes = R.topk_keys(1, 40000)
    keys[torch.isfinite(keys)] = 0.625
    check_topk(ops, ffi, dev, keys, boxes, 8193)


# ============================================================================= 5. the detection record kernel
@gpu
@pytest.mark.parametrize("n_class", [1, 2, 64, 65, 129])
def test_detections_pitched_rows_ties_and_nan(ops, dev, n_class):
    """Class counts around one wave, RoI counts that are no multiple of the four waves of a block, score and loc rows as slices
    of one wider matrix, ties between the first and the last class and between classes 63 and 64, one row with a NaN logit."""
    worst = 0.0
    for K in (1, 3, 5, 1001):
        g = torch.Generator().manual_seed(29 * n_class + K)
        wide = torch.full((1, K, 5 * n_class + 7), FAR)
        scores = torch.randn(1, K, n_class, generator=g)
        locs = torch.randn(1, K, 4 * n_class, generator=g) * 0.2
        scores[0, 0, 0] = scores[0, 0, n_class - 1] = 9.0                      # first and last class tie: the first wins
        if n_class > 64 and K > 2:
            scores[0, 1, 63] = scores[0, 1, 64] = 8.0                           # a tie across the lane wrap: class 63 wins
        if K > 2:
            scores[0, K - 1, n_class // 2] = float("nan")                       # NaN wins, as in torch.max
        wide[:, :, 2:2 + n_class] = scores
        wide[:, :, 5 + n_class:5 + 5 * n_class] = locs
        rois = R.rand_boxes(g, K, span=100.0, wh=60.0).unsqueeze(0)
        ref = oracle.detections_from_outputs(locs, scores, rois)
        wd = wide.to(dev)
        s_view, l_view = wd[:, :, 2:2 + n_class], wd[:, :, 5 + n_class:5 + 5 * n_class]
        assert ops._row_pitch(s_view, n_class) == 5 * n_class + 7 and ops._row_pitch(l_view, 4 * n_class) == 5 * n_class + 7
        got = ops.detections(l_view, s_view, rois.to(dev)).cpu()
        assert torch.equal(got[..., 5], ref[..., 5]), (n_class, K)
        assert torch.equal(bits(got[..., 4]), bits(ref[..., 4])), (n_class, K)
        assert got[0, 0, 5] == 0.0 and (K <= 2 or (got[0, K - 1, 5] == n_class // 2 and torch.isnan(got[0, K - 1, 4])))
        assert n_class <= 64 or K <= 2 or got[0, 1, 5] == 63.0
        r = ratio_of(got[..., :4], ref[..., :4], 1e-3)
        assert r < 1.0, (n_class, K, r)
        worst = max(worst, r)
    record("detections", "pitched rows", [n_class], worst)
