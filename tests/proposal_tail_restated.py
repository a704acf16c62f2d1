"""Plain CPU references for the proposal tail and the detection tail (csrc/rpn_decode.hip, sort_topk.hip, nms.hip,
roi_pool.hip), written from the reference's definitions in torch on the CPU, with the inputs and the bars
tests/test_proposal_tail_gpu.py holds the kernels to.  Nothing here imports the package under test; where oracle/ already
restates an op (loc2bbox, the anchor grid, RoIPool, RoIAlign, NMS and its pad, the detection records, postprocess) that
restatement is called, not copied.

The bars are derived, not measured.  With u = 2^-24 (f32 round to nearest):

  mean over the bins (roi_pool_avg, roi_align_avg)
      The kernels add the PW bins of a bin row in order (the first add, to 0, is exact: PW - 1 roundings), then the PH row
      sums in order (PH - 1 roundings), then divide once.  A value that took part in k rounded operations carries at most
      k u of its magnitude (to first order), so with m the exact f32 bin values
          |got - mean(m)| <= (PW - 1 + PH - 1 + 1) u sum|m| / (PH PW)   (+ O(u^2))
      and the bar is SUM_ROUNDINGS(PH, PW) u sum|m| / (PH PW) with SUM_ROUNDINGS = PW + PH + 1, two roundings of slack for
      the second-order terms.  RoIPool's bin maxima are exact (gather + compare), so that is the whole bar; RoIAlign's bins
      are held to the project's 1e-5 per bin (tests/test_hip_ops.py), so the mean of them gets the sum bar + 1e-5.
  box decode     1e-3 absolute (boxes), 1e-6 (fg), 2e-4 absolute (loc2bbox), 2e-6 relative (bbox2loc): the bars of
                 test_rpn_decode, test_utils_loc2bbox_* and test_utils_bbox2loc_surface, unchanged.
  everything else (anchors, keys, gathers, sort order, NMS keep lists, RoIPool maxima, record classes and scores) is exact.
"""
import torch

import oracle
from oracle import targets as oracle_targets
from oracle.box import _lib as oracle_lib

U = 2.0 ** -24
BIN_BAR = 1e-5                      # RoIAlign bin values against oracle.roi_align (tests/test_hip_ops.py)
BORDER_TOL = 1e-3                   # a min-size decision may differ only where the reference's shorter side is this close
BORDER_CAP = 1e-4                   # ... and at most this fraction of the boxes may be that close
NEG_INF = float("-inf")


def rand_boxes(g, n, span=800.0, wh=300.0):
    """[n,4] xyxy boxes: corners uniform in [0, span), sides uniform in [1, wh + 1)."""
    xy = torch.rand(n, 2, generator=g) * span
    return torch.cat([xy, xy + torch.rand(n, 2, generator=g) * wh + 1.0], dim=1)


# ----------------------------------------------------------------------------- box decode (rpn_decode.hip)
def decode_clamp(anchor, loc, clamp_x, clamp_y):
    """nets/rpn.py:47-51: loc2bbox, then x into [0, clamp_x] and y into [0, clamp_y]."""
    roi = oracle.loc2bbox(anchor, loc)
    roi[:, 0::2] = roi[:, 0::2].clamp(0, clamp_x)
    roi[:, 1::2] = roi[:, 1::2].clamp(0, clamp_y)
    return roi


def min_size_mask(roi, min_size):
    """nets/rpn.py:52-54 -> (keep mask, shorter side)."""
    w, h = roi[:, 2] - roi[:, 0], roi[:, 3] - roi[:, 1]
    return (w >= min_size) & (h >= min_size), torch.minimum(w, h)


def border_boxes(side, min_size):
    """The boxes whose min-size decision f32 noise may flip: the reference's shorter side within BORDER_TOL of min_size."""
    return (side - min_size).abs() < BORDER_TOL


def rpn_decode_ref(locs, scores, base, B, Hf, Wf, stride, clamp_x, clamp_y, min_size):
    """locs [B*Hf*Wf, 4A], scores [B*Hf*Wf, 2A] -> anchors [n,4], boxes [B,n,4], fg [B,n], keep [B,n] bool, side [B,n]."""
    anchor = oracle.enumerate_shifted_anchor(base, stride, Hf, Wf)
    fg = torch.softmax(scores.reshape(B, -1, 2), dim=-1)[:, :, 1]
    boxes = torch.stack([decode_clamp(anchor, l, clamp_x, clamp_y) for l in locs.reshape(B, -1, 4)])
    keep, side = zip(*(min_size_mask(b, min_size) for b in boxes))
    return anchor, boxes, fg, torch.stack(keep), torch.stack(side)


def big_rpn_case():
    """The grid-stride case of rpn_decode and proposal_decode: B = 2 maps of 243 x 243 at stride 16 with the 9 base anchors,
    1 062 882 boxes (> 4096 * 256), seed 12, locs = randn * 0.4.  -> dict of inputs and of the reference's results."""
    g = torch.Generator().manual_seed(12)
    base = oracle.generate_basic_anchor()
    A, B, Hf, Wf, stride = base.shape[0], 2, 243, 243, 16
    locs = torch.randn(B * Hf * Wf, 4 * A, generator=g) * 0.4
    scores = torch.randn(B * Hf * Wf, 2 * A, generator=g) * 2
    H, W = Hf * stride, Wf * stride
    anchor, boxes, fg, keep, side = rpn_decode_ref(locs, scores, base, B, Hf, Wf, stride, H, W, 16.0)
    return dict(base=base, A=A, B=B, Hf=Hf, Wf=Wf, stride=stride, clamp_x=H, clamp_y=W, min_size=16.0, locs=locs,
                scores=scores, anchor=anchor, boxes=boxes, fg=fg, keep=keep, side=side, n=B * Hf * Wf * A)


def detection_keys_ref(det, thr, background_class):
    """[n,6] records -> sort keys: the score where it passes the threshold and is not the background class, -inf otherwise
    (a NaN score fails the comparison and is dropped)."""
    s, c = det[:, 4], det[:, 5]
    ok = (s >= thr) & ((c != float(background_class)) if background_class >= 0 else torch.ones_like(s, dtype=torch.bool))
    return torch.where(ok, s, torch.full_like(s, NEG_INF))


def gather_rows_ref(src, idx):
    """src [B,n,C], idx [B,m] -> [B,m,C]: src[b, idx[b,r]], zero rows where the index is negative or >= n."""
    n, C = src.shape[1], src.shape[2]
    ok = (idx >= 0) & (idx < n)
    rows = torch.gather(src, 1, idx.clamp(0, n - 1).long().unsqueeze(-1).expand(-1, -1, C))
    return torch.where(ok.unsqueeze(-1), rows, torch.zeros_like(rows))


def bbox2loc_ref(src, dst):
    return oracle_targets.bbox2loc(src, dst)


# ----------------------------------------------------------------------------- top-k (sort_topk.hip)
def topk_keys(B, n, seed=13):
    """The keys of test_sort_topk_exact: rounded to 1/4096 (many exact ties), 30 % filtered (-inf), and with B > 1 the first
    half of row 0 one tie group."""
    g = torch.Generator().manual_seed(seed)
    keys = (torch.rand(B, n, generator=g) * 4096).round() / 4096
    keys[torch.rand(B, n, generator=g) < 0.3] = NEG_INF
    if B > 1:
        keys[0, : n // 2] = 1.0
    return keys, torch.randn(B, n, 4, generator=g)


def stable_topk_ref(keys_row, n_pre):
    """Source indices of the n_pre largest finite keys of one row, descending, equal keys in index order."""
    valid = torch.nonzero(torch.isfinite(keys_row)).squeeze(1)
    return valid[torch.sort(keys_row[valid], descending=True, stable=True).indices[:n_pre]]


# The launch rule of tsod_sort_topk_desc_ws_f32, restated (test_topk_path_restates_the_launch_rule holds it to the source).
TOPK_FULL_RANK_WORK = 3.0e8
TOPK_THREADS = 1024
TOPK_KPT = (10, 20, 40, 80)
TOPK_RANK_PARTS, TOPK_RANK_STRIP = 16, 512


def topk_path(B, n, n_pre):
    """('full',) | ('select', keys per thread) | ('stream',): which kernel orders [B,n] keys."""
    if float(B) * n * n <= TOPK_FULL_RANK_WORK:
        return ("full",)
    if n > TOPK_KPT[-1] * TOPK_THREADS:
        return ("stream",)
    return ("select", next(k for k in TOPK_KPT if n <= k * TOPK_THREADS))


def rank_strip(n_cand):
    """(64-blocks of candidates, passes one wave makes over its strip) in topk_rank_kernel."""
    blocks = (n_cand + 63) // 64
    per = (blocks + TOPK_RANK_PARTS - 1) // TOPK_RANK_PARTS * 64
    return blocks, (per + TOPK_RANK_STRIP - 1) // TOPK_RANK_STRIP


# ----------------------------------------------------------------------------- NMS (nms.hip)
def nms_keep_ref(boxes_sorted, n, thr):
    """Greedy NMS over the first n boxes (already in score order) -> every survivor, in order."""
    if n == 0:
        return torch.zeros(0, dtype=torch.int64)
    return oracle.nms(boxes_sorted[:n], torch.arange(n, 0, -1, dtype=torch.float32), thr)


def nms_pad_ref(boxes_sorted, n, thr, n_post):
    """oracle_nms_pad: (number kept, or -2 where the reference's pad 0,1,2,... indexes past n; keep list [n_post])."""
    out = torch.zeros(n_post, dtype=torch.int64)
    b = boxes_sorted[:max(n, 1)].contiguous()
    return int(oracle_lib().oracle_nms_pad(b.data_ptr(), n, thr, n_post, out.data_ptr())), out


def dense_boxes(g, n, span=60.0, wh=8.0, base=16.0):
    """rand_boxes with near-equal sides (base + [1, wh + 1)) on a small span, so that 0.7 really prunes a set of 200: about
    140 survive (at rand_boxes' default spacing and sizes 197 of 200 do, and NMS has nothing to decide)."""
    b = rand_boxes(g, n, span=span, wh=wh)
    b[:, 2:] += base
    return b


def disjoint_boxes(n=200):
    """n boxes of side 10 on a grid of pitch 20, 16 to a row: no two overlap."""
    i = torch.arange(n)
    xy = torch.stack([(i % 16) * 20, (i // 16) * 20], dim=1).float()
    return torch.cat([xy, xy + 10.0], dim=1)


def chain_boxes(n=200, lead=0):
    """[i, 0, i + 8, 8]: IoU with the next box 7/9 > 0.7, with the one after 6/10 < 0.7, so at 0.7 every survivor suppresses
    exactly its successor.  ``lead`` far-away boxes are put in front: they shift the chain, and with it the parity of the
    survivors at every 64-block edge (n boxes in all)."""
    i = torch.arange(n - lead).float()
    z = torch.zeros_like(i)
    chain = torch.stack([i, z, i + 8, z + 8], dim=1)
    far = torch.stack([torch.tensor([1000.0 + 20 * k, 1000.0, 1008.0 + 20 * k, 1008.0]) for k in range(lead)]) if lead else chain[:0]
    return torch.cat([far, chain])


def overlapping_records(seed, B=2, R=300, n_class=21, span=300.0):
    """Detection records [B,R,6] with heavy overlap and scores rounded to 1/8 (exact ties: the stable rule matters)."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(B, R, 2, generator=g) * span
    score = (torch.randn(B, R, 1, generator=g) * 8).round() / 8
    return torch.cat([xy, xy + torch.rand(B, R, 2, generator=g) * 200 + 5, score,
                      torch.randint(0, n_class, (B, R, 1), generator=g).float()], dim=-1)


# ----------------------------------------------------------------------------- RoI head (roi_pool.hip)
def SUM_ROUNDINGS(PH, PW):
    """Roundings counted for one mean over PH x PW bins (module docstring)."""
    return PW + PH + 1


def sum_bar(bins, PH, PW):
    """bins [K,C,PH,PW] (the exact f32 bin values) -> per-output bar [K,C] of the f32 mean over the bins."""
    return SUM_ROUNDINGS(PH, PW) * U * bins.double().abs().sum(dim=(2, 3)) / (PH * PW)


def mean_and_bar(bins, extra=0.0):
    """bins [K,C,PH,PW] f32 -> (f64 mean over the bins [K,C], its bar [K,C])."""
    PH, PW = bins.shape[2:]
    return bins.double().mean(dim=(2, 3)), sum_bar(bins, PH, PW) + extra


def roi_to_map(rois, img_h, img_w, Hf, Wf):
    """nets/classify.py:35-36 in f32, op for op: divide by the image side, then multiply by the map side.  rois [...,4]."""
    r = rois.float()
    sx, sy = torch.tensor(float(img_w)), torch.tensor(float(img_h))
    out = torch.empty_like(r)
    out[..., 0::2] = r[..., 0::2] / sx * float(Wf)
    out[..., 1::2] = r[..., 1::2] / sy * float(Hf)
    return out


def map_to_image(fm, img_h, img_w, Hf, Wf):
    """Image coordinates that roi_to_map sends back to ``fm``: exactly where some f32 within 8 ulp of fm * side / map does
    (searched), else the nearest.  Not every value is reachable through the two roundings (no y gives 3.5 on a 13-row map),
    which is why geometry_rois chooses its .5 coordinates and the tests their image sides.  [...,4] -> [...,4]."""
    fm = fm.float()
    out = torch.empty_like(fm)
    for sl, side, cells in ((slice(0, None, 2), img_w, Wf), (slice(1, None, 2), img_h, Hf)):
        want = fm[..., sl].contiguous()
        x0 = (want * float(side) / float(cells)).contiguous()
        best = x0.clone()
        err = (x0 / torch.tensor(float(side)) * float(cells) - want).abs()
        for d in range(-8, 9):
            cand = (x0.view(torch.int32) + d).view(torch.float32)
            e = (cand / torch.tensor(float(side)) * float(cells) - want).abs()
            better = torch.isfinite(cand) & (e < err)
            best, err = torch.where(better, cand, best), torch.where(better, e, err)
        out[..., sl] = best
    return out


def geometry_rois(g, Hf, Wf, n_random=8):
    """[K,4] RoIs in feature-map coordinates: random ones, then the shapes at which a RoI kernel goes wrong (named in
    GEOMETRY_NAMES, in this order after the random ones)."""
    H, W = float(Hf), float(Wf)
    rnd = rand_boxes(g, n_random, span=W, wh=W * 0.5) - 2.0
    named = torch.tensor([
        [3, 2, 3, 2],                      # one pixel wide and tall
        [3, 0, 3, H - 1],                  # one pixel wide
        [0, 2, W - 1, 2],                  # one pixel tall
        [2, 1, 4, H - 2],                  # narrower than PW: several bins share a column
        [1, 1, 2, 2],                      # narrower and shorter than the bins
        [5, 1, 2, 4],                      # x2 < x1
        [1, 4, 4, 2],                      # y2 < y1
        [0, 0, W - 1, H - 1],              # the whole map
        [-4, 1, 2, 4],                     # hanging off the left
        [W - 3, 1, W + 4, 4],              # ... the right
        [1, -5, 4, 2],                     # ... the top
        [1, H - 2, 4, H + 6],              # ... the bottom
        [-3, -3, W + 2, H + 2],            # ... all four
        [-30, -30, -20, -20],              # entirely outside (before)
        [W + 5, H + 5, W + 9, H + 9],      # entirely outside (after)
        [0.5, 1.5, 3.5, 4.5],              # .5 coordinates: round half away from zero
        [2.5, 0.5, 4.5, 2.5],
        [-0.5, -1.5, 2.5, 4.5],            # ... on the negative side
    ], dtype=torch.float32)
    return torch.cat([rnd, named])


GEOMETRY_NAMED = 18
HALF_ROWS = (-3, -2, -1)                   # the .5 RoIs of geometry_rois


def marked_map(g, B, C, Hf, Wf):
    """[B,C,Hf,Wf] randn with one column of every map row raised to a large value unique to that row (50 + row, the same in
    every channel): a bin maximum taken over a wrong column moves the mean by >= 1 / (PH PW), far beyond a rounding bar."""
    feat = torch.randn(B, C, Hf, Wf, generator=g)
    for b in range(B):
        for h in range(Hf):
            feat[b, :, h, (5 * h + 3 * b) % Wf] = 50.0 + h
    return feat


def rois5_of(rois_fm, roi_indices, R):
    """[B*R,4] map-coordinate RoIs + the image index of every group of R -> [B*R,5] rows (index, x1, y1, x2, y2)."""
    idx = roi_indices.float().repeat_interleave(R).view(-1, 1)
    return torch.cat([idx, rois_fm.reshape(-1, 4)], dim=1)


def roi_pool_avg_ref(feat_nchw, rois5, PH, PW):
    """-> (f64 mean of the reference's f32 bin maxima [K,C], bar [K,C])."""
    return mean_and_bar(oracle.roi_pool(feat_nchw, rois5, (PH, PW), 1.0))


def roi_align_avg_ref(feat_nchw, rois5, PH, PW, sampling_ratio, aligned):
    """-> (f64 mean of the reference's f32 bins [K,C], bar [K,C] = the sum bar + the per-bin bar)."""
    return mean_and_bar(oracle.roi_align(feat_nchw, rois5, (PH, PW), 1.0, sampling_ratio, aligned), BIN_BAR)
