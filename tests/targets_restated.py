"""Plain CPU restatement of csrc/targets.hip (AnchorTargetCreator, ProposalTargetCreator, bbox2loc) that exposes every
stage, and the case list of the switch-level sweep (tests/test_targets_restated.py on the CPU,
tests/test_target_kernels_gpu.py on the device).  Nothing here imports the package under test.

The arithmetic is torch f32 on oracle.box.bbox_iou: every decision below depends on the reference's own f32 rounding of
the IoU, so a higher-precision IoU would be another function, not a better reference.  oracle/targets.py returns final
results only and raises on quirk T2; ``anchor_stages`` / ``proposal_stages`` never raise and return what each stage
holds, which is what the kernels leave in memory.  ``mutant=`` selects one deliberately wrong variant (MUTANTS); the CPU
test file shows that each of them differs from the truth on some case of the sweep.

The launch geometry restated here (pinned to the source text by test_targets_restated.py):
  rowmax_kernel           256 candidates per block, ground-truth boxes through LDS 256 at a time
  colargmax_kernel        one block of 256 threads (4 waves of 64) per ground-truth box, thread t reads anchors t, t+256, ...
  anchor_label_kernel     one block of 1024 threads; thread t owns anchors [t*chunk, (t+1)*chunk), chunk = ceil(A / 1024)
  proposal_select_kernel  the same over the R + G candidates
  bbox2loc_kernel         at most 4096 blocks of 256 threads, grid-stride beyond

Cases sit on a small integer grid (sides 1..4), so every intersection, area and union is a small integer, the IoU is one
correctly rounded division of two of them, and exact ties and exact threshold hits are plentiful:
[0,0,1,1] against [0,0,2,1] is exactly 0.5, against [0,0,4,1] exactly 0.25.
"""
import functools

import torch

from oracle import targets as oracle_targets
from oracle.box import bbox_iou

THREADS = 1024            # anchor_label_kernel / proposal_select_kernel
WAVE = 64
ROW_BLOCK = 256           # rowmax_kernel: candidates per block and ground-truth boxes per LDS chunk
COL_THREADS = 256         # colargmax_kernel
B2L_BLOCKS, B2L_THREADS = 4096, 256

ANCHOR_THR = dict(pos_iou_thresh=0.5, neg_iou_thresh=0.25)
PROPOSAL_THR = (0.5, 0.5, 0.25)          # pos_iou_thresh, neg_iou_thresh_high, neg_iou_thresh_low
BOTH_THR = (0.25, 0.5, 0.25)             # neg_iou_thresh_high > pos_iou_thresh: IoU in [0.25, 0.5) is positive AND negative
LOC_REL_BAR = 2e-6                       # test_utils_bbox2loc_surface's bar (division and logf, a few ulp), denominator floored at 1

ANCHOR_MUTANTS = ("row_last", "row_chunk_last", "col_last", "first_claim", "cap_off_by_one", "pos_gt", "neg_le", "t1_lt2",
                  "prefix_reset")
PROPOSAL_MUTANTS = ("row_last", "row_chunk_last", "pos_gt", "neg_hi_le", "neg_lo_gt", "cap_off_by_one", "t2_slots",
                    "neg_unclipped", "prefix_reset")


def chunk_of(n_items):
    return (n_items + THREADS - 1) // THREADS


# ----------------------------------------------------------------------------- arg-max rules
def _arg(ious, dim, rule="first"):
    """Index of the maximum along ``dim`` by an explicit rule, not by what torch.max happens to return on ties."""
    m = ious.max(dim=dim, keepdim=True).values
    idx = torch.arange(ious.shape[dim]).view((-1, 1) if dim == 0 else (1, -1)).expand_as(ious)
    hit = ious == m
    if rule == "last":
        return torch.where(hit, idx, torch.full_like(idx, -1)).max(dim=dim).values
    if rule == "chunk_last":             # first within a chunk of 256, but a later chunk takes a tie
        last = torch.where(hit, idx, torch.full_like(idx, -1)).max(dim=dim, keepdim=True).values
        hit = hit & (idx // ROW_BLOCK == last // ROW_BLOCK)
    return torch.where(hit, idx, torch.full_like(idx, 1 << 40)).min(dim=dim).values


def _row_max(cand, bbox, mutant):
    ious = bbox_iou(cand, bbox)
    n = cand.shape[0]
    if bbox.shape[0] == 0:               # len(bbox) == 0: zeros
        return ious, torch.zeros(n), torch.zeros(n, dtype=torch.int64)
    rule = {"row_last": "last", "row_chunk_last": "chunk_last"}.get(mutant, "first")
    return ious, ious.max(dim=1).values, _arg(ious, 1, rule)


def _block_rank(is_pos):
    """MUTANT: the running count of positives starts again at every 1024th candidate."""
    rank = torch.zeros_like(is_pos, dtype=torch.int64)
    for s in range(0, is_pos.numel(), THREADS):
        seg = is_pos[s:s + THREADS].long()
        rank[s:s + THREADS] = torch.cumsum(seg, 0) - seg
    return rank


# ----------------------------------------------------------------------------- AnchorTargetCreator
def anchor_stages(bbox, anchor, n_sample=256, pos_ratio=0.5, pos_iou_thresh=0.7, neg_iou_thresh=0.3, mutant=None):
    """Every stage of AnchorTargetCreator(n_sample, pos_iou_thresh, neg_iou_thresh, pos_ratio)(bbox, anchor)."""
    assert mutant is None or mutant in ANCHOR_MUTANTS, mutant
    A, G = anchor.shape[0], bbox.shape[0]
    ious, max_iou, row = _row_max(anchor, bbox, mutant)
    gt_argmax = _arg(ious, 0, "last" if mutant == "col_last" else "first") if G else torch.zeros(0, dtype=torch.int64)
    row_after = row.clone()
    for i in (reversed(range(G)) if mutant == "first_claim" else range(G)):    # in gt order: the last claiming box wins
        row_after[gt_argmax[i]] = i
    label_thr = torch.full((A,), -1, dtype=torch.int64)
    label_thr[(max_iou <= neg_iou_thresh) if mutant == "neg_le" else (max_iou < neg_iou_thresh)] = 0
    label_thr[(max_iou > pos_iou_thresh) if mutant == "pos_gt" else (max_iou >= pos_iou_thresh)] = 1
    label_claim = label_thr.clone()
    label_claim[gt_argmax] = 1
    n_pos = int(pos_ratio * n_sample)
    pos = torch.where(label_claim == 1)[0]
    total_pos = pos.numel()
    label_cap = label_claim.clone()
    if total_pos > n_pos:
        if mutant == "prefix_reset":
            label_cap[pos[_block_rank(label_claim == 1)[pos] >= n_pos]] = -1
        else:
            label_cap[pos[n_pos + (1 if mutant == "cap_off_by_one" else 0):]] = -1
    pos_length = min(total_pos, n_pos)
    n_neg = n_sample - pos_length
    label = label_cap.clone()
    if (2 if mutant == "t1_lt2" else 1) > n_neg:                     # T1: all negatives at n_neg == 0; the reference's slice below 0
        label[torch.where(label_cap == 0)[0][n_neg:]] = -1
    flag = int((label > 0).any())
    loc = oracle_targets.bbox2loc(anchor, bbox[row_after]) if flag else torch.zeros_like(anchor)
    return dict(ious=ious, max_iou=max_iou, argmax_before=row, argmax=row_after, gt_argmax=gt_argmax, label_thr=label_thr,
                label_claim=label_claim, label_cap=label_cap, label=label, flag=flag, loc=loc, n_pos=n_pos, total_pos=total_pos,
                pos=pos, pos_length=pos_length, n_neg=n_neg)


# ----------------------------------------------------------------------------- ProposalTargetCreator
def proposal_stages(roi, bbox, label, n_sample=128, pos_ratio=0.5, pos_iou_thresh=0.5, neg_iou_thresh_high=0.5,
                    neg_iou_thresh_low=0.0, mutant=None):
    """Every stage of ProposalTargetCreator(...)(roi, bbox, label).  Never raises: ``status`` is 1 where the reference's
    ``gt_roi_label[neg_index] = 0`` raises IndexError, and ``label_after`` then holds the zeroes of the in-range positions."""
    assert mutant is None or mutant in PROPOSAL_MUTANTS, mutant
    G = bbox.shape[0]
    ppi = int(n_sample * pos_ratio)
    cand = torch.cat((roi, bbox), dim=0)
    ious, max_iou, assign = _row_max(cand, bbox, mutant)
    base_label = (label[assign] + 1) if G else torch.zeros(cand.shape[0], dtype=label.dtype)
    is_pos = (max_iou > pos_iou_thresh) if mutant == "pos_gt" else (max_iou >= pos_iou_thresh)
    is_neg = ((max_iou <= neg_iou_thresh_high) if mutant == "neg_hi_le" else (max_iou < neg_iou_thresh_high)) & \
             ((max_iou > neg_iou_thresh_low) if mutant == "neg_lo_gt" else (max_iou >= neg_iou_thresh_low))
    pos_all = torch.where(is_pos)[0]
    if mutant == "prefix_reset":
        pos_idx = pos_all[_block_rank(is_pos)[pos_all] < ppi]
    else:
        pos_idx = pos_all[:ppi + (1 if mutant == "cap_off_by_one" and pos_all.numel() > ppi else 0)]
    pos_len = pos_idx.numel()
    neg_all = torch.where(is_neg)[0]
    room = n_sample - pos_len
    neg_idx = neg_all[:room] if neg_all.numel() > room and mutant != "neg_unclipped" else neg_all
    neg_len = neg_idx.numel()
    keep = torch.cat((pos_idx, neg_idx))
    S = keep.numel()
    sample_roi = cand[keep]
    label_before = base_label[keep]
    label_after = label_before.clone()
    t2 = torch.zeros(0, dtype=torch.int64)
    status = 0
    if G:
        loc = oracle_targets.bbox2loc(sample_roi, bbox[assign[keep]])
        where = (pos_len + torch.arange(neg_len)) if mutant == "t2_slots" else neg_idx      # T2: ORIGINAL indices on the kept list
        t2 = where[where < S]
        label_after[t2] = 0
        status = int((where >= S).any())
    else:
        loc = torch.zeros_like(sample_roi)
    return dict(ious=ious, max_iou=max_iou, assign=assign, is_pos=is_pos, is_neg=is_neg, pos_all=pos_all, neg_all=neg_all,
                pos_idx=pos_idx, neg_idx=neg_idx, keep=keep, pos_len=pos_len, neg_len=neg_len, S=S, sample_roi=sample_roi, loc=loc,
                label_before=label_before, label_after=label_after, t2=t2, status=status, ppi=ppi, room=room, N=cand.shape[0])


# ----------------------------------------------------------------------------- case builders
def grid_boxes(g, n, span, max_side=4):
    """[n,4] xyxy boxes with integer corners in [0, span) and integer sides in 1..max_side."""
    xy = torch.randint(0, span, (n, 2), generator=g)
    wh = torch.randint(1, max_side + 1, (n, 2), generator=g)
    return torch.cat([xy, xy + wh], dim=1).float()


def _box(x, y, w, h):
    return torch.tensor([x, y, x + w, y + h], dtype=torch.float32)


class _Slots:
    """Hands out distinct indices of [0, n) in a seeded order, skipping the reserved ones."""

    def __init__(self, g, n, reserved=()):
        self.free = [i for i in torch.randperm(n, generator=g).tolist() if i not in set(reserved)]

    def take(self, k=1):
        if len(self.free) < k:
            return None
        out, self.free = self.free[:k], self.free[k:]
        return out


def pick_cut(pos, n_items, cut):
    """How many positives to keep so that the cap cuts where ``cut`` says.  pos: ascending indices of all positives."""
    chunk, total = chunk_of(n_items), pos.numel()
    if isinstance(cut, int):
        return cut
    if cut == "none":
        return total + 5
    if cut == "exact":
        return total
    if cut == "plus1":
        assert total >= 1
        return total - 1
    if cut == "zero":
        return 0
    thread = pos // chunk
    for j in sorted(range(1, total), key=lambda j: abs(j - total // 2)):        # the fitting cut nearest the middle
        kept, dropped = int(thread[j - 1]), int(thread[j])
        if {"inside": kept == dropped,
            "chunk_edge": kept != dropped and kept // WAVE == dropped // WAVE,
            "wave_edge": kept // WAVE != dropped // WAVE}[cut]:
            return j
    raise AssertionError(f"no '{cut}' cut among {total} positives of {n_items}")


# name: (A, G, seed, span, cut, t1)   t1: None (pos_ratio 0.5, n_sample = 2 n_pos), "fires" (n_neg == 0), "spared" (n_neg == 1)
ANCHOR_CASES = {
    "A1-G0": (1, 0, 1, 4, "none", None),
    "A1-G1": (1, 1, 2, 3, "exact", None),
    "A1-G2": (1, 2, 3, 3, "zero", None),
    "A63-G2": (63, 2, 4, 8, "exact", None),
    "A64-G1": (64, 1, 5, 6, "plus1", None),
    "A65-G255": (65, 255, 6, 20, "chunk_edge", None),
    "A255-G256": (255, 256, 7, 24, "exact", "fires"),
    "A256-G257": (256, 257, 8, 24, "wave_edge", None),
    "A257-G513": (257, 513, 9, 32, "exact", "spared"),
    "A1023-G2": (1023, 2, 10, 10, "chunk_edge", None),
    "A1024-G0": (1024, 0, 11, 16, "none", None),
    "A1024-G257": (1024, 257, 12, 28, "wave_edge", None),
    "A1025-G1": (1025, 1, 13, 8, "zero", None),
    "A1025-G2": (1025, 2, 14, 2, "inside", None),
    "A1025-G255": (1025, 255, 15, 28, "chunk_edge", None),
    "A1025-G257": (1025, 257, 16, 28, "inside", None),
    "A1025-G513": (1025, 513, 17, 36, "plus1", None),
    "A2049-G0": (2049, 0, 18, 16, "none", None),
    "A2049-G1": (2049, 1, 19, 8, "plus1", None),
    "A2049-G256": (2049, 256, 20, 30, "inside", None),
    "A2049-G257": (2049, 257, 21, 30, 40, "fires"),
    "A2049-G513": (2049, 513, 22, 40, "wave_edge", None),
    "A300-G1025": (300, 1025, 23, 40, "chunk_edge", None),
}


@functools.lru_cache(maxsize=None)
def anchor_case(name):
    """-> dict(bbox, anchor, kw): grid boxes with planted ties, exact threshold hits, a box that overlaps nothing and an anchor
    that three boxes claim, wherever A and G have room for them.  Planted boxes live at x >= 100, away from the random ones."""
    A, G, seed, span, cut, t1 = ANCHOR_CASES[name]
    g = torch.Generator().manual_seed(seed)
    anchor, bbox = grid_boxes(g, A, span), grid_boxes(g, G, span)
    sa = _Slots(g, A, reserved=(250, 256))
    sg = _Slots(g, G, reserved=(255, 256, 1024))
    planted = []
    if G >= 257 and (a := sa.take(1)):                               # a row maximum at g = 255 and again at g = 256
        anchor[a[0]] = bbox[255] = bbox[256] = _box(100, 40, 2, 3)
        planted.append("row_tie_255_256")
    if G >= 1025 and (a := sa.take(1)) and (q := sg.take(2)):        # three claims, the last from the override loop's second trip
        anchor[a[0]] = bbox[q[0]] = bbox[q[1]] = bbox[1024] = _box(100, 50, 3, 2)
        planted.append("claim_across_1024")
    if A >= 257 and (q := sg.take(1)):                               # column tie: the FIRST anchor sits in a higher lane
        anchor[250] = anchor[256] = bbox[q[0]] = _box(100, 60, 2, 2)
        planted.append("col_tie_250_256")
    if A >= 8 and G >= 2 and (q := sg.take(2)):                      # exact hits of both thresholds, each box claimed elsewhere
        p = sa.take(4)
        anchor[p[0]], anchor[p[1]], bbox[q[0]] = _box(100, 0, 1, 1), _box(100, 0, 2, 1), _box(100, 0, 2, 1)      # 0.5
        anchor[p[2]], anchor[p[3]], bbox[q[1]] = _box(100, 10, 1, 1), _box(100, 10, 4, 1), _box(100, 10, 4, 1)   # 0.25
        planted.append("threshold_hits")
    if A >= 8 and G >= 3 and (q := sg.take(1)):                      # overlaps no anchor: ties at 0.0 everywhere -> anchor 0
        bbox[q[0]] = _box(100, 20, 1, 1)
        planted.append("lonely_gt")
    if A >= 8 and G >= 8 and (q := sg.take(3)) and (a := sa.take(1)):
        anchor[a[0]] = _box(100, 30, 3, 3)
        for i in q:
            bbox[i] = _box(100, 30, 3, 3)
        planted.append("triple_claim")
    free = anchor_stages(bbox, anchor, n_sample=1 << 30, pos_ratio=0.5, **ANCHOR_THR)
    n_pos = pick_cut(free["pos"], A, cut)
    if t1 == "fires":                                                # pos_length == n_sample: n_neg == 0
        n_pos = min(n_pos, free["total_pos"])
        kw = dict(n_sample=n_pos, pos_ratio=1.0)
    elif t1 == "spared":                                             # pos_length == n_sample - 1: n_neg == 1
        assert n_pos == free["total_pos"]
        kw = dict(n_sample=n_pos + 1, pos_ratio=1.0)
    else:
        kw = dict(n_sample=2 * n_pos, pos_ratio=0.5) if n_pos else dict(n_sample=64, pos_ratio=0.0)
    assert int(kw["pos_ratio"] * kw["n_sample"]) == (n_pos if t1 != "spared" else n_pos + 1)
    return dict(name=name, bbox=bbox, anchor=anchor, kw=dict(kw, **ANCHOR_THR), planted=tuple(planted))


# name: (R, G, seed, kind, span, thresholds, cut, pos_ratio, n_sample)
#   kind "random": grid boxes.  "dense": every proposal shares a ground-truth box's corner and height, so its IoU is >= 0.25
#   and it is positive or negative.  "front": the only negatives are the first 12 proposals, everything else is positive, so
#   T2 zeroes positives' slots and nothing raises whatever the cap.
#   n_sample None: derived from the cut (pos_ratio 0.5 -> 2 ppi, 1.0 -> ppi, 0.25 -> 4 ppi); else the cut is what it gives.
PROPOSAL_CASES = {
    "R1-G0": (1, 0, 31, "random", 4, (0.5, 0.5, 0.0), None, 0.5, 8),
    "R0-G1": (0, 1, 32, "random", 4, PROPOSAL_THR, None, 0.5, 8),
    "R255-G1": (255, 1, 33, "random", 3, PROPOSAL_THR, "chunk_edge", 0.5, None),
    "R256-G0": (256, 0, 34, "random", 8, (0.5, 0.5, 0.0), None, 0.25, 96),
    "R256-G0-lo": (256, 0, 35, "random", 8, PROPOSAL_THR, None, 0.25, 96),
    "R0-G256": (0, 256, 36, "random", 24, PROPOSAL_THR, None, 0.5, 64),
    "R255-G2": (255, 2, 37, "dense", 8, PROPOSAL_THR, None, 1.0, 512),
    "R1-G256": (1, 256, 38, "random", 24, PROPOSAL_THR, None, 1.0, 300),
    "R0-G257": (0, 257, 39, "random", 24, PROPOSAL_THR, "exact", 1.0, None),
    "R767-G257": (767, 257, 40, "random", 30, PROPOSAL_THR, "wave_edge", 0.5, None),
    "R767-G257-dense": (767, 257, 41, "dense", 30, PROPOSAL_THR, None, 1.0, 2048),
    "R1024-G0": (1024, 0, 42, "random", 16, (0.5, 0.5, 0.0), None, 0.5, 2000),
    "R1023-G2": (1023, 2, 43, "front", 8, PROPOSAL_THR, "inside", 0.5, None),
    "R1023-G2-random": (1023, 2, 53, "random", 2, PROPOSAL_THR, "inside", 0.25, None),
    "R512-G513": (512, 513, 44, "random", 36, PROPOSAL_THR, "plus1", 0.5, None),
    "R512-G513-both": (512, 513, 45, "dense", 36, BOTH_THR, "inside", 0.5, None),
    "R2048-G1": (2048, 1, 46, "dense", 8, PROPOSAL_THR, None, 1.0, 4096),
    "R2048-G1-both": (2048, 1, 47, "dense", 8, BOTH_THR, None, 1.0, 4200),
    "R1536-G513": (1536, 513, 48, "front", 40, PROPOSAL_THR, "inside", 0.5, None),
    "R1536-G513-edge": (1536, 513, 49, "front", 40, PROPOSAL_THR, "wave_edge", 0.25, None),
    "R1792-G257": (1792, 257, 50, "random", 40, PROPOSAL_THR, "zero", 0.0, 128),
    "R1792-G257-full": (1792, 257, 51, "random", 40, PROPOSAL_THR, "chunk_edge", 1.0, None),
    "R1792-G257-dense": (1792, 257, 52, "dense", 40, PROPOSAL_THR, None, 0.5, 3000),
}


@functools.lru_cache(maxsize=None)
def proposal_case(name):
    """-> dict(roi, bbox, label, kw)."""
    R, G, seed, kind, span, thr, cut, pos_ratio, n_sample = PROPOSAL_CASES[name]
    g = torch.Generator().manual_seed(seed)
    bbox = grid_boxes(g, G, span)
    label = torch.randint(0, 20, (G,), generator=g)
    if kind == "random" or G == 0:
        roi = grid_boxes(g, R, span)
    else:
        src = bbox[torch.randint(0, G, (R,), generator=g)]
        roi = src.clone()
        if kind == "dense":                                          # same corner and height, any width 1..4: IoU >= 1/4
            roi[:, 2] = roi[:, 0] + torch.randint(1, 5, (R,), generator=g).float()
        else:                                                        # "front": copies (IoU 1), but the first 12 at IoU 1/4 .. < 1/2
            w = src[:12, 2] - src[:12, 0]
            roi[:12, 2] = src[:12, 0] + torch.where(w >= 3, torch.ones_like(w), 4 * w)       # 1/w or 1/4
    if R >= 4 and G >= 4 and kind == "random":                       # exact hits of the thresholds, away from everything else
        p = _Slots(g, R).take(2)
        q = _Slots(g, G).take(2)
        roi[p[0]], bbox[q[0]] = _box(100, 0, 1, 1), _box(100, 0, 2, 1)
        roi[p[1]], bbox[q[1]] = _box(100, 10, 1, 1), _box(100, 10, 4, 1)
    kw = dict(pos_iou_thresh=thr[0], neg_iou_thresh_high=thr[1], neg_iou_thresh_low=thr[2], pos_ratio=pos_ratio)
    if n_sample is None:
        free = proposal_stages(roi, bbox, label, n_sample=1 << 30, **kw)
        ppi = pick_cut(free["pos_all"], R + G, cut)
        n_sample = {0.5: 2 * ppi, 1.0: ppi, 0.25: 4 * ppi}[pos_ratio]
        assert int(n_sample * pos_ratio) == ppi and n_sample > 0
    return dict(name=name, roi=roi, bbox=bbox, label=label, kw=dict(kw, n_sample=n_sample))


@functools.lru_cache(maxsize=None)
def anchor_want(name, mutant=None):
    c = anchor_case(name)
    return anchor_stages(c["bbox"], c["anchor"], mutant=mutant, **c["kw"])


@functools.lru_cache(maxsize=None)
def proposal_want(name, mutant=None):
    c = proposal_case(name)
    return proposal_stages(c["roi"], c["bbox"], c["label"], mutant=mutant, **c["kw"])


def bbox2loc_boxes(n, seed=60):
    """Two sets of n boxes with non-integer sides >= 0.5 (finite offsets everywhere), two sources of zero width / height."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=g) * 700
    src = torch.cat([xy, xy + torch.rand(n, 2, generator=g) * 300 + 0.5], dim=1)
    xy2 = torch.rand(n, 2, generator=g) * 700
    dst = torch.cat([xy2, xy2 + torch.rand(n, 2, generator=g) * 300 + 0.5], dim=1)
    src[n // 2, 2] = src[n // 2, 0]                                  # floored at f32 eps
    src[n - 1, 3] = src[n - 1, 1]
    return src, dst


def loc_error(got, ref):
    """-> (finiteness pattern equal, largest |got - ref| / max(|ref|, 1) over the finite entries)."""
    fin = torch.isfinite(ref)
    same = torch.equal(torch.isfinite(got), fin)
    rel = ((got - ref).abs() / ref.abs().clamp_min(1.0))[fin]
    return same, (rel.max().item() if rel.numel() else 0.0)
