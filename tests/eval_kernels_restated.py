"""Designed cases for the kernels of csrc/eval_metrics.hip (DESIGN.md sections 4.14 and 4.25), CPU only.

The evaluator tests run whole evaluators over random data sets; which kernel paths those reach is chance.  The tables here
name the sizes at which the kernels change behaviour (the AP scan's 4096-position chunks, the offsets scan's 256-image trips,
the radix pass count, the match kernels' 64-lane trips) and the builders make small inputs that sit on each of them.
tests/test_eval_kernels_gpu.py checks the tables against the source text, checks that every case is what its name says, and
runs the kernels on them against the restatements of tests/coco_eval_restated.py and tests/test_detection_eval.py.

An accumulate case is a dict of record columns (score, cls, rank, tp [N,4], ig [N,4]) of `capacity` rows, `n_records`, npig
[C,A], T, caps and max_dets.  A match case is a dict of the metric's settings and `updates`; an update carries the images the
metric sees (for the restatement) and the padded arrays the kernel gets (padding filled with valid-looking rows).
"""
import numpy as np

import coco_eval_restated as CR

# ------------------------------------------------------------------------------------------- the kernels' constants, restated
THREADS = 256                      # kThreads
AP_ITEMS = 16                      # kApItems
AP_CHUNK = THREADS * AP_ITEMS      # positions per trip of the AP scans
RADIX_ITEMS = 16                   # kRadixItems
RADIX_TILE = THREADS * RADIX_ITEMS
MAX_R, MAX_G, MAX_T = 8192, 1024, 32
MAX_CLASSES = 1 << 18
WAVE = 64
PLAIN_INTS, COCO_INTS = 3, 11
SENTINEL = -1234567                # what record rows hold before a kernel writes them


def np_of(R):
    """NP of the match launchers: the bitonic sort's size."""
    n = 64
    while n < R:
        n <<= 1
    return n


def cap_chunk(R):
    """Positions per thread in the cap scan of sort_and_cap_detections."""
    return (np_of(R) + THREADS - 1) // THREADS


def class_bits(C):
    bits = 1
    while bits < 31 and (1 << bits) < C:
        bits += 1
    return bits


def radix_passes(C):
    return (32 + class_bits(C) + 7) // 8


def desc_score_bits(s):
    """The accumulate's sort key of a score: ascending u32 = descending score, -0 == +0."""
    u = np.asarray(s, np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    asc = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return (~asc & 0xFFFFFFFF).astype(np.uint64)


# ------------------------------------------------------------------------------------------------------------ the tables
SEGMENT_LENGTHS = (1, 15, 16, 17, 4095, 4096, 4097, 8192, 12293)
TP_PATTERNS = ("all", "none", "at4095", "at4096", "alternating", "random")
CLASS_COUNTS = (1, 2, 3, 256, 257, 65536, 65537, 262144)
SORT_WIDTHS = ((0, 33), (0, 41), (0, 49))
SORT_SIZES = (4095, 4096, 4097)
OFFSET_BATCHES = (257, 600)
CLASSES_PER_IMAGE = (1, 4, 5, 9, 130)
DETS_VS_CAP = ((63, 64), (64, 64), (64, 100), (65, 64), (129, 64), (130, 128), (200, 65), (5, 1), (10, 20))
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
GT_COUNTS = (0, 1, 63, 64, 65, 130)
BEFORE, AFTER = 37, 300            # records of the classes around the class under test


# ------------------------------------------------------------------------------------------------------ accumulate cases
def _assemble(parts, C, npig, T, caps, max_dets, rng, name):
    """parts: per class columns in sorted order (ties in record order).  Records are dealt to random rows; rows of equal
    (class, score) keep their order, so every part stays the stable sort of its rows."""
    cols = {k: np.concatenate([p[k] for p in parts]) for k in ("score", "cls", "rank", "tp", "ig")}
    N = len(cols["score"])
    key = (cols["cls"].astype(np.uint64) << np.uint64(32)) | desc_score_bits(cols["score"])
    assert (key[1:] >= key[:-1]).all(), "parts come in class order, each sorted by descending score"
    slots = rng.permutation(N)
    slots = slots[np.lexsort((slots, key))]
    out = {k: np.empty_like(v) for k, v in cols.items()}
    for k, v in cols.items():
        out[k][slots] = v
    out.update(name=name, C=C, npig=np.asarray(npig, np.int64), T=T, caps=tuple(caps), max_dets=max_dets, n_records=N)
    return out


def _part(cls, score, tp, rank=None, ig=None):
    n = len(score)
    tp = np.asarray(tp, np.uint32)
    tp4 = np.zeros((n, 4), np.uint32)
    tp4[:, :tp.shape[1] if tp.ndim == 2 else 1] = tp.reshape(n, -1)
    ig4 = np.zeros((n, 4), np.uint32)
    if ig is not None:
        ig = np.asarray(ig, np.uint32).reshape(n, -1)
        ig4[:, :ig.shape[1]] = ig
    return dict(score=np.asarray(score, np.float32), cls=np.full(n, cls, np.int32),
                rank=np.zeros(n, np.int32) if rank is None else np.asarray(rank, np.int32), tp=tp4, ig=ig4)


def _random_part(cls, n, rng, words=1, bits=1):
    score = np.sort((np.round(rng.random(n) * 50) / 50).astype(np.float32))[::-1]          # quantised: ties
    tp = rng.integers(0, 1 << bits, (n, words), dtype=np.uint64).astype(np.uint32)
    return _part(cls, score, tp, rank=rng.integers(0, 100, n))


def descending_scores(L):
    """L distinct f32 scores, strictly descending (j / 16384 is exact)."""
    return (1.0 - np.arange(L) / 16384.0).astype(np.float32)


def tp_pattern(pattern, L, rng):
    j = np.arange(L)
    return {"all": np.ones(L, bool), "none": np.zeros(L, bool), "at4095": j == 4095, "at4096": j == 4096,
            "alternating": j % 2 == 0, "random": rng.random(L) < .3}[pattern].astype(np.uint32)


def segment_case(L, pattern, coco):
    """Class 1, L records with distinct scores and the TP pattern along its sorted order, between a 37-record and a
    300-record class.  coco: range 1 ignores half the records at random and caps (10, 100) cut by a random rank."""
    rng = np.random.default_rng(1000 * L + TP_PATTERNS.index(pattern))
    tp = tp_pattern(pattern, L, rng)
    A = 2 if coco else 1
    mid = _part(1, descending_scores(L), np.stack([tp] * A, 1), rank=rng.integers(0, 100, L) if coco else None,
                ig=np.stack([np.zeros(L, np.uint32), (rng.random(L) < .5).astype(np.uint32)], 1) if coco else None)
    parts = [_random_part(0, BEFORE, rng, A), mid, _random_part(2, AFTER, rng, A)]
    case = _assemble(parts, 3, np.zeros((3, A), np.int64), 1, (10, 100) if coco else (1,), 100 if coco else 1, rng,
                     f"L{L}-{pattern}")
    case["n_tp"] = int(tp.sum())
    return case


def npig_values(n_tp):
    """0, 1, the TP count and three times it, without a value below the TP count but 0."""
    return sorted({0, n_tp, 3 * n_tp} | ({1} if n_tp <= 1 else set()))


def with_npig(case, value):
    out = dict(case)
    npig = np.zeros_like(case["npig"])
    npig[0], npig[1], npig[2] = BEFORE + 3, value, AFTER + 30
    out["npig"] = npig
    return out


def sparse_case(kind):
    """COCO kernel only, 12293 records (four chunks) of class 1 with alternating TP:
    dead_middle   range 0 ignores every record of the middle chunk;
    carry_n_apart the cap admits 10 records of the first two chunks, so the live count trails the position by 8182."""
    L = 12293
    rng = np.random.default_rng(77)
    j = np.arange(L)
    tp = (j % 2 == 0).astype(np.uint32)
    ig, rank = np.zeros(L, np.uint32), rng.integers(0, 50, L)
    if kind == "dead_middle":
        ig[AP_CHUNK:2 * AP_CHUNK] = 1
    else:
        rank[10:2 * AP_CHUNK] = 60
    parts = [_random_part(0, BEFORE, rng), _part(1, descending_scores(L), tp, rank=rank, ig=ig), _random_part(2, AFTER, rng)]
    live = (rank < 50) & (ig == 0)
    case = _assemble(parts, 3, [[BEFORE + 3], [int((tp & live).sum())], [AFTER + 30]], 1, (50,), 100, rng, kind)
    case["live_sorted"] = live
    return case


def odd_scores_case():
    """8200 records of class 1: +inf, a run of equal scores with different TP bits across sorted positions 4095 / 4096, a
    denormal, +0.0 and -0.0 mixed (one key), negative scores."""
    rng = np.random.default_rng(5)
    head = descending_scores(4090 - 3) * np.float32(.5) + np.float32(.5)                  # (0.5, 1.0]
    run = np.full(12, .25, np.float32)
    tail_n = 8200 - 3 - len(head) - 12 - 1 - 4
    below = (np.float32(.2) - np.arange(2000) / 65536.0).astype(np.float32)
    negative = (-.5 - np.arange(tail_n - 2000) / 16384.0).astype(np.float32)
    score = np.concatenate([np.full(3, np.inf, np.float32), head, run, below, np.float32([1e-40]),
                            np.float32([0.0, -0.0, 0.0, -0.0]), negative])
    tp = np.zeros(len(score), np.uint32)              # few TP: each one's position shows in the envelope
    tp[4090:4102] = [1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0]                                   # position 4095: 0, 4096: 1
    zero_at = len(score) - len(negative) - 4
    tp[zero_at:zero_at + 4] = [1, 0, 0, 1]
    tp[-1] = 1                                                                             # and the most negative score
    parts = [_random_part(0, BEFORE, rng), _part(1, score, tp), _random_part(2, AFTER, rng)]
    case = _assemble(parts, 3, [[BEFORE + 3], [int(tp.sum())], [AFTER + 30]], 1, (1,), 1, rng, "odd_scores")
    case["zero_at"] = zero_at
    return case


def pass_case(C):
    """Records in class 0, in the top class and in one between (where there are that many classes); T = 1."""
    rng = np.random.default_rng(C)
    classes = sorted({0, C // 2, C - 1})
    parts = [_random_part(c, 4500 // len(classes) + 100 * i, rng) for i, c in enumerate(classes)]    # two radix tiles
    npig = np.zeros((C, 1), np.int64)
    for p, c in zip(parts, classes):
        npig[c] = int(p["tp"][:, 0].sum()) + 2
    if C > 3:
        npig[1] = 5                                                                        # ground truth and no record
    case = _assemble(parts, C, npig, 1, (100,), 100, rng, f"C{C}")
    case["classes"] = classes
    return case


def live_count_cases():
    """(name, case, the case whose answer it must give).  The dead tail holds true positives of class 1 with the best score."""
    base = segment_case(4097, "random", True)
    base = with_npig(base, 3 * base["n_tp"])
    N = base["n_records"]
    tail = 500
    padded = dict(base)
    for k, fill in (("score", 2.0), ("cls", 1), ("rank", 0)):
        padded[k] = np.concatenate([base[k], np.full(tail, fill, base[k].dtype)])
    padded["tp"] = np.concatenate([base["tp"], np.ones((tail, 4), np.uint32)])
    padded["ig"] = np.concatenate([base["ig"], np.zeros((tail, 4), np.uint32)])
    padded["name"] = "dead_tail"
    empty = dict(padded, n_records=0, name="no_records")
    over = dict(base, n_records=N + 1000, name="count_above_capacity")
    return [(padded, base), (empty, empty), (over, base)]


def cell_case():
    """T = 32, A = 4, M = 4: a random mask word per range, ranks over the four caps, 5000 records in class 1."""
    rng = np.random.default_rng(9)
    caps = (1, 3, 10, 100)
    parts = []
    for c, n in ((0, BEFORE), (1, 5000), (2, AFTER)):
        p = _random_part(c, n, rng, words=4, bits=32)
        p["ig"] = (rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64) & rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64)
                   ).astype(np.uint32)                                                     # a quarter of the bits
        p["rank"] = rng.choice([0, 1, 2, 5, 9, 50, 99], n).astype(np.int32)
        parts.append(p)
    npig = np.zeros((3, 4), np.int64)
    for c, p in enumerate(parts):
        for a in range(4):
            hits = (p["tp"][:, a] & ~p["ig"][:, a])[:, None] >> np.arange(32, dtype=np.uint32)[None, :] & np.uint32(1)
            npig[c, a] = int(hits.sum(0).max()) + a
    return _assemble(parts, 3, npig, 32, caps, 100, rng, "cells")


def plain_rows(case):
    return np.stack([case["score"].view(np.int32), case["cls"], case["tp"][:, 0].view(np.int32)], 1).astype(np.int32)


def coco_rows(case):
    return np.concatenate([case["score"].view(np.int32)[:, None], case["cls"][:, None], case["rank"][:, None],
                           case["tp"].view(np.int32), case["ig"].view(np.int32)], 1).astype(np.int32)


def sorted_segment(case, c):
    """Record rows of class c in the accumulate's order (live records only)."""
    n = min(case["n_records"], len(case["score"]))
    idx = np.nonzero(case["cls"][:n] == c)[0]
    return idx[np.argsort(-case["score"][idx], kind="stable")]


def want_accumulate(case, coco):
    """coco_eval_restated.accumulate over the live records, restricted to the classes with records or ground truth; every
    other class is (-1, -1, 0, 0, 0).  -> precision, recall, TP, FP, FN of [C,A,M,T] (plain: range 0, one cap over all)."""
    n = min(case["n_records"], len(case["score"]))
    cls = case["cls"][:n]
    npig = case["npig"] if coco else case["npig"][:, :1]
    C, A = npig.shape
    caps = case["caps"] if coco else (1,)
    rank = case["rank"][:n] if coco else np.zeros(n, np.int32)
    ig = case["ig"][:n] if coco else np.zeros((n, 4), np.uint32)
    present = np.union1d(np.unique(cls), np.nonzero(npig.any(1))[0]).astype(np.int64)
    local = np.searchsorted(present, cls).astype(np.int32)
    part = CR.accumulate(case["score"][:n], local, rank, case["tp"][:n], ig, npig[present], case["T"], list(caps))
    shape = (C, A, len(caps), case["T"])
    full = [np.full(shape, -1.0), np.full(shape, -1.0), np.zeros(shape, np.int64), np.zeros(shape, np.int64),
            np.zeros(shape, np.int64)]
    for dst, src in zip(full, part):
        dst[present] = src
    return full


# ------------------------------------------------------------------------------------------------------------ match cases
FILL_DET = np.float32([0, 0, 10, 10, .99, 0])           # padding rows look like good detections / ground truth of class 0
FILL_GT = np.float32([0, 0, 10, 10])


def boxes_of(rng, n, lo=4, hi=150, span=400):
    xy = rng.uniform(0, span, (n, 2)).astype(np.float32)
    return np.concatenate([xy, xy + rng.uniform(lo, hi, (n, 2)).astype(np.float32)], 1)


def make_image(rng, dets, gts, crowd_p=0.0, steps=20):
    """dets / gts: {class: count}.  Detections are jittered copies of their class's ground truth (random boxes without one),
    scores quantised to 1/steps, rows shuffled."""
    gl = np.concatenate([np.full(n, c, np.int64) for c, n in gts.items()] + [np.zeros(0, np.int64)])
    gl = gl[rng.permutation(len(gl))]
    gb = boxes_of(rng, len(gl))
    rows = []
    for c, n in dets.items():
        mine = np.nonzero(gl == c)[0]
        box = gb[rng.choice(mine, n)] + rng.normal(0, 4, (n, 4)).astype(np.float32) if len(mine) else boxes_of(rng, n)
        far = rng.random(n) < .3
        box[far] = boxes_of(rng, int(far.sum()))
        d = np.zeros((n, 6), np.float32)
        d[:, :4], d[:, 4], d[:, 5] = box, np.round(rng.random(n) * steps) / steps, c
        rows.append(d)
    d = np.concatenate(rows + [np.zeros((0, 6), np.float32)])
    d = d[rng.permutation(len(d))]
    crowd = (rng.random(len(gl)) < crowd_p).astype(np.uint8) if crowd_p else None
    return (d, gb, gl, crowd, None)


def pad_update(images, R=None, G=None):
    """The kernel's arrays for one update; rows past counts / gt_counts hold FILL_DET / FILL_GT of class 0."""
    B = len(images)
    R = R or max(1, max(len(im[0]) for im in images))
    G = max(1, max(len(im[2]) for im in images)) + 2 if G is None else G
    det = np.tile(FILL_DET, (B, R, 1))
    gb = np.tile(FILL_GT, (B, G, 1))
    gl = np.zeros((B, G), np.int64)
    crowd = np.zeros((B, G), np.uint8)
    area = np.full((B, G), 100, np.float32)
    for b, im in enumerate(images):
        n, g = len(im[0]), len(im[2])
        det[b, :n], gb[b, :g], gl[b, :g] = im[0], np.asarray(im[1], np.float32).reshape(-1, 4), im[2]
        if im[3] is not None:
            crowd[b, :g] = im[3]
        area[b, :g] = CR.box_area(gb[b, :g]) if im[4] is None else im[4]
    return dict(images=images, det=det, counts=np.int32([len(im[0]) for im in images]), keep=None, n_kept=None, gb=gb, gl=gl,
                gt_counts=np.int32([len(im[2]) for im in images]),
                crowd=crowd if any(im[3] is not None for im in images) else None,
                area=area if any(im[4] is not None for im in images) else None)


COCO_RANGES = tuple((r[1], r[2]) for r in CR.COCO_AREA_RANGES)


def match_case(name, updates, C, thr=(.5, .75), max_dets=100, ignore_class=-1, areas=COCO_RANGES, capacity=None):
    return dict(name=name, updates=updates, C=C, thr=tuple(float(np.float32(v)) for v in thr), max_dets=max_dets,
                ignore_class=ignore_class, areas=tuple(areas), capacity=capacity)


def tiny_images(rng, B, C=3):
    out = []
    for _ in range(B):
        n = int(rng.integers(0, 7))
        dets = {c: int(k) for c, k in enumerate(rng.multinomial(n, [1 / C] * C)) if k}
        gts = {c: int(rng.integers(0, 3)) for c in range(C)}
        out.append(make_image(rng, dets, gts, crowd_p=.1))
    return out


def offsets_case(B):
    """One update of B tiny images (0 to 6 detections each) after an update of five: n_records starts above zero."""
    rng = np.random.default_rng(B)
    first, big = tiny_images(rng, 5), tiny_images(rng, B)
    return match_case(f"B{B}", [pad_update(first, R=6), pad_update(big, R=6)], 3)


def overflow_case():
    rng = np.random.default_rng(41)
    images = tiny_images(rng, 40)
    total = sum(len(im[0]) for im in images)
    return match_case("overflow", [pad_update(images, R=6)], 3, capacity=total // 2 + 1)


def filler_image(rng):
    return make_image(rng, {0: 2, 1: 1}, {0: 2, 1: 1})


def classes_case(n_classes):
    """n_classes classes with 1, 2, 3, 1, ... detections: segment starts at 6 k + {0, 1, 3} of the sorted keys."""
    rng = np.random.default_rng(100 + n_classes)
    dets = {c + 1: 1 + c % 3 for c in range(n_classes)}
    gts = {c + 1: 1 + (c % 2) for c in range(n_classes)}
    return match_case(f"classes{n_classes}", [pad_update([filler_image(rng), make_image(rng, dets, gts, crowd_p=.1)])], 132)


def cap_case(n, max_dets):
    """Class 1 with n detections before the cap, after 3 detections of class 0 and before 2 of class 2."""
    rng = np.random.default_rng(1000 * n + max_dets)
    im = make_image(rng, {0: 3, 1: n, 2: 2}, {0: 2, 1: 12, 2: 1}, crowd_p=.1, steps=50)
    return match_case(f"n{n}-cap{max_dets}", [pad_update([filler_image(rng), im])], 3, max_dets=max_dets)


def rows_case(R):
    """An image of exactly R detections over five classes of uneven size (class 3 holds half of them), cap 100."""
    rng = np.random.default_rng(7000 + R)
    n = rng.multinomial(R, [.1, .15, .15, .5, .1])
    dets = {c: int(k) for c, k in enumerate(n) if k}
    im = make_image(rng, dets, {c: 6 for c in range(5)}, crowd_p=.1, steps=200)
    assert len(im[0]) == R
    few = min(2, R - 1)
    filler = make_image(rng, {0: few} if few else {}, {0: 2, 1: 1})
    return match_case(f"R{R}", [pad_update([filler, im], R=R)], 5, thr=(.5,))


def gt_case(n_gt):
    """n_gt ground-truth boxes of class 1 among boxes of classes 0 and 2, labels -1 and C, padding past gt_counts; class 2 has
    detections and ground truth and is the ignored class."""
    rng = np.random.default_rng(300 + n_gt)
    d, gb, gl, crowd, _ = make_image(rng, {0: 3, 1: 40, 2: 5}, {0: 2, 1: n_gt, 2: 3}, crowd_p=.1)
    gb = np.concatenate([gb, boxes_of(rng, 2)])
    gl = np.concatenate([gl, [-1, 4]])
    crowd = np.concatenate([crowd, [0, 0]]).astype(np.uint8)
    order = rng.permutation(len(gl))
    im = (d, gb[order], gl[order], crowd[order], None)
    return match_case(f"gt{n_gt}", [pad_update([filler_image(rng), im], G=len(gl) + 5)], 4, ignore_class=2)


def det(*rows):
    return np.array(rows, np.float32).reshape(-1, 6)


def _im(d, gb, gl, crowd=None, area=None):
    return (det(*d), np.asarray(gb, np.float32).reshape(-1, 4), np.asarray(gl, np.int64),
            None if crowd is None else np.asarray(crowd, np.uint8), None if area is None else np.asarray(area, np.float32))


HALF_UP = float(np.nextafter(np.float32(.5), np.float32(1)))


def tie_cases():
    out = {}
    # equal IoU (1/3) with two different boxes: taking the later one leaves the first for the exact second detection
    out["equal_iou_later_gt"] = match_case("equal_iou_later_gt", [pad_update([_im(
        [[5, 0, 15, 10, .9, 0], [0, 0, 10, 10, .8, 0]], [[0, 0, 10, 10], [10, 0, 20, 10]], [0, 0])])], 1, thr=(.3,))
    out["duplicate_gt"] = match_case("duplicate_gt", [pad_update([_im(
        [[0, 0, 10, 10, .9, 0], [0, 0, 10, 10, .8, 0], [0, 0, 10, 10, .7, 0]], [[0, 0, 10, 10]] * 2 + [[50, 50, 60, 60]],
        [0, 0, 0])])], 1, thr=(.5, .75))
    out["iou_at_threshold"] = match_case("iou_at_threshold", [pad_update([_im(
        [[0, 0, 2, 1, .9, 0]], [[0, 0, 1, 1]], [0])])], 1, thr=(.5, HALF_UP))
    # equal scores: the lower row first; the cap of 4 cuts class 0's five equal scores after rows 1, 2, 3
    out["equal_scores_cap"] = match_case("equal_scores_cap", [pad_update([_im(
        [[70, 70, 80, 80, .9, 0]] + [[20 * i, 0, 20 * i + 10, 10, .5, 0] for i in range(5)] + [[0, 50, 9, 59, .5, 1]],
        [[20 * i, 0, 20 * i + 10, 10] for i in range(5)], [0] * 5)])], 2, thr=(.5,), max_dets=4)
    return out


def keep_case():
    """keep holds a permutation of the rows with -1 and R among its first n_kept entries and valid rows after them."""
    rng = np.random.default_rng(8)
    R = 40
    ups = []
    src = [make_image(rng, {0: 12, 1: 20, 2: 8}, {0: 3, 1: 4, 2: 2}) for _ in range(3)]
    keep = np.zeros((3, R), np.int32)
    n_kept = np.int32([30, 40, 0])
    seen = []
    for b, im in enumerate(src):
        k = rng.permutation(R).astype(np.int32)
        k[[3, 17]] = -1, R
        keep[b] = k
        live = [r for r in k[:n_kept[b]] if 0 <= r < R]
        seen.append((im[0][live],) + im[1:])
    up = pad_update(src, R=R)
    up.update(images=seen, counts=None, keep=keep, n_kept=n_kept)
    ups.append(up)
    return match_case("keep", ups, 3)


def odd_rows_case():
    d = [[0, 0, 10, 10, np.nan, 0], [0, 0, 10, 10, -0.0, 0], [0, 0, 10, 10, 0.0, 0], [20, 0, 30, 10, 0.0, 0],
         [40, 0, 50, 10, .5, 2.7], [40, 0, 50, 10, .6, -1], [40, 0, 50, 10, .7, -.5], [40, 0, 50, 10, .8, 3],
         [40, 0, 50, 10, -1.5, 2], [20, 0, 30, 10, np.inf, 0]]
    return match_case("odd_rows", [pad_update([_im(d, [[0, 0, 10, 10], [20, 0, 30, 10], [40, 0, 50, 10]], [0, 0, 2])])], 3)


def coco_special_case(areas=COCO_RANGES, name="coco_special", derived=False):
    """One image: class 0 a crowd region holding three detections; class 1 ground truth of area exactly 32^2 and 96^2 (the
    second by gt_area, its box is smaller), class 2 an unmatched 20 x 20 detection far from its ground truth.
    derived: no gt_area array at all (the 96^2 box is then drawn at that size)."""
    big = [200, 0, 296, 96] if derived else [200, 0, 260, 60]
    d = [[10, 10, 30, 30, .9, 0], [40, 40, 60, 60, .8, 0], [20, 50, 50, 90, .7, 0],
         [100, 0, 132, 32, .9, 1], big + [.8, 1], [300, 300, 320, 320, .9, 2]]
    gb = [[0, 0, 100, 100], [100, 0, 132, 32], big, [500, 500, 530, 530]]
    area = None if derived else [10000., 32. ** 2, 96. ** 2, 900.]
    return match_case(name, [pad_update([_im(d, gb, [0, 1, 1, 2], [1, 0, 0, 0], area)])], 3, thr=(.5, .75), areas=areas)


def negative_area_case():
    """The smallest input on which the plain metric and the COCO metric with the one range "all" differ: class 0 has a
    detection of area -100, which matches nothing, and a ground truth of area -200; class 1 an exact match.  The plain
    metric compares no area: a false positive and a counted ground truth.  "all" ignores both boxes of class 0."""
    d = [[10, 10, 5, 30, .9, 0], [100, 100, 120, 120, .8, 1]]
    gb = [[50, 50, 40, 70], [100, 100, 120, 120]]
    return match_case("negative_area", [pad_update([_im(d, gb, [0, 1])])], 2, thr=(.5, .75), areas=(COCO_RANGES[0],))


def want_match(case, coco):
    """The records of every update in order and npig: int32 rows [n, 11] and npig [C,A] from coco_eval_restated.match_image,
    or rows [n, 3] and npig [C] from test_detection_eval.evaluate_np."""
    if not coco:
        from test_detection_eval import evaluate_np
        r = evaluate_np([[im[:3] for im in up["images"]] for up in case["updates"]], case["C"], case["thr"],
                        case["max_dets"], case["ignore_class"])
        rows = np.stack([r["score"].view(np.int32), r["cls"], r["mask"].view(np.int32)], 1) if len(r["score"]) else \
            np.zeros((0, PLAIN_INTS), np.int32)
        return rows.astype(np.int32), r["npig"]
    lo = [np.float32(a[0]) for a in case["areas"]]
    hi = [np.float32(a[1]) for a in case["areas"]]
    recs, npig = [], np.zeros((case["C"], len(lo)), np.int64)
    for up in case["updates"]:
        for im in up["images"]:
            r, n = CR.match_image(im, list(case["thr"]), lo, hi, case["C"], case["max_dets"], case["ignore_class"])
            recs += r
            npig += n
    rows = np.zeros((len(recs), COCO_INTS), np.int32)
    for i, (s, c, q, tp, ig) in enumerate(recs):
        rows[i, 0] = np.float32(s).view(np.int32)
        rows[i, 1:3] = c, q
        rows[i, 3:7] = np.array(tp, np.uint32).view(np.int32)
        rows[i, 7:11] = np.array(ig, np.uint32).view(np.int32)
    return rows, npig
