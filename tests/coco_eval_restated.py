"""The COCO detection metric of DESIGN.md section 4.25, restated in numpy from its definition (CPU, no GPU).

Plain loops per image, class, area range, threshold, detection and ground truth, with f32 boxes, areas and IoUs; the
accumulate is per (class, range, cap, threshold) with integer counts and f64 precision.  tests/test_coco_eval.py pins its
answers by hand, tests/test_hip_coco_eval.py measures the HIP evaluator against it.

An image is ``(det [n,6], gt_boxes [G,4], gt_labels [G])`` or ``(det, gt_boxes, gt_labels, crowd [G] | None, area [G] | None)``;
a batch is a list of images; ``updates`` is a list of batches.
"""
import math

import numpy as np

N_RECALL = 101
MAX_AREAS = 4
EPS = np.float32(1e-8)
COCO_THRESHOLDS = tuple(np.linspace(0.5, 0.95, 10).astype(np.float32).tolist())
COCO_AREA_RANGES = (("all", 0, 1e10), ("small", 0, 32 ** 2), ("medium", 32 ** 2, 96 ** 2), ("large", 96 ** 2, 1e10))


def box_area(b):
    b = np.asarray(b, np.float32).reshape(-1, 4)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def intersection(a, b):
    """[n,4] x [m,4] f32 -> [n,m] f32 intersection areas (negative extents clamp to 0)."""
    a = np.asarray(a, np.float32).reshape(-1, 1, 4)
    b = np.asarray(b, np.float32).reshape(1, -1, 4)
    w = np.fmax(np.fmin(a[..., 2], b[..., 2]) - np.fmax(a[..., 0], b[..., 0]), np.float32(0))
    h = np.fmax(np.fmin(a[..., 3], b[..., 3]) - np.fmax(a[..., 1], b[..., 1]), np.float32(0))
    return w * h


def iou_f32(a, b):
    """The project's bbox_iou: inter / (area_a + area_b - inter + 1e-8), every step rounded to f32."""
    inter = intersection(a, b)
    return inter / (box_area(a)[:, None] + box_area(b)[None, :] - inter + EPS)


def crowd_iou_f32(a, b):
    """Detection a against crowd region b: inter / (area_a + 1e-8)."""
    return intersection(a, b) / (box_area(a)[:, None] + EPS)


def match_image(image, thr, lo, hi, num_classes, max_dets, ignore_class):
    """One image -> (records [(score, class, rank, tp masks [4], ignore masks [4])] in per-image order, npig [C,A])."""
    det = np.asarray(image[0], np.float32).reshape(-1, 6)
    gt_boxes = np.asarray(image[1], np.float32).reshape(-1, 4)
    gt_labels = np.asarray(image[2], np.int64).reshape(-1)
    G, A, T = len(gt_labels), len(lo), len(thr)
    crowd = np.zeros(G, bool) if len(image) < 4 or image[3] is None else np.asarray(image[3]).reshape(-1) != 0
    g_area = box_area(gt_boxes) if len(image) < 5 or image[4] is None else np.asarray(image[4], np.float32).reshape(-1)
    gt_ok = (gt_labels >= 0) & (gt_labels < num_classes) & (gt_labels != ignore_class)
    with np.errstate(invalid="ignore"):
        g_ignore = [crowd | (g_area < lo[a]) | (g_area > hi[a]) for a in range(A)]
    npig = np.zeros((num_classes, A), np.int64)
    for g in np.nonzero(gt_ok)[0]:
        for a in range(A):
            if not g_ignore[a][g]:
                npig[gt_labels[g], a] += 1
    s, c = det[:, 4], det[:, 5]
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(s) & (c >= 0) & (c < num_classes)
    cls = np.where(ok, c, 0).astype(np.int64)
    ok &= cls != ignore_class
    rows = np.nonzero(ok)[0]
    d_area = box_area(det[:, :4])
    records = []
    for k in np.unique(cls[rows]):
        mine = rows[cls[rows] == k]
        order = mine[np.lexsort((mine, -s[mine]))][:max_dets]            # descending score, ties to the lower row
        g_idx = np.nonzero(gt_ok & (gt_labels == k))[0]
        plain = iou_f32(det[order, :4], gt_boxes[g_idx])
        ious = np.where(crowd[g_idx][None, :], crowd_iou_f32(det[order, :4], gt_boxes[g_idx]), plain).tolist()
        is_crowd = crowd[g_idx].tolist()
        tp = [[0] * MAX_AREAS for _ in order]
        ig = [[0] * MAX_AREAS for _ in order]
        for a in range(A):
            ign = g_ignore[a][g_idx].tolist()
            walk = [j for j in range(len(g_idx)) if not ign[j]] + [j for j in range(len(g_idx)) if ign[j]]
            with np.errstate(invalid="ignore"):
                d_out = ((d_area[order] < lo[a]) | (d_area[order] > hi[a])).tolist()
            for t in range(T):
                matched = [False] * len(g_idx)
                for q in range(len(order)):
                    best, m = thr[t], -1
                    for j in walk:
                        if matched[j] and not is_crowd[j]:
                            continue
                        if m >= 0 and not ign[m] and ign[j]:
                            break
                        if not ious[q][j] >= best:
                            continue
                        best, m = ious[q][j], j
                    if m >= 0:
                        matched[m] = True
                        if ign[m]:
                            ig[q][a] |= 1 << t
                        else:
                            tp[q][a] |= 1 << t
                    elif d_out[q]:
                        ig[q][a] |= 1 << t
        for q, r in enumerate(order):
            records.append((s[r], int(k), q, tp[q], ig[q]))
    return records, npig


def accumulate(score, cls, rank, tp, ig, npig, T, caps):
    C, A = npig.shape
    M = len(caps)
    precision = np.full((C, A, M, T), -1.0)
    recall = np.full((C, A, M, T), -1.0)
    TP = np.zeros((C, A, M, T), np.int64)
    FP = np.zeros((C, A, M, T), np.int64)
    FN = np.zeros((C, A, M, T), np.int64)
    for c in range(C):
        idx = np.nonzero(cls == c)[0]
        idx = idx[np.argsort(-score[idx], kind="stable")]                 # ties keep record order
        for a in range(A):
            n_gt = int(npig[c, a])
            for m, cap in enumerate(caps):
                for t in range(T):
                    live = idx[(rank[idx] < cap) & (((ig[idx, a] >> np.uint32(t)) & np.uint32(1)) == 0)]
                    hits = ((tp[live, a] >> np.uint32(t)) & np.uint32(1)).astype(np.int64)
                    cum = np.cumsum(hits)
                    n = len(live)
                    TP[c, a, m, t] = cum[-1] if n else 0
                    FP[c, a, m, t] = n - TP[c, a, m, t]
                    FN[c, a, m, t] = n_gt - TP[c, a, m, t]
                    if n_gt == 0:
                        continue
                    prec = cum.astype(np.float64) / np.arange(1, n + 1, dtype=np.float64)
                    env = np.maximum.accumulate(prec[::-1])[::-1] if n else prec
                    at = np.searchsorted(100 * cum, np.arange(N_RECALL) * n_gt, side="left")   # first i: 100 tp >= k npig
                    total = 0.0
                    for i in at.tolist():
                        total += float(env[i]) if i < n else 0.0
                    precision[c, a, m, t] = total / N_RECALL
                    recall[c, a, m, t] = float(TP[c, a, m, t]) / float(n_gt)
    return precision, recall, TP, FP, FN


def mean_valid(x):
    vals = [float(v) for v in np.asarray(x, np.float64).ravel() if v > -1]
    return math.fsum(vals) / len(vals) if vals else float("nan")


def summarize(precision, recall, thresholds, area_names, caps):
    """COCO's twelve numbers (those whose threshold, range and cap are configured)."""
    names = list(area_names)
    stats, last = {}, len(caps) - 1
    if "all" in names:
        a = names.index("all")
        stats["AP"] = mean_valid(precision[:, a, last, :])
        for key, v in (("AP50", 0.5), ("AP75", 0.75)):
            if float(np.float32(v)) in thresholds:
                stats[key] = mean_valid(precision[:, a, last, thresholds.index(float(np.float32(v)))])
        for m, cap in enumerate(caps):
            stats[f"AR{cap}"] = mean_valid(recall[:, a, m, :])
    for key, name in (("s", "small"), ("m", "medium"), ("l", "large")):
        if name in names:
            stats["AP" + key] = mean_valid(precision[:, names.index(name), last, :])
            stats["AR" + key] = mean_valid(recall[:, names.index(name), last, :])
    return stats


def evaluate_coco_np(updates, num_classes, thresholds=COCO_THRESHOLDS, max_dets=(1, 10, 100), area_ranges=COCO_AREA_RANGES,
                     ignore_class=-1):
    thr = [float(np.float32(v)) for v in thresholds]
    caps = [int(m) for m in max_dets]
    lo = [np.float32(r[1]) for r in area_ranges]
    hi = [np.float32(r[2]) for r in area_ranges]
    recs, npig = [], np.zeros((num_classes, len(area_ranges)), np.int64)
    for batch in updates:
        for image in batch:
            r, n = match_image(image, thr, lo, hi, num_classes, caps[-1], ignore_class)
            recs += r
            npig += n
    score = np.array([r[0] for r in recs], np.float32)
    cls = np.array([r[1] for r in recs], np.int32)
    rank = np.array([r[2] for r in recs], np.int32)
    tp = np.array([r[3] for r in recs], np.uint32).reshape(-1, MAX_AREAS)
    ig = np.array([r[4] for r in recs], np.uint32).reshape(-1, MAX_AREAS)
    precision, recall, TP, FP, FN = accumulate(score, cls, rank, tp, ig, npig, len(thr), caps)
    return dict(score=score, cls=cls, rank=rank, tp=tp, ig=ig, npig=npig, precision=precision, recall=recall, TP=TP, FP=FP,
                FN=FN, stats=summarize(precision, recall, thr, [r[0] for r in area_ranges], caps))
