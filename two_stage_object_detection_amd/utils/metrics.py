"""Detection mAP on HIP: COCO's mAP@[.5:.95] with 101 recall points, computed on the GPU.

The reference's ``calculate_metrics`` (nets/frcnn_training.py:372-565) loops over an empty range and calls the one-argument
``compute_ap`` with two arguments, so it defines no number to match: the metric is this project's, and it is COCOeval's
``evaluateImg`` + ``accumulate`` with area range "all" and no crowd / ignore flags:

* per image and class: detections ordered by descending score (ties: the lower row), the first ``max_dets`` kept (the cap
  is per (image, class), as COCOeval's), each taking the not yet matched ground truth of its class with the largest
  IoU >= t (equal IoUs: the higher GT index, COCOeval's ``<`` loop), every threshold on its own; IoU is the reference's
  ``bbox_iou`` (eps 1e-8, no +1) in f32, thresholds are f32;
* per class and threshold, over everything passed to ``update``: records sorted by descending score (ties: update order,
  then the image's position in its batch, then the per-image order), integer cumulative TP / FP, f64 precision made
  monotone from the right, sampled at the first position where ``100 tp >= k npig`` for k = 0..100 (0 where there is
  none) - an exact integer form of COCO's float ``searchsorted``, which differs from pycocotools only where a recall lands
  exactly on k/100 - and AP = the mean of the 101 samples;
* a class without ground truth is excluded (COCO's -1); a class with ground truth and no detection scores 0; mAP is the mean
  over the (class, threshold) pairs whose class has ground truth (NaN when there is none).

Deliberate deviations from the reference's evident intent: one-to-one matching (the reference counts a detection as a TP
when any GT of its class has IoU > t); classes without ground truth are excluded (the reference appends 0); the mAP is one
dataset-level number (the reference averages per-batch values); every image is scored against its own ground truth (the
reference uses ``bboxes[0]`` only).

``COCOEvaluator`` is the same metric with COCO's area ranges, crowd regions, ignore rules and
detection caps: the whole COCO table (AP, AP50, AP75, APs / APm / APl, AR1 / AR10 / AR100, ARs / ARm / ARl) from one pass.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import hip_ops
from .._ffi import TsodError, require_cuda

COCO_IOU_THRESHOLDS = tuple(float(np.float32(v)) for v in np.linspace(0.5, 0.95, 10))
COCO_AREA_RANGES = (("all", 0, 1e10), ("small", 0, 32 ** 2), ("medium", 32 ** 2, 96 ** 2), ("large", 96 ** 2, 1e10))
MAX_THRESHOLDS = 32


def _as_list(x, what, who="DetectionEvaluator.update"):
    if isinstance(x, torch.Tensor):
        return None
    if isinstance(x, (list, tuple)):
        return list(x)
    raise TypeError(f"{who}: {what} must be a tensor or a list of tensors, got {type(x).__name__}")


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _require_gpu(t, what):
    """require_cuda without its float32 rule (flags and labels)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        require_cuda(t, what)


def pack_ground_truth(gt_boxes, gt_labels, B, dev, gt_counts=None, who="DetectionEvaluator.update"):
    """Ground truth as the kernels take it -> (boxes [B,G,4] f32, labels [B,G] int64, counts [B] int32), all on ``dev``.
    Lists of [G_i,4] / [G_i] GPU tensors are padded to the largest G_i (zero boxes, label -1; the counts are uploaded without
    blocking; lists of equal lengths are stacked, there is nothing to pad); padded tensors [B,G,4] / [B,G] pass through with
    ``gt_counts`` (None: every row counts).  ``who`` names the caller in the messages.  Shared by both evaluators and the
    trainer's batched target assignment."""
    boxes, labels = _as_list(gt_boxes, "gt_boxes", who), _as_list(gt_labels, "gt_labels", who)
    if (boxes is None) != (labels is None):
        raise ValueError(f"{who}: gt_boxes and gt_labels are both lists or both tensors")
    if boxes is not None:
        if len(boxes) != B or len(labels) != B:
            raise ValueError(f"{who}: {B} images, {len(boxes)} box sets, {len(labels)} label sets")
        for bx, lb in zip(boxes, labels):
            require_cuda(bx, who)
            if not isinstance(lb, torch.Tensor) or not lb.is_cuda:
                require_cuda(lb, who)
            if bx.dim() != 2 or bx.shape[1] != 4 or lb.shape != bx.shape[:1]:
                raise ValueError(f"{who}: ground truth [G,4] / [G], got {tuple(bx.shape)} / "
                                 f"{tuple(lb.shape)}")
        G = max(bx.shape[0] for bx in boxes)
        if min(bx.shape[0] for bx in boxes) == G:                     # nothing to pad (B = 1 among them): one copy each
            return (torch.stack(boxes).to(dev), torch.stack(labels).to(dev, torch.int64),
                    torch.full((B,), G, dtype=torch.int32, device=dev))
        pb = torch.zeros((B, G, 4), dtype=torch.float32, device=dev)
        pl = torch.full((B, G), -1, dtype=torch.int64, device=dev)
        for b in range(B):
            g = boxes[b].shape[0]
            pb[b, :g].copy_(boxes[b])
            pl[b, :g].copy_(labels[b])
        gc = torch.tensor([bx.shape[0] for bx in boxes], dtype=torch.int32).to(dev, non_blocking=True)
        return pb, pl, gc
    require_cuda(gt_boxes, who)
    if not gt_labels.is_cuda:
        require_cuda(gt_labels, who)
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 4 or tuple(gt_labels.shape) != tuple(gt_boxes.shape[:2]):
        raise ValueError(f"{who}: padded ground truth [B,G,4] / [B,G] for B={B}, got "
                         f"{tuple(gt_boxes.shape)} / {tuple(gt_labels.shape)}")
    G = gt_boxes.shape[1]
    if gt_counts is None:
        gc = torch.full((B,), G, dtype=torch.int32, device=dev)
    else:
        gc = torch.as_tensor(gt_counts).to(dev, torch.int32, non_blocking=True).contiguous()
    return _aligned(gt_boxes), gt_labels.to(dev, torch.int64).contiguous(), gc


class DetectionEvaluator:
    """COCO-style detection mAP accumulated on the GPU.

    ``DetectionEvaluator(num_classes, iou_thresholds=0.50:0.95:0.05, max_dets=100, ignore_class=None)``: classes are
    evaluated in ``[0, num_classes)``; detections of ``ignore_class`` (and ground truth labelled with it) are not counted.

    ``update(det, gt_boxes, gt_labels, *, counts=None, keep=None, n_kept=None)`` takes the detections of a batch as
      * a padded [B,R,6] tensor of rows (x1,y1,x2,y2,score,class) with ``counts`` [B] (None: all R rows), or
      * ``postprocess()``'s triple: ``det`` = det_sorted [B,R,6], ``keep`` [B,R], ``n_kept`` [B], or
      * ``predict()``'s list of [n_i,6] tensors;
    and the ground truth as lists of [G_i,4] boxes / [G_i] labels or padded [B,G,4] / [B,G] tensors (pad labels with -1).
    Rows with a NaN score or a class outside the range are dropped.  GPU tensors only; no host synchronisation: the record
    buffer grows from the host-known upper bound B*R per call.  ``compute()`` reads the results back once and returns a dict
    (``mAP``, ``AP50`` / ``AP75`` when those thresholds are evaluated, ``AP`` [C,T] f64 with -1 for classes without ground
    truth, ``recall`` (likewise), ``TP`` / ``FP`` / ``FN`` [C,T] int64, ``npig`` [C] int64, ``iou_thresholds``).  ``reset()``
    clears the state."""

    _RECORD_INTS = hip_ops.EVAL_RECORD_INTS       # int32 words of one record row

    def __init__(self, num_classes: int, iou_thresholds=COCO_IOU_THRESHOLDS, max_dets: int = 100, ignore_class=None):
        thr = [float(np.float32(v)) for v in iou_thresholds]
        if not 0 < len(thr) <= MAX_THRESHOLDS:
            raise ValueError(f"DetectionEvaluator: 1 to {MAX_THRESHOLDS} IoU thresholds, got {len(thr)}")
        if int(num_classes) <= 0 or int(max_dets) <= 0:
            raise ValueError("DetectionEvaluator: num_classes and max_dets must be positive")
        self.num_classes = int(num_classes)
        self.iou_thresholds = tuple(thr)
        self.max_dets = int(max_dets)
        self.ignore_class = -1 if ignore_class is None else int(ignore_class)
        self.reset()

    def reset(self):
        self._device = None
        self._records = None            # [capacity, 3] int32: tsod_eval_record rows
        self._bound = 0                 # host-known upper bound of the live record count
        self._n = None                  # [1] int64 on the device: the live count
        self._npig = None               # [C] int64
        self._thr = None

    # -------------------------------------------------------------------------------------------------------------- state
    def _state(self, dev):
        if self._device is None:
            self._device = dev
            self._records = torch.empty((0, self._RECORD_INTS), dtype=torch.int32, device=dev)
            self._n = torch.zeros((1,), dtype=torch.int64, device=dev)
            self._npig = torch.zeros((self.num_classes,), dtype=torch.int64, device=dev)
            self._thr = torch.tensor(self.iou_thresholds, dtype=torch.float32, device=dev)
        elif dev != self._device:
            raise TsodError(f"DetectionEvaluator: inputs on {dev}, state on {self._device}")

    def _reserve(self, extra: int):
        need = self._bound + extra
        cap = self._records.shape[0]
        if need > cap:
            grown = torch.empty((max(need, 2 * cap), self._RECORD_INTS), dtype=torch.int32, device=self._device)
            if self._bound:
                grown[:self._bound].copy_(self._records[:self._bound])
            self._records = grown

    # ------------------------------------------------------------------------------------------------------------- inputs
    def _detections(self, det, counts, keep, n_kept):
        rows = _as_list(det, "det")
        if rows is not None:                                              # predict()'s list
            if counts is not None or keep is not None or n_kept is not None:
                raise ValueError("DetectionEvaluator.update: counts / keep / n_kept go with a padded det tensor")
            if not rows:
                raise ValueError("DetectionEvaluator.update: empty batch")
            for r in rows:
                require_cuda(r, "DetectionEvaluator.update")
                if r.dim() != 2 or r.shape[1] != 6:
                    raise ValueError(f"DetectionEvaluator.update: detections are [n,6] rows, got {tuple(r.shape)}")
            dev = rows[0].device
            R = max(1, max(r.shape[0] for r in rows))
            padded = torch.zeros((len(rows), R, 6), dtype=torch.float32, device=dev)
            for b, r in enumerate(rows):
                padded[b, :r.shape[0]].copy_(r)
            ns = torch.tensor([r.shape[0] for r in rows], dtype=torch.int32).to(dev, non_blocking=True)
            return padded, ns, None, None
        require_cuda(det, "DetectionEvaluator.update")
        if det.dim() != 3 or det.shape[2] != 6 or det.shape[0] == 0 or det.shape[1] == 0:
            raise ValueError(f"DetectionEvaluator.update: detections are [B,R,6], got {tuple(det.shape)}")
        B, R = det.shape[:2]
        det = det.contiguous()
        if (keep is None) != (n_kept is None):
            raise ValueError("DetectionEvaluator.update: keep and n_kept go together")
        if keep is not None:
            if counts is not None:
                raise ValueError("DetectionEvaluator.update: counts or (keep, n_kept), not both")
            if tuple(keep.shape) != (B, R) or tuple(n_kept.shape) != (B,):
                raise ValueError(f"DetectionEvaluator.update: keep {tuple(keep.shape)} / n_kept {tuple(n_kept.shape)} for "
                                 f"detections {tuple(det.shape)}")
            return det, None, keep.to(det.device, torch.int32).contiguous(), n_kept.to(det.device, torch.int32).contiguous()
        if counts is None:
            counts = torch.full((B,), R, dtype=torch.int32, device=det.device)
        elif tuple(counts.shape) != (B,):
            raise ValueError(f"DetectionEvaluator.update: counts {tuple(counts.shape)} for {B} images")
        return det, counts.to(det.device, torch.int32).contiguous(), None, None

    def _ground_truth(self, gt_boxes, gt_labels, B, dev, gt_counts):
        return pack_ground_truth(gt_boxes, gt_labels, B, dev, gt_counts)

    def update(self, det, gt_boxes, gt_labels, *, counts=None, keep=None, n_kept=None, gt_counts=None):
        self._update(det, gt_boxes, gt_labels, counts, keep, n_kept, gt_counts)

    def _update(self, det, gt_boxes, gt_labels, counts, keep, n_kept, gt_counts, **per_gt):
        """``update`` of both evaluators; ``per_gt``: a subclass's arrays beside the labels, padded by its ``_per_gt`` and
        passed on to its ``_match``."""
        det, counts, keep, n_kept = self._detections(det, counts, keep, n_kept)
        B, R = det.shape[:2]
        dev = det.device
        gb, gl, gc = self._ground_truth(gt_boxes, gt_labels, B, dev, gt_counts)
        per_gt = {what: self._per_gt(x, what, gl) for what, x in per_gt.items()}
        self._state(dev)
        self._reserve(B * R)
        self._match(det, gb, gl, gc, counts=counts, keep=keep, n_kept=n_kept, **per_gt)
        self._bound += B * R

    def _match(self, det, gb, gl, gc, **rows):
        hip_ops.eval_match(det, gb, gl, gc, self._thr, self.num_classes, self.max_dets, self.ignore_class, self._records,
                           self._n, self._npig, **rows)

    # ------------------------------------------------------------------------------------------------------------ results
    def records(self):
        """The records so far, in record order, read back to the host (a test / debugging accessor):
        (score [N] f32, class [N] int32, TP mask [N] uint32) numpy arrays."""
        if self._device is None:
            return np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint32)
        n = int(self._n.item())
        r = self._records[:n].cpu().numpy()
        return r[:, 0].view(np.float32).copy(), r[:, 1].copy(), r[:, 2].view(np.uint32).copy()

    def _accumulate(self, T):
        return hip_ops.eval_accumulate(self._records, self._n, self._npig, T)

    def _compute(self):
        """The accumulate and the one host read -> (AP, recall) as f64 arrays and the result entries both evaluators have."""
        if self._device is None:
            raise RuntimeError(f"{type(self).__name__}.compute: nothing was passed to update()")
        self._reserve(1)                                                  # capacity > 0 even when every batch was empty
        out = self._accumulate(len(self.iou_thresholds))
        host = torch.cat([out.view(-1), self._npig.view(-1)]).cpu().numpy()   # the one host read
        body = host[:out.numel()].reshape(tuple(out.shape))
        ap, recall = body[0].view(np.float64), body[4].view(np.float64)
        return ap, recall, {
            "recall": torch.from_numpy(recall.copy()),
            "TP": torch.from_numpy(body[1].copy()),
            "FP": torch.from_numpy(body[2].copy()),
            "FN": torch.from_numpy(body[3].copy()),
            "npig": torch.from_numpy(host[out.numel():].reshape(tuple(self._npig.shape)).copy()),
            "iou_thresholds": self.iou_thresholds,
        }

    def compute(self) -> dict:
        ap, _, common = self._compute()
        has_gt = common["npig"].numpy() > 0
        res = {"mAP": _mean(ap[has_gt].ravel()), "AP": torch.from_numpy(ap.copy()), **common}
        for name, v in (("AP50", 0.5), ("AP75", 0.75)):
            for t, thr in enumerate(self.iou_thresholds):
                if thr == float(np.float32(v)):
                    res[name] = _mean(ap[has_gt, t])
        return res


class COCOEvaluator(DetectionEvaluator):
    """COCOeval's detection table in one pass on the GPU: ``DetectionEvaluator``'s metric with area
    ranges, crowd regions, COCO's ignore rules and several detection caps.

    ``COCOEvaluator(num_classes, iou_thresholds=0.50:0.95:0.05, max_dets=(1, 10, 100), area_ranges=COCO_AREA_RANGES,
    ignore_class=None)``: ``max_dets`` are ascending caps per (image, class), at most 4; ``area_ranges`` are at most 4
    ``(name, lo, hi)`` triples with both bounds inclusive (f32).

    ``update(det, gt_boxes, gt_labels, *, gt_crowd=None, gt_area=None, counts=None, keep=None, n_kept=None, gt_counts=None)``
    takes every input form of ``DetectionEvaluator.update``; ``gt_crowd`` (nonzero = a crowd region) and ``gt_area`` (replaces
    the box's own area (x2-x1)*(y2-y1)) are lists of [G_i] tensors or padded [B,G] tensors.  No host synchronisation.
    ``compute()`` reads the results back once and returns COCO's numbers - ``AP`` / ``AP50`` / ``AP75`` (area "all", the last
    cap), ``APs`` / ``APm`` / ``APl``, ``AR<cap>`` for every cap (area "all"), ``ARs`` / ``ARm`` / ``ARl`` (the last cap), each
    the mean over the entries that are not -1 and present only when its threshold, range ("all" / "small" / "medium" / "large"
    by name) and cap are configured - with the arrays ``precision`` and ``recall`` [C,A,M,T] f64 (-1 where the class has no
    not-ignored ground truth in the range), ``TP`` / ``FP`` / ``FN`` [C,A,M,T] int64, ``npig`` [C,A] int64 and
    ``iou_thresholds``, ``area_ranges``, ``max_dets``."""

    _RECORD_INTS = hip_ops.EVAL_COCO_RECORD_INTS

    def __init__(self, num_classes: int, iou_thresholds=COCO_IOU_THRESHOLDS, max_dets=(1, 10, 100),
                 area_ranges=COCO_AREA_RANGES, ignore_class=None):
        caps = tuple(int(m) for m in max_dets)
        if not 0 < len(caps) <= hip_ops.EVAL_COCO_MAX_CAPS or caps[0] <= 0 or any(a >= b for a, b in zip(caps, caps[1:])):
            raise ValueError(f"COCOEvaluator: 1 to {hip_ops.EVAL_COCO_MAX_CAPS} ascending positive caps, got {max_dets}")
        ranges = tuple((str(name), float(np.float32(lo)), float(np.float32(hi))) for name, lo, hi in area_ranges)
        if not 0 < len(ranges) <= hip_ops.EVAL_COCO_MAX_AREAS:
            raise ValueError(f"COCOEvaluator: 1 to {hip_ops.EVAL_COCO_MAX_AREAS} area ranges, got {len(ranges)}")
        super().__init__(num_classes, iou_thresholds, caps[-1], ignore_class)
        self.caps = caps
        self.area_ranges = ranges

    def _state(self, dev):
        fresh = self._device is None
        super()._state(dev)
        if fresh:
            self._npig = torch.zeros((self.num_classes, len(self.area_ranges)), dtype=torch.int64, device=dev)
            self._lo = torch.tensor([r[1] for r in self.area_ranges], dtype=torch.float32, device=dev)
            self._hi = torch.tensor([r[2] for r in self.area_ranges], dtype=torch.float32, device=dev)

    @staticmethod
    def _per_gt(x, what, like):
        """gt_crowd (uint8) / gt_area (f32) as a padded [B,G] tensor beside the padded labels ``like`` (None stays None)."""
        if x is None:
            return None
        dtype = {"gt_crowd": torch.uint8, "gt_area": torch.float32}[what]
        B, G = like.shape
        rows = _as_list(x, what)
        if rows is None:
            _require_gpu(x, "COCOEvaluator.update")
            if tuple(x.shape) != (B, G):
                raise ValueError(f"COCOEvaluator.update: {what} {tuple(x.shape)} beside ground truth [{B},{G}]")
            return (x != 0).to(dtype).contiguous() if dtype == torch.uint8 else x.to(dtype).contiguous()
        if len(rows) != B:
            raise ValueError(f"COCOEvaluator.update: {B} images, {len(rows)} {what} sets")
        out = torch.zeros((B, G), dtype=dtype, device=like.device)
        for b, r in enumerate(rows):
            _require_gpu(r, "COCOEvaluator.update")
            if r.dim() != 1 or r.shape[0] > G:
                raise ValueError(f"COCOEvaluator.update: {what} [G] per image, got {tuple(r.shape)}")
            out[b, :r.shape[0]].copy_((r != 0) if dtype == torch.uint8 else r)
        return out

    def update(self, det, gt_boxes, gt_labels, *, gt_crowd=None, gt_area=None, counts=None, keep=None, n_kept=None,
               gt_counts=None):
        self._update(det, gt_boxes, gt_labels, counts, keep, n_kept, gt_counts, gt_crowd=gt_crowd, gt_area=gt_area)

    def _match(self, det, gb, gl, gc, **rows):
        hip_ops.eval_match_coco(det, gb, gl, gc, self._thr, self._lo, self._hi, self.num_classes, self.max_dets,
                                self.ignore_class, self._records, self._n, self._npig, **rows)

    def records(self):
        """The records so far, in record order, read back to the host (a test / debugging accessor): (score [N] f32,
        class [N] int32, rank [N] int32, TP masks [N,4] uint32, ignore masks [N,4] uint32) numpy arrays."""
        n = 0 if self._device is None else int(self._n.item())
        r = self._records[:n].cpu().numpy() if n else np.zeros((0, self._RECORD_INTS), np.int32)
        return (r[:, 0].view(np.float32).copy(), r[:, 1].copy(), r[:, 2].copy(), r[:, 3:7].view(np.uint32).copy(),
                r[:, 7:11].view(np.uint32).copy())

    def _accumulate(self, T):
        return hip_ops.eval_accumulate_coco(self._records, self._n, self._npig, T, self.caps, self.max_dets)

    def compute(self) -> dict:
        ap, recall, common = self._compute()
        res = {"precision": torch.from_numpy(ap.copy()), **common, "area_ranges": self.area_ranges, "max_dets": self.caps}
        res.update(coco_summary(ap, recall, self.iou_thresholds, [r[0] for r in self.area_ranges], self.caps))
        return res


def coco_summary(precision, recall, iou_thresholds, area_names, caps) -> dict:
    """COCO's summary numbers from the [C,A,M,T] arrays: each the ``_mean`` of the entries that are not -1 (NaN when there is
    none); a key is present only when its threshold, area range (by name) and cap are configured."""
    area = {name: a for a, name in reversed(list(enumerate(area_names)))}

    def valid(x):
        return x[x > -1]

    res = {}
    last = len(caps) - 1
    if "all" in area:
        res["AP"] = _mean(valid(precision[:, area["all"], last, :]))
        for name, v in (("AP50", 0.5), ("AP75", 0.75)):
            for t, thr in enumerate(iou_thresholds):
                if thr == float(np.float32(v)):
                    res[name] = _mean(valid(precision[:, area["all"], last, t]))
        for m, cap in enumerate(caps):
            res[f"AR{cap}"] = _mean(valid(recall[:, area["all"], m, :]))
    for key, name in (("s", "small"), ("m", "medium"), ("l", "large")):
        if name in area:
            res["AP" + key] = _mean(valid(precision[:, area[name], last, :]))
            res["AR" + key] = _mean(valid(recall[:, area[name], last, :]))
    return res


def _mean(values) -> float:
    """Mean of f64 values with one correctly rounded sum (math.fsum): independent of their order; NaN when empty."""
    values = list(np.asarray(values, dtype=np.float64).ravel())
    return math.fsum(values) / len(values) if values else float("nan")
