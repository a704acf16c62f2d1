"""Detections drawn on the GPU: the figure of the reference's demo script (multi_inference.py:104-154)
as one HIP launch on u8 device images - box outlines and 5x7 bitmap text tags, painted in place, with no host read of the records.

The module is ``overlay``, not ``draw``: the reference's ``utils.draw`` is its matplotlib plotter of training curves.

* ``draw_bounding_boxes``  one style over one set of boxes (torchvision's ``draw_bounding_boxes`` on device images);
* ``draw_detections``      ground truth (green, ``GT: name`` above) and predictions (red, ``Pred: name`` / ``Conf: 0.xyz``
                           below) in one launch;
* ``multi_inference``      the script's loop body on a batch: trainer forward, the demo NMS at 0.1, ``draw_detections``.

The pixel rules are stated in include/tsod.h ("detection overlay"); nothing here touches a pixel.
"""
from __future__ import annotations

import torch

from .. import _ffi, hip_ops
from .._ffi import require_cuda
from .metrics import pack_ground_truth

GT_COLOR, PRED_COLOR = (0, 128, 0), (255, 0, 0)          # matplotlib's 'green' and 'red'
TAG_BG, TAG_ALPHA = (255, 255, 255), 204                 # the script's facecolor='white', alpha=0.8

_TABLES = {}                                             # (names, prefix, device) -> u8 [n,32] on that device


def _names(class_names):
    """class_names as a tuple indexed by class: a sequence, or the reference's ``{index: name}`` dict (holes are named
    ``class_<index>``, as the script's ``.get`` does)."""
    if class_names is None:
        return ()
    if isinstance(class_names, dict):
        n = max(class_names, default=-1) + 1
        return tuple(str(class_names.get(i, f"class_{i}")) for i in range(n))
    return tuple(str(s) for s in class_names)


def encode_strings(names, prefix=""):
    """HOST: ``prefix + name`` for every name as the kernel's table, a u8 [n,32] CPU tensor of zero-terminated rows.  A string
    longer than 31 bytes (UTF-8) raises ValueError."""
    rows = torch.zeros((len(names), _ffi.DRAW_STRING_BYTES), dtype=torch.uint8)
    for i, name in enumerate(names):
        raw = (prefix + name).encode("utf-8")
        if len(raw) > _ffi.DRAW_STRING_BYTES - 1 or b"\0" in raw:
            raise ValueError(f"overlay: {prefix + name!r} is {len(raw)} bytes; a tag string holds at most "
                             f"{_ffi.DRAW_STRING_BYTES - 1} and no zero byte")
        rows[i, :len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    return rows


def string_table(class_names, prefix, device):
    """The device table of ``prefix + name``, built and uploaded once per (class_names, prefix, device)."""
    key = (_names(class_names), str(prefix), torch.device(device))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = encode_strings(key[0], key[1]).to(key[2])
    return t


def _pad_rows(rows, what, widths):
    """A list of [n_i,w] tensors -> (padded [B,R,w] zeros-filled, counts [B] i32), as ``DetectionEvaluator._detections`` pads."""
    if not rows:
        raise ValueError(f"overlay: empty {what} list")
    for r in rows:
        require_cuda(r, "overlay")
        if r.dim() != 2 or r.shape[1] not in widths or r.shape[1] != rows[0].shape[1]:
            raise ValueError(f"overlay: {what} are [n,{'|'.join(str(w) for w in widths)}] rows, got {tuple(r.shape)}")
    dev = rows[0].device
    R = max(1, max(r.shape[0] for r in rows))
    padded = torch.zeros((len(rows), R, rows[0].shape[1]), dtype=torch.float32, device=dev)
    for b, r in enumerate(rows):
        padded[b, :r.shape[0]].copy_(r)
    ns = torch.tensor([r.shape[0] for r in rows], dtype=torch.int32).to(dev, non_blocking=True)
    return padded, ns


def _images(images, out):
    """-> (the [B,H,W,3] tensor to paint, the tensor to return)."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        require_cuda(images, "overlay")
    if images.dtype != torch.uint8 or images.dim() not in (3, 4) or images.shape[-1] != 3:
        raise ValueError(f"overlay: images are u8 [B,H,W,3] or [H,W,3], got {images.dtype} {tuple(images.shape)}")
    if out is None:
        out = images.clone(memory_format=torch.contiguous_format)
    elif out is not images:
        if not isinstance(out, torch.Tensor) or out.shape != images.shape or out.dtype != torch.uint8 or out.device != images.device:
            raise ValueError("overlay: out must be a u8 tensor of the images' shape on their device")
        out.copy_(images)
    return (out if out.dim() == 4 else out.unsqueeze(0)), out


def _rows(B, boxes, counts, keep, n_kept, what="boxes"):
    """The three row conventions of ``DetectionEvaluator.update`` -> (boxes [B,R,4|6], counts, keep, n_kept)."""
    if isinstance(boxes, (list, tuple)):
        if counts is not None or keep is not None or n_kept is not None:
            raise ValueError("overlay: counts / keep / n_kept go with a padded tensor")
        if len(boxes) != B:
            raise ValueError(f"overlay: {B} images, {len(boxes)} sets of {what}")
        boxes, counts = _pad_rows(list(boxes), what, (4, 6))
        return boxes, counts, None, None
    require_cuda(boxes, "overlay")
    if boxes.dim() == 2 and B == 1:
        boxes = boxes.unsqueeze(0)
    if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] not in (4, 6):
        raise ValueError(f"overlay: {what} are [B,R,4] or [B,R,6] for B={B}, got {tuple(boxes.shape)}")
    R = boxes.shape[1]
    if (keep is None) != (n_kept is None):
        raise ValueError("overlay: keep and n_kept go together")
    if keep is not None and counts is not None:
        raise ValueError("overlay: counts or (keep, n_kept), not both")
    dev = boxes.device
    if keep is not None:
        if tuple(keep.shape) != (B, R) or tuple(n_kept.shape) != (B,):
            raise ValueError(f"overlay: keep {tuple(keep.shape)} / n_kept {tuple(n_kept.shape)} for {what} {tuple(boxes.shape)}")
        keep, n_kept = keep.to(dev, torch.int32).contiguous(), n_kept.to(dev, torch.int32).contiguous()
    if counts is not None:
        counts = torch.as_tensor(counts)
        if tuple(counts.shape) != (B,):
            raise ValueError(f"overlay: counts {tuple(counts.shape)} for {B} images")
        counts = counts.to(dev, torch.int32, non_blocking=True).contiguous()
    return boxes.contiguous(), counts, keep, n_kept


def _group(B, boxes, labels, scores, counts, keep, n_kept, *, strings, color, width, alpha, tag, font_scale, padding,
           box_scale, label_offset, tag_bg=TAG_BG, tag_alpha=TAG_ALPHA):
    """One group dict of ``hip_ops.draw_groups``; ``strings``: the group's (first, count) rows of the string table."""
    if tag not in hip_ops.DRAW_TAGS:
        raise ValueError(f"overlay: tag is 'none', 'above' or 'below', got {tag!r}")
    boxes, counts, keep, n_kept = _rows(B, boxes, counts, keep, n_kept)
    R = boxes.shape[1]
    dev = boxes.device
    if isinstance(labels, (list, tuple)):
        if keep is not None or len(labels) != B:
            raise ValueError("overlay: a list of labels goes with a list of boxes, one entry per image")
        padded = torch.zeros((B, R), dtype=torch.int64, device=dev)
        for b, lb in enumerate(labels):
            if not isinstance(lb, torch.Tensor) or not lb.is_cuda:
                require_cuda(lb, "overlay")
            if lb.dim() != 1 or lb.shape[0] > R:
                raise ValueError(f"overlay: labels [n] beside boxes [n,4], got {tuple(lb.shape)}")
            padded[b, :lb.shape[0]].copy_(lb)
        labels = padded
    elif labels is not None:
        if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
            require_cuda(labels, "overlay")
        if labels.dim() == 1 and B == 1:
            labels = labels.unsqueeze(0)
        if tuple(labels.shape) != (B, R):
            raise ValueError(f"overlay: labels {tuple(labels.shape)} for boxes {tuple(boxes.shape)}")
        labels = labels.to(dev, torch.int64).contiguous()
    if scores is not None:
        require_cuda(scores, "overlay")
        if scores.dim() == 1 and B == 1:
            scores = scores.unsqueeze(0)
        if tuple(scores.shape) != (B, R):
            raise ValueError(f"overlay: scores {tuple(scores.shape)} for boxes {tuple(boxes.shape)}")
        rec = torch.zeros((B, R, 6), dtype=torch.float32, device=dev)          # the scores packed beside the boxes
        rec[..., :4].copy_(boxes[..., :4])
        rec[..., 4].copy_(scores)
        if boxes.shape[2] == 6:
            rec[..., 5].copy_(boxes[..., 5])
        boxes = rec
    return dict(boxes=boxes, counts=counts, keep=keep, n_kept=n_kept, labels=labels, label_offset=int(label_offset),
                strings=strings, scale=tuple(float(v) for v in box_scale), color=color, alpha=alpha, width=width,
                tag=tag if tag is not None else "none", text_color=color, tag_bg=tag_bg, tag_alpha=tag_alpha,
                font_scale=font_scale, padding=padding, score_line=boxes.shape[2] == 6)


def draw_bounding_boxes(images, boxes, labels=None, scores=None, *, counts=None, keep=None, n_kept=None, class_names=None,
                        prefix="", color=(255, 0, 0), width=2, alpha=255, tag="below", font_scale=1, box_scale=(1.0, 1.0),
                        label_offset=0, padding=2, tag_bg=TAG_BG, tag_alpha=TAG_ALPHA, out=None):
    """Box outlines and tags on u8 device images, one launch.

    ``images`` u8 [B,H,W,3] or [H,W,3]; the painted tensor is returned: ``out`` when given (``out=images`` paints in place),
    else a copy.  ``boxes``: [B,R,4], or [B,R,6] records (x1,y1,x2,y2,score,class), or a list of [n_i,4|6] tensors; the rows
    drawn follow ``DetectionEvaluator.update``: all, the first ``counts[b]``, or ``keep[b, :n_kept[b]]``.  ``labels`` ([B,R]
    int64 or a list of [n_i]) name the rows, else a record's class column does; ``scores`` [B,R] are packed beside the boxes
    and printed as ``Conf: d.ddd``, as a record's score column is.  Tag line 1 is ``prefix + class_names[label +
    label_offset]`` (``class_<index>`` outside the names or without names); rows that have neither label nor score get no
    tag, rows with a score only print the bare prefix.  ``box_scale`` = (sx, sy) maps box coordinates to image pixels.  No
    device-to-host copy, no synchronisation."""
    canvas, result = _images(images, out)
    B = canvas.shape[0]
    names = _names(class_names)
    unlabeled = labels is None and scores is not None and not isinstance(boxes, (list, tuple)) and boxes.shape[-1] == 4
    if unlabeled:
        names = ("",)
    strings = string_table(names, prefix, canvas.device) if names else None
    g = _group(B, boxes, labels, scores, counts, keep, n_kept, strings=(0, len(names)), color=color,
               width=width, alpha=alpha, tag=tag, font_scale=font_scale, padding=padding, box_scale=box_scale,
               label_offset=0 if unlabeled else label_offset, tag_bg=tag_bg, tag_alpha=tag_alpha)
    hip_ops.draw_groups(canvas, [g], strings)
    return result


def draw_detections(images, det, gt_boxes=None, gt_labels=None, *, counts=None, keep=None, n_kept=None, gt_counts=None,
                    class_names=None, box_scale=(1.0, 1.0), label_offset=0, gt_label_offset=0, width=2, font_scale=1, padding=2,
                    out=None):
    """The demo script's figure in ONE launch: ground truth in green with ``GT: <name>`` above each box, then predictions in
    red with ``Pred: <name>`` / ``Conf: d.ddd`` below, width 2, white tag backgrounds at alpha 204 (the script's 0.8).

    ``det``: ``FasterRCNN.predict``'s list of [n_i,6] tensors, or [B,R,6] records with ``counts``, or with ``keep`` /
    ``n_kept`` straight from ``postprocess``.  Ground truth: lists of [G_i,4] / [G_i] tensors or padded [B,G,4] / [B,G] with
    ``gt_counts`` (``metrics.pack_ground_truth``); None draws predictions only.  ``label_offset`` / ``gt_label_offset`` are
    added to the class before the name lookup (the trainer's predictions are 1-based: -1).  No device-to-host copy and no
    synchronisation."""
    canvas, result = _images(images, out)
    B = canvas.shape[0]
    dev = canvas.device
    names = _names(class_names)
    n = len(names)
    strings = None
    if n:                                                    # one table, two windows: GT rows first, then Pred rows
        key = (names, "GT: |Pred: ", dev)
        strings = _TABLES.get(key)
        if strings is None:
            strings = _TABLES[key] = torch.cat([encode_strings(names, "GT: "), encode_strings(names, "Pred: ")]).to(dev)
    style = dict(width=width, alpha=255, font_scale=font_scale, padding=padding, box_scale=box_scale)
    groups = []
    if gt_boxes is not None:
        gb, gl, gc = pack_ground_truth(gt_boxes, gt_labels, B, dev, gt_counts, who="draw_detections")
        groups.append(_group(B, gb, gl, None, gc, None, None, strings=(0, n), color=GT_COLOR, tag="above",
                             label_offset=gt_label_offset, **style))
    if isinstance(det, (list, tuple)):
        for r in det:
            if isinstance(r, torch.Tensor) and (r.dim() != 2 or r.shape[1] != 6):
                raise ValueError(f"draw_detections: detections are [n,6] rows, got {tuple(r.shape)}")
    elif isinstance(det, torch.Tensor) and det.shape[-1] != 6:
        raise ValueError(f"draw_detections: detections are [B,R,6] records, got {tuple(det.shape)}")
    groups.append(_group(B, det, None, None, counts, keep, n_kept, strings=(n, n), color=PRED_COLOR, tag="below",
                         label_offset=label_offset, **style))
    hip_ops.draw_groups(canvas, groups, strings)
    return result


def multi_inference(trainer, imgs, bboxes, labels, images_u8, class_names, iou_threshold=0.1):
    """The loop body of the reference's multi_inference.py:78-154 on a batch -> (annotated, det, keep, n_kept).

    ``trainer.forward(imgs, bboxes, labels)`` under ``torch.inference_mode()``; the demo's class-agnostic NMS at
    ``iou_threshold`` over ``anchors_pred`` with ``classes_score_pred`` as score (``hip_ops.filter_detections``); then
    ``draw_detections`` on ``images_u8`` (u8 [B,H,W,3], any size: ``box_scale`` is the ratio of the two sizes) with each
    image's own ground truth.  ``det`` [B,S,6] are the records in descending-score order, ``keep`` / ``n_kept`` the NMS
    survivors, as ``FasterRCNN.postprocess`` returns them.  The trainer's classes are 1-based (0 is the background), the
    ground-truth labels 0-based, as in the script; both are looked up in the same ``class_names``."""
    with torch.inference_mode():
        _, anchors_pred, classes_pred, classes_score_pred = trainer.forward(imgs, bboxes, labels)[:4]
        det = torch.cat([anchors_pred.float(), classes_score_pred.float().unsqueeze(-1), classes_pred.float().unsqueeze(-1)], dim=-1)
        det, keep, n_kept = hip_ops.filter_detections(det, iou_thr=iou_threshold)
        in_h, in_w = (imgs[0].shape[-2:] if isinstance(imgs, (list, tuple)) else imgs.shape[-2:])
        out_h, out_w = images_u8.shape[-3], images_u8.shape[-2]
        annotated = draw_detections(images_u8, det, list(bboxes), [lb.to(torch.int64) for lb in labels], keep=keep, n_kept=n_kept,
                                    class_names=class_names, box_scale=(out_w / in_w, out_h / in_h), label_offset=-1)
    return annotated, det, keep, n_kept
