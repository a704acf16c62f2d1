"""Training-side module surface of the reference (nets/frcnn_training.py) on HIP kernels.

The two target creators are deterministic in the reference (they keep "the first n by index", there is no random
sampling) and are reproduced with their indexing quirks (oracle/targets.py T1-T4, pinned by fixtures the reference's own
classes produced):

    AnchorTargetCreator(n_sample, pos_iou_thresh, neg_iou_thresh, pos_ratio)(bbox, anchor) -> (loc [A,4], label [A] int64)
    ProposalTargetCreator(n_sample, pos_ratio, pos_iou_thresh, neg_iou_thresh_high, neg_iou_thresh_low)
        (roi, bbox, label, loc_normalize_std) -> (sample_roi [S,4], gt_roi_loc [S,4], gt_roi_label [S] int64)

``FasterRCNNTrainer`` (nets/frcnn_training.py:179-342) is the class the reference's scripts instantiate: its forward runs
the detector conditioned on ground truth and returns the four losses, their sum and the head's per-RoI predictions
(pinned by tests/golden/trainer_ref.npz, made by the reference's own class).  Its eval_fn / calculate_metrics are not
provided: the reference's calculate_metrics has no return statement, loops over an empty range and calls the
one-argument compute_ap with two arguments, so it returns None or raises TypeError - there is no defined mAP to match.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import hip_ops
from .._ffi import TsodError, require_cuda
from ..models.hardnet import HarNetClassifier
from .classify import HarNetRoIHead
from .frcnn import _UID, _make_extractor
from .rpn import RegionProposalNetwork


class AnchorTargetCreator:
    def __init__(self, n_sample=256, pos_iou_thresh=0.7, neg_iou_thresh=0.3, pos_ratio=0.5):
        self.n_sample = n_sample
        self.pos_iou_thresh = pos_iou_thresh
        self.neg_iou_thresh = neg_iou_thresh
        self.pos_ratio = pos_ratio

    def __call__(self, bbox, anchor):
        """bbox [G,4] ground truth, anchor [A,4] -> (loc [A,4], label [A]: 1 positive / 0 negative / -1 ignored).
        Four launches (row arg-max, column arg-max, labels + positive cap, offsets), no host synchronisation."""
        require_cuda(anchor, "AnchorTargetCreator")
        loc, label, _ = hip_ops.anchor_targets(bbox, anchor, int(self.pos_ratio * self.n_sample), self.n_sample,
                                               self.pos_iou_thresh, self.neg_iou_thresh)
        return loc, label


class ProposalTargetCreator(object):
    def __init__(self, n_sample=128, pos_ratio=0.5, pos_iou_thresh=0.5, neg_iou_thresh_high=0.5, neg_iou_thresh_low=0):
        self.n_sample = n_sample
        self.pos_ratio = pos_ratio
        self.pos_roi_per_image = int(self.n_sample * self.pos_ratio)
        self.pos_iou_thresh = pos_iou_thresh
        self.neg_iou_thresh_high = neg_iou_thresh_high
        self.neg_iou_thresh_low = neg_iou_thresh_low

    def __call__(self, roi, bbox, label, loc_normalize_std=(0.1, 0.1, 0.2, 0.2)):
        """roi [R,4], bbox [G,4], label [G] -> (sample_roi [S,4], gt_roi_loc [S,4], gt_roi_label [S]), S <= n_sample.
        ``loc_normalize_std`` is accepted and unused, as in the reference (the division is commented out there).
        Two launches; reading S (and the IndexError flag of the reference's quirk T2) is the one host synchronisation."""
        require_cuda(roi, "ProposalTargetCreator")
        sample_roi, gt_roi_loc, gt_roi_label, counts = hip_ops.proposal_targets(
            roi, bbox, label, self.n_sample, self.pos_roi_per_image, self.pos_iou_thresh, self.neg_iou_thresh_high,
            self.neg_iou_thresh_low)
        n_keep, _, _, status = counts.tolist()
        if status:
            raise IndexError("index of a sampled negative is out of bounds for the kept labels "
                             "(the reference raises IndexError at nets/frcnn_training.py:175)")
        return sample_roi[:n_keep], gt_roi_loc[:n_keep], gt_roi_label[:n_keep].to(label.dtype)


class FasterRCNNTrainer(nn.Module):
    """The reference's ground-truth-conditioned forward (nets/frcnn_training.py:179-342) with its four losses.

    ``FasterRCNNTrainer(mode, num_classes, feat_stride=16, anchor_scales=[8,16,32], ratios=[0.5,1,2])`` as in the reference,
    plus the keyword-only ``backbone`` / ``roi_op`` of ``FasterRCNN`` and ``head_img_size``.  The attribute names are the
    reference's (``feat_extra``, ``classifier``, ``rpn``, ``head``, ...), so its ``state_dict`` has the reference's key set
    and shapes and a checkpoint of train/train.py loads with ``load_state_dict(ckpt['model_state_dict'], strict=True)``.

    ``forward(imgs, bboxes, labels, scale=1)`` -> (losses, anchors_pred [B,S,4], classes_pred [B,S] int64,
    classes_score_pred [B,S], bboxes[0][None], (labels[0] + 1)[None]) with losses = [rpn_loc, rpn_cls, roi_loc, roi_cls,
    their sum]: zero-dimensional tensors, each summed over the images and divided by their number (:333-342).
    ``imgs``: [B,3,H,W] on the GPU or a list of [3,H,W]; ``bboxes`` / ``labels``: lists (or batched tensors) of [G,4] / [G].

    The stages are the detector's own NHWC entry points, composed as ``FasterRCNN.forward`` composes them: the backbone
    plan, ``rpn.propose`` (train numbers with mode="train": 12000 -> 600), per image the two target creators, the head's
    fused GEMM on the stacked samples, then tsod_rpn_losses_f32 (reads the fused RPN output in place) and
    tsod_roi_losses_f32.  The host synchronises where ProposalTargetCreator does, once per image, and reads the two
    kernels' status words once after the last launch.

    Decisions (DESIGN.md "The trainer's forward"):
      * img_size: the reference hands imgs.shape[1:] = (C,H,W) to the RPN (quirk Q1) AND to the head (:252, quirk Q2 -
        the head then divides y by C = 3); a checkpoint of the reference learned its head that way, so that is the default.
        ``head_img_size="hw"`` hands the head (H,W), as ``FasterRCNN.forward`` does.
      * batch: the reference runs imgs[0] only and fails for more than one image; here every image runs against its own
        ground truth and the losses are averaged over B.  B = 1 is the reference's computation.
      * fewer than n_sample samples from ProposalTargetCreator (the reference's head fails there, quirk Q5): RuntimeError.
      * the module must be in eval() (BatchNorm folded), like the rest of the HIP path.
      * an IndexError of the proposal padding (quirk Q4) is recorded on the device as in ``FasterRCNN``: ``raise_if_error()``.

    Not provided: backward, optimizer and training (this is the forward with its losses - validation loss, the demo
    script's predictions); eval_fn / calculate_metrics (see the module docstring); graph capture and tuning (the forward
    runs whatever plan the backbone holds)."""

    def __init__(self, mode, num_classes, feat_stride=16, anchor_scales=[8, 16, 32], ratios=[0.5, 1, 2], *,
                 backbone="hardnet39", roi_op="pool", head_img_size="chw"):
        super().__init__()
        if head_img_size not in ("chw", "hw"):
            raise ValueError(f"head_img_size must be 'chw' (the reference's) or 'hw', got {head_img_size!r}")
        self.feat_extra, feat_ch, native_stride = _make_extractor(backbone)
        self.feat_stride = native_stride if (feat_stride == 16 and native_stride != 16) else feat_stride
        self.rpn_sigma = 1
        self.roi_sigma = 1
        self.n_classes = num_classes
        self.anchor_target_creator = AnchorTargetCreator()
        self.proposal_target_creator = ProposalTargetCreator()
        self.classifier = HarNetClassifier()
        self.rpn = RegionProposalNetwork(feat_ch, ratios=ratios, anchor_scales=anchor_scales, feat_stride=self.feat_stride,
                                         mode=mode)
        self.head = HarNetRoIHead(n_class=num_classes + 1, roi_size=7, spatial_scale=1, classifier=self.classifier,
                                  in_channels=feat_ch, roi_op=roi_op)
        self.loc_normalize_std = [0.1, 0.1, 0.2, 0.2]
        self.backbone = backbone
        self.head_img_size = head_img_size
        self.__dict__["_uid"] = next(_UID)          # scratch ownership, as FasterRCNN's

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__["_uid"] = next(_UID)

    def raise_if_error(self):
        """Surface the deferred IndexError of the proposal padding and a range violation of the fp16x2 conv arithmetic."""
        self.rpn.raise_if_error()
        self.feat_extra.raise_if_error()

    def forward(self, imgs, bboxes, labels, scale=1):
        if self.training:
            raise TsodError("the HIP path implements the inference forward only: call .eval() first")
        x = torch.stack(list(imgs)) if isinstance(imgs, (list, tuple)) else imgs
        require_cuda(x, "FasterRCNNTrainer.forward")
        B = x.shape[0]
        if len(bboxes) != B or len(labels) != B:
            raise ValueError(f"FasterRCNNTrainer.forward: {B} images, {len(bboxes)} box sets, {len(labels)} label sets")
        dev = x.device
        img_size = tuple(x.shape[1:])                                    # (C,H,W): quirk Q1 (RPN), Q2 (head)
        head_size = img_size if self.head_img_size == "chw" else tuple(x.shape[2:])
        n_sample = self.proposal_target_creator.n_sample
        with hip_ops.ARENA.scope((self._uid, 0)):
            feat = self.feat_extra.forward_nhwc(x, 0)
            plan = self.feat_extra._plan_for(x, 0)
            feat_amax, flag = (getattr(plan, "output_amax", 0) or None), getattr(plan, "range_flag", None)
            rpn_out, rois, anchor = self.rpn.propose(feat, img_size, scale, want_anchors=True, feat_amax=feat_amax,
                                                     range_flag=flag)
            gt_locs, gt_labels, s_rois, s_locs, s_labels = [], [], [], [], []
            for i in range(B):
                bbox = bboxes[i].to(dev, torch.float32)
                label = labels[i].to(dev)
                gt_loc, gt_label = self.anchor_target_creator(bbox, anchor)
                gt_locs.append(gt_loc)
                gt_labels.append(gt_label)
                s_roi, s_loc, s_label = self.proposal_target_creator(rois[i], bbox, label, self.loc_normalize_std)
                if s_roi.shape[0] < n_sample:
                    raise RuntimeError(f"ProposalTargetCreator kept {s_roi.shape[0]} samples for image {i}, fewer than "
                                       f"n_sample = {n_sample}: the reference's head fails on that (quirk Q5)")
                s_rois.append(s_roi)
                s_locs.append(s_loc)
                s_labels.append(s_label)
            rpn_loss, rpn_status = hip_ops.rpn_losses(rpn_out, self.rpn.anchor_base.shape[0], torch.stack(gt_locs),
                                                      torch.stack(gt_labels), self.rpn_sigma)
            sample_rois = torch.stack(s_rois)
            roi_indices = torch.arange(B, dtype=torch.int32, device=dev)
            roi_cls_locs, roi_scores = self.head.forward_nhwc(feat, sample_rois, roi_indices, head_size, feat_amax=feat_amax,
                                                              range_flag=flag)
            anchors_pred, classes_pred, classes_score_pred, roi_loss, roi_status = hip_ops.roi_losses(
                roi_cls_locs, roi_scores, sample_rois, torch.stack(s_locs), torch.stack(s_labels), self.roi_sigma)
            self.feat_extra.publish_range_word(plan)
        # (one read of the two status words, after the last launch: the reference raises IndexError there)
        bad = rpn_status.sum() + roi_status.sum()
        if int(bad):
            raise IndexError("a target class index is out of bounds for the logits it indexes "
                             "(the reference raises IndexError at nets/frcnn_training.py:274 / 313-331)")
        per = torch.cat([rpn_loss, roi_loss], dim=1).sum(0) / B        # [rpn_loc, rpn_cls, roi_loc, roi_cls]
        losses = list(per.unbind(0))
        losses = losses + [sum(losses)]
        return (losses, anchors_pred, classes_pred, classes_score_pred, torch.unsqueeze(bboxes[0], dim=0),
                torch.unsqueeze(labels[0] + 1, dim=0))
