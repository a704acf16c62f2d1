"""Training-side module surface of the reference (nets/frcnn_training.py) on HIP kernels.

The two target creators are deterministic in the reference (they keep "the first n by index", there is no random
sampling) and are reproduced with their indexing quirks (oracle/targets.py T1-T4, pinned by fixtures the reference's own
classes produced):

    AnchorTargetCreator(n_sample, pos_iou_thresh, neg_iou_thresh, pos_ratio)(bbox, anchor) -> (loc [A,4], label [A] int64)
    ProposalTargetCreator(n_sample, pos_ratio, pos_iou_thresh, neg_iou_thresh_high, neg_iou_thresh_low)
        (roi, bbox, label, loc_normalize_std) -> (sample_roi [S,4], gt_roi_loc [S,4], gt_roi_label [S] int64)

Beyond the reference, both have ``batch``: the same assignment for every image of a batch in one pass (four and two launches
for all of them, nothing read back), which is what ``FasterRCNNTrainer.forward`` calls.

``FasterRCNNTrainer`` (nets/frcnn_training.py:179-342) is the class the reference's scripts instantiate: its forward runs
the detector conditioned on ground truth and returns the four losses, their sum and the head's per-RoI predictions
(pinned by tests/golden/trainer_ref.npz, made by the reference's own class).  Its ``eval_fn`` / ``calculate_metrics``
score with the project's own metric (``utils.metrics.DetectionEvaluator``): the reference's
calculate_metrics loops over an empty range and calls the one-argument compute_ap with two arguments, so there is no
reference mAP to match.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import nn

from .. import hip_ops
from .._ffi import TsodError, require_cuda
from ..models.hardnet import HarNetClassifier
from .classify import HarNetRoIHead
from .frcnn import _UID, _make_extractor
from .rpn import RegionProposalNetwork
from ..utils.metrics import COCOEvaluator, DetectionEvaluator, pack_ground_truth


def _check_pos_ratio(who, pos_ratio):
    """With pos_ratio > 1 the positive cap exceeds n_sample and the reference's negative slices (``i[n_neg:]``,
    ``i[:neg_roi_per_this_image]``) take a negative bound: they drop only the LAST |n_sample - positives| negatives.  The
    kernels do not restate that accident (they clamp at zero), and a negative ratio is a negative cap, so both are refused."""
    if not 0.0 <= pos_ratio <= 1.0:
        raise ValueError(f"{who}: pos_ratio must lie in [0, 1], got {pos_ratio}")


class PackedGroundTruth(NamedTuple):
    """A batch's ground truth as the batched target kernels take it (``pack_targets``): both creators' ``batch`` accept it in
    place of ``bboxes``, so a caller packs and uploads once."""
    boxes: torch.Tensor            # [B,Gmax,4] f32 on the device
    labels: torch.Tensor           # [B,Gmax] on the device (any value in the pad rows)
    counts: torch.Tensor           # [B] int32 on the device
    host_counts: tuple             # the same numbers on the host, each in [0, Gmax]


def host_gt_counts(gt_counts, bboxes, who):
    """``gt_counts`` (a sequence of ints or a CPU integer tensor) checked on the host against padded ``bboxes`` [B,Gmax,4] ->
    a tuple of B ints, each in [0, Gmax]; ValueError otherwise."""
    if not isinstance(bboxes, torch.Tensor) or bboxes.dim() != 3:
        raise ValueError(f"{who}: gt_counts goes with padded tensors [B,Gmax,4] / [B,Gmax], not with lists")
    if isinstance(gt_counts, torch.Tensor) and gt_counts.is_cuda:
        raise ValueError(f"{who}: gt_counts must be known on the host (a sequence of ints or a CPU integer tensor)")
    host = tuple(int(v) for v in (gt_counts.tolist() if isinstance(gt_counts, torch.Tensor) else gt_counts))
    B, Gmax = bboxes.shape[:2]
    if len(host) != B:
        raise ValueError(f"{who}: {len(host)} gt_counts for {B} images")
    bad = [v for v in host if not 0 <= v <= Gmax]
    if bad:
        raise ValueError(f"{who}: gt_counts must lie in [0, Gmax = {Gmax}], got {bad[0]}")
    return host


def pack_targets(bboxes, labels, gt_counts, dev, who) -> PackedGroundTruth:
    """Lists of [G_i,4] / [G_i] tensors, or padded [B,Gmax,4] / [B,Gmax] tensors with ``gt_counts`` (a sequence of ints or a CPU
    integer tensor; None: every row counts) -> ``PackedGroundTruth`` on ``dev``.  Lists are packed by the evaluators' helper
    (``utils.metrics.pack_ground_truth``).  ``labels=None``: zeros (the anchor targets do not read them).  ``gt_counts`` is
    validated here, on the host: a value outside [0, Gmax] raises ValueError before anything is launched; it is uploaded
    without blocking."""
    if isinstance(bboxes, torch.Tensor):
        bboxes = bboxes.to(dev, torch.float32)
        if bboxes.dim() != 3 or bboxes.shape[-1] != 4:
            raise ValueError(f"{who}: padded ground truth [B,Gmax,4], got {tuple(bboxes.shape)}")
        B, Gmax = bboxes.shape[:2]
        labels = torch.zeros((B, Gmax), dtype=torch.int64, device=dev) if labels is None else labels.to(dev)
        host = (Gmax,) * B if gt_counts is None else host_gt_counts(gt_counts, bboxes, who)
    else:
        if gt_counts is not None:
            host_gt_counts(gt_counts, bboxes, who)                   # (raises: lists carry their own counts)
        bboxes = [b.to(dev, torch.float32) for b in bboxes]
        labels = ([torch.zeros(b.shape[:1], dtype=torch.int64, device=dev) for b in bboxes] if labels is None else
                  [lb.to(dev) for lb in labels])
        B, host = len(bboxes), tuple(b.shape[0] for b in bboxes)
    dtype = labels.dtype if isinstance(labels, torch.Tensor) else (labels[0].dtype if labels else torch.int64)
    pb, pl, gc = pack_ground_truth(bboxes, labels, B, dev, None if gt_counts is None else torch.tensor(host, dtype=torch.int32),
                                   who=who)
    return PackedGroundTruth(pb, pl.to(dtype), gc, host)


T2_INDEX_ERROR = ("index of a sampled negative is out of bounds for the kept labels "
                  "(the reference raises IndexError at nets/frcnn_training.py:175)")
Q5_TOO_FEW = ("ProposalTargetCreator kept {} samples for image {}, fewer than n_sample = {}: the reference's head fails on that "
              "(quirk Q5)")


def raise_for_counts(counts, n_sample=None):
    """A host copy of ProposalTargetCreator's count words - rows of (kept, positives, negatives, status), one per image - into
    the reference's exceptions, in image order: status 1 is the IndexError of quirk T2; with ``n_sample`` (the trainer), fewer
    kept rows than that is the RuntimeError of quirk Q5."""
    for i, (n_keep, _, _, status) in enumerate(counts):
        if status:
            raise IndexError(T2_INDEX_ERROR)
        if n_sample is not None and n_keep < n_sample:
            raise RuntimeError(Q5_TOO_FEW.format(n_keep, i, n_sample))


class AnchorTargetCreator:
    def __init__(self, n_sample=256, pos_iou_thresh=0.7, neg_iou_thresh=0.3, pos_ratio=0.5):
        _check_pos_ratio("AnchorTargetCreator", pos_ratio)
        self.n_sample = n_sample
        self.pos_iou_thresh = pos_iou_thresh
        self.neg_iou_thresh = neg_iou_thresh
        self.pos_ratio = pos_ratio

    def __call__(self, bbox, anchor):
        """bbox [G,4] ground truth, anchor [A,4] -> (loc [A,4], label [A]: 1 positive / 0 negative / -1 ignored).
        Four launches (row arg-max, column arg-max, labels + positive cap, offsets), no host synchronisation."""
        _check_pos_ratio("AnchorTargetCreator", self.pos_ratio)       # read here, not in __init__: it may have been reassigned
        require_cuda(anchor, "AnchorTargetCreator")
        loc, label, _ = hip_ops.anchor_targets(bbox, anchor, int(self.pos_ratio * self.n_sample), self.n_sample,
                                               self.pos_iou_thresh, self.neg_iou_thresh)
        return loc, label

    def batch(self, bboxes, anchor, gt_counts=None):
        """``__call__`` for every image of a batch at once: ``bboxes`` a list of [G_i,4] tensors, a padded [B,Gmax,4] tensor with
        ``gt_counts`` (host ints, validated against Gmax here), or a ``PackedGroundTruth`` -> (loc [B,A,4], label [B,A]).
        Image b's rows are bit for bit ``self(bboxes[b][:gt_counts[b]], anchor)``.  Four launches for the whole batch
        (tsod_anchor_targets_batch_f32), no host synchronisation."""
        _check_pos_ratio("AnchorTargetCreator", self.pos_ratio)
        require_cuda(anchor, "AnchorTargetCreator.batch")
        gt = bboxes if isinstance(bboxes, PackedGroundTruth) else pack_targets(bboxes, None, gt_counts, anchor.device,
                                                                               "AnchorTargetCreator.batch")
        loc, label, _ = hip_ops.anchor_targets_batch(gt.boxes, gt.counts, anchor, int(self.pos_ratio * self.n_sample),
                                                     self.n_sample, self.pos_iou_thresh, self.neg_iou_thresh)
        return loc, label


class ProposalTargetCreator(object):
    def __init__(self, n_sample=128, pos_ratio=0.5, pos_iou_thresh=0.5, neg_iou_thresh_high=0.5, neg_iou_thresh_low=0):
        _check_pos_ratio("ProposalTargetCreator", pos_ratio)
        self.n_sample = n_sample
        self.pos_ratio = pos_ratio
        self.pos_roi_per_image = int(self.n_sample * self.pos_ratio)
        self.pos_iou_thresh = pos_iou_thresh
        self.neg_iou_thresh_high = neg_iou_thresh_high
        self.neg_iou_thresh_low = neg_iou_thresh_low

    def _sample(self, fn, roi, bbox, label):
        """``fn`` = hip_ops.proposal_targets or proposal_targets_src -> its outputs cut to the S kept rows (counts dropped)."""
        require_cuda(roi, "ProposalTargetCreator")
        sample_roi, gt_roi_loc, gt_roi_label, counts, *src = fn(
            roi, bbox, label, self.n_sample, self.pos_roi_per_image, self.pos_iou_thresh, self.neg_iou_thresh_high,
            self.neg_iou_thresh_low)
        host = counts.tolist()
        raise_for_counts([host])
        n_keep = host[0]
        return (sample_roi[:n_keep], gt_roi_loc[:n_keep], gt_roi_label[:n_keep].to(label.dtype), *(t[:n_keep] for t in src))

    def __call__(self, roi, bbox, label, loc_normalize_std=(0.1, 0.1, 0.2, 0.2)):
        """roi [R,4], bbox [G,4], label [G] -> (sample_roi [S,4], gt_roi_loc [S,4], gt_roi_label [S]), S <= n_sample.
        ``loc_normalize_std`` is accepted and unused, as in the reference (the division is commented out there).
        Two launches; reading S (and the IndexError flag of the reference's quirk T2) is the one host synchronisation."""
        return self._sample(hip_ops.proposal_targets, roi, bbox, label)

    def with_sources(self, roi, bbox, label):
        """``__call__`` plus sample_src [S] int32: the row of cat(roi, bbox) each sample came from (the reference's keep_index;
        < len(roi): a proposal).  What FasterRCNNTrainer(head_grads=True) maps the regression target's gradient back with."""
        return self._sample(hip_ops.proposal_targets_src, roi, bbox, label)

    def batch(self, rois, bboxes, labels, gt_counts=None, with_sources=False):
        """``__call__`` / ``with_sources`` for every image of a batch at once, WITHOUT reading anything back: rois [B,R,4];
        ``bboxes`` / ``labels`` lists of [G_i,4] / [G_i] tensors, padded [B,Gmax,4] / [B,Gmax] tensors with ``gt_counts`` (host
        ints, validated against Gmax here), or ``bboxes`` a ``PackedGroundTruth`` (``labels`` is then ignored) ->
        (sample_roi [B,n_sample,4], gt_roi_loc [B,n_sample,4], gt_roi_label [B,n_sample], counts [B,4] int32 on the device,
        sample_src [B,n_sample] int32 or None).  The first counts[b,0] rows of image b are bit for bit what ``__call__`` returns
        for it; the rows behind them are zeros (-1 in sample_src).  Two launches for the whole batch
        (tsod_proposal_targets_batch_f32).  Reading ``counts`` - and raising what the reference raises, ``raise_for_counts`` on
        a host copy - stays with the caller: that is the point of this method."""
        require_cuda(rois, "ProposalTargetCreator.batch")
        gt = bboxes if isinstance(bboxes, PackedGroundTruth) else pack_targets(bboxes, labels, gt_counts, rois.device,
                                                                               "ProposalTargetCreator.batch")
        sample_roi, gt_roi_loc, gt_roi_label, counts, src = hip_ops.proposal_targets_batch(
            rois, gt.boxes, gt.labels, gt.counts, self.n_sample, self.pos_roi_per_image, self.pos_iou_thresh,
            self.neg_iou_thresh_high, self.neg_iou_thresh_low, want_src=with_sources)
        return sample_roi, gt_roi_loc, gt_roi_label.to(gt.labels.dtype), counts, src


HEAD_PARAMS = ("rpn.loc.weight", "rpn.loc.bias", "rpn.score.weight", "rpn.score.bias",
               "head.cls_loc.weight", "head.cls_loc.bias", "head.score.weight", "head.score.bias")


class _HeadLosses(torch.autograd.Function):
    """The five losses as one differentiable node whose backward is HIP kernels only (csrc/head_grads.hip, feature_grads.hip).

    forward(per [4], saved, features or None, *params) -> [rpn_loc, rpn_cls, roi_loc, roi_cls, total] (total summed in the
    order of the default path, so the values are identical).  backward: tsod_rpn_losses_grad_f32, tsod_roi_losses_grad_f32,
    tsod_rpn_roi_scatter_f32 (the indirect term through the proposals), then
      * with ``params`` (head_grads=True): tsod_wgrad_f32 for the RPN (feature map rows) and for the head (fc7 rows), each pair
        skipped when none of its four parameters requires grad.  It writes / adds the eight ``.grad`` tensors itself (the fused
        [56,C] / [408,C] results go straight into the reference's parameter shapes) and returns no gradient for them, so
        ``torch.autograd.grad`` on these parameters is not supported - ``.backward()`` is;
      * with ``features`` (the caller's feature map, requiring grad): d feat = d rpn_out . W_rpn (1x1 f32 GEMM) + the backward
        of the head's pooling of d fc7 = d both . W_head (tsod_roi_pool_avg_grad_f32 / tsod_roi_align_avg_grad_f32, adding in
        place), one NHWC -> NCHW pass, returned to autograd as d features."""

    @staticmethod
    def forward(ctx, per, saved, features, *params):
        ctx.saved = saved
        ctx.params = params
        return torch.cat([per, (per[0] + per[1] + per[2] + per[3]).view(1)])

    @staticmethod
    def backward(ctx, g):
        sv, params = ctx.saved, ctx.params
        up = g.contiguous()
        d_rpn, _ = hip_ops.rpn_losses_grad(sv["rpn_out"], sv["A"], sv["gt_loc"], sv["gt_label"], sv["rpn_sigma"], up, sv["inv_B"])
        d_both, d_roi = hip_ops.roi_losses_grad(sv["both"], sv["n_class"], sv["sample_roi"], sv["gt_roi_loc"], sv["gt_roi_label"],
                                                sv["roi_sigma"], up, sv["inv_B"])
        hip_ops.rpn_roi_scatter(d_rpn, d_roi, sv["sample_src"], sv["keep_idx"], sv["sort_idx"], sv["rpn_out"], sv["anchor"],
                                sv["A"], sv["clamp_x"], sv["clamp_y"])
        feat = sv["feat"]
        if params:
            if any(p.requires_grad for p in params[0:4]):
                _wgrad_into(d_rpn, feat.view(-1, feat.shape[-1])[:, :params[0].shape[1]], params[0:4])   # (pixel rows may be padded)
            if any(p.requires_grad for p in params[4:8]):
                _wgrad_into(d_both, sv["fc7"], params[4:8])
        d_features = None
        if ctx.needs_input_grad[2]:
            n, h, w = feat.shape[:3]
            d_feat = sv["rpn"].input_grad(d_rpn, n, h, w, wt=sv["rpn_wt"])                     # [n,h,w,C] NHWC
            d_fc7 = sv["head"].fc7_grad(d_both, wt=sv["head_wt"])
            sv["head"].pooled_grad(feat, sv["sample_roi"], sv["roi_indices"], sv["head_size"], d_fc7, d_feat=d_feat,
                                   accumulate=True)
            d_features = hip_ops.nhwc_to_nchw(d_feat)
        return (None, None, d_features) + (None,) * len(params)


def _wgrad_into(dy, x, params):
    """One tsod_wgrad_f32 launch pair into (w0, b0, w1, b1).grad: written when none of them has a gradient yet, added to
    otherwise (a missing one starts from zeros); a parameter that does not require grad gets a scratch destination."""
    have = [p.requires_grad and p.grad is not None for p in params]
    accumulate = any(have)
    dst = []
    for p, h in zip(params, have):
        if not p.requires_grad:
            dst.append(torch.empty_like(p))
        elif not h:
            p.grad = torch.zeros_like(p) if accumulate else torch.empty_like(p)
            dst.append(p.grad)
        else:
            dst.append(p.grad)
    K = x.shape[1]
    hip_ops.wgrad(dy, x, dst[0].view(-1, K), dst[1], dst[2].view(-1, K), dst[3], accumulate=accumulate)


class FasterRCNNTrainer(nn.Module):
    """The reference's ground-truth-conditioned forward (nets/frcnn_training.py:179-342) with its four losses.

    ``FasterRCNNTrainer(mode, num_classes, feat_stride=16, anchor_scales=[8,16,32], ratios=[0.5,1,2])`` as in the reference,
    plus the keyword-only ``backbone`` / ``roi_op`` of ``FasterRCNN`` and ``head_img_size``.  The attribute names are the
    reference's (``feat_extra``, ``classifier``, ``rpn``, ``head``, ...), so its ``state_dict`` has the reference's key set
    and shapes and a checkpoint of train/train.py loads with ``load_state_dict(ckpt['model_state_dict'], strict=True)``.

    ``head_grads=True`` (keyword-only) makes the five losses differentiable w.r.t. the eight head parameters (rpn.loc,
    rpn.score, head.cls_loc, head.score: weight and bias) while grad mode is on: any scalar combination of them can call
    ``.backward()`` (train/train.py's ``losses[-1] / 32``), and the backward - HIP kernels only -
    adds into those ``.grad`` tensors what the reference's autograd puts there with the backbone frozen, including the
    indirect term of the RoI regression loss through the (not detached) proposals.  The backbone must be frozen
    (``feat_extra.requires_grad_(False)``): no gradient reaches it.  The autograd node keeps its own copies of what its
    backward reads, so a backward issued after a later forward still gives its own forward's gradients.  The default
    (``head_grads=False``) returns losses that do not require grad.

    ``forward(..., features=f)`` (keyword-only): ``f`` [B, C, h, w] float32 on the GPU (any strides, any autograd history; C =
    the RPN's in_channels) is the feature map instead of ``feat_extra(imgs)``; ``imgs`` is then used for its shape only
    (img_size, B).  When grad mode is on and ``f.requires_grad``, the losses are differentiable w.r.t. ``f``: the node returns
    d f through autograd (``loss.backward()`` or ``torch.autograd.grad(loss, f)``) - the RPN's input GEMM, the head's input
    GEMM and the RoIPool / RoIAlign + mean backward on HIP, whatever ``head_grads`` is.  No gradient
    flows through the RoI coordinates into the pooling (as in torchvision); the frozen-backbone check does not apply.

    ``forward(imgs, bboxes, labels, scale=1)`` -> (losses, anchors_pred [B,S,4], classes_pred [B,S] int64,
    classes_score_pred [B,S], bboxes[0][None], (labels[0] + 1)[None]) with losses = [rpn_loc, rpn_cls, roi_loc, roi_cls,
    their sum]: zero-dimensional tensors, each summed over the images and divided by their number (:333-342).
    ``imgs``: [B,3,H,W] on the GPU or a list of [3,H,W]; ``bboxes`` / ``labels``: lists (or batched tensors) of [G,4] / [G].

    The stages are the detector's own NHWC entry points, composed as ``FasterRCNN.forward`` composes them: the backbone
    plan, ``rpn.propose`` (train numbers with mode="train": 12000 -> 600), the two target creators' ``batch`` - six launches
    for all B images on ground truth packed once -, the head's fused GEMM on the [B, n_sample]
    samples, then tsod_rpn_losses_f32 (reads the fused RPN output in place) and tsod_roi_losses_f32.  The host reads once per
    forward, after the last launch: the creators' count words and the two loss kernels' status words in one transfer, from
    which it raises what the reference raises - per image the IndexError of quirk T2, then the RuntimeError of quirk Q5, then
    the losses' IndexError.  A creator that has been replaced by a plain callable (no ``batch``) puts the forward on the
    per-image route: each image through both creators, one host synchronisation per image.

    ``forward(..., gt_counts=c)`` (keyword-only): ``bboxes`` / ``labels`` are padded tensors [B,Gmax,4] / [B,Gmax] as a collate
    function makes them and ``c`` (a sequence of ints or a CPU integer tensor, each in [0, Gmax]: ValueError otherwise, before
    any launch) says how many rows of each image count; the rows behind them are never read.  The last two return values are
    then cut to ``c[0]`` rows.

    Decisions (DESIGN.md "The trainer's forward"):
      * img_size: the reference hands imgs.shape[1:] = (C,H,W) to the RPN (quirk Q1) AND to the head (:252, quirk Q2 -
        the head then divides y by C = 3); a checkpoint of the reference learned its head that way, so that is the default.
        ``head_img_size="hw"`` hands the head (H,W), as ``FasterRCNN.forward`` does.
      * batch: the reference runs imgs[0] only and fails for more than one image; here every image runs against its own
        ground truth and the losses are averaged over B.  B = 1 is the reference's computation.
      * fewer than n_sample samples from ProposalTargetCreator (the reference's head fails there, quirk Q5): RuntimeError.
      * the module must be in eval() (BatchNorm folded), like the rest of the HIP path.
      * an IndexError of the proposal padding (quirk Q4) is recorded on the device as in ``FasterRCNN``: ``raise_if_error()``.

      * in-place updates of the eight head parameters (an optimizer step) are detected through their ``_version`` and the
        RPN's and head's packed weight images are rebuilt before the next forward.

    ``backbone_grads="tail"`` (keyword-only, HarDNet backbones; default None = everything above): with ``features=None`` and
    grad mode on, ``forward`` switches ``feat_extra.train_tail`` on, takes the feature map with the tail's autograd node and
    continues on the ``features=`` path, so ``losses[-1].backward()`` also fills ``.grad`` of the six tail tensors
    (``feat_extra.tail_parameters()``: the two depthwise 3x3 stride-2 convs and the grouped 1x1 the reference adds on top of
    HarDNet, which no pretrained checkpoint holds) - the backward of tsod_gconv1x1_pair_f32 and tsod_dwconv3x3_f32 on HIP
    (DESIGN.md section 4.17).  The frozen-backbone check then applies to every backbone parameter except those six.

    ``backbone_grads=n`` (an int >= 1, at most the backbone's HarDBlocks): the same with ``feat_extra.train_blocks(n)`` - the
    tail plus the last ``n`` HarDBlocks, their transition layers and the ``DWConvLayer``s between them
    (``feat_extra.trainable_parameters()``, BN ``weight`` / ``bias`` included).  BatchNorm stays in eval
    mode and the stem is never reached.

    ``backbone_grads="full"``: the same with ``feat_extra.train_full()`` - every parameter of the backbone, the stem
    (``base.0`` - ``base.2``) included; the frozen-backbone check has nothing left to refuse.

    ``bn_batch_stats=True`` (keyword-only, with ``backbone_grads`` an int or "full"): the reference's ``model.train()``
    contract for the trainable section - ``forward`` is then allowed under ``.train()``, the mode is set with
    ``batch_stats=True`` and every BatchNorm the mode reaches normalises with the statistics of the batch, backpropagates
    through them and moves its running statistics (``HarDNetFeatureExtraction.set_train_mode``); the
    frozen section below stays folded.  Under ``.eval()`` nothing changes.

    ``dropout=True`` (keyword-only, needs ``bn_batch_stats=True``: ValueError otherwise): the mode is set with ``dropout=True``
    too, so the ``nn.Dropout`` of the trainable section (HarDNet-85: p = 0.1 in front of the last transition layer) is active
    under ``.train()`` - a Philox mask on HIP with one host-drawn key per forward (DESIGN.md section 4.26;
    ``feat_extra.last_dropout_key``, ``feat_extra.dropout_generator``).  Without it dropout stays the identity, as on every
    other path; backbones without an ``nn.Dropout`` in the section run exactly as with ``dropout=False``.

    ``backbone_grads="layer4" | "layer3" | "layer2"`` (ResNet backbones that offer the stage: ``feat_extra.trainable_stages``,
    resnet50 / resnet101): the same with ``feat_extra.train_from(stage)`` - every Bottleneck from the first block of that stage to
    the end of ``layer4``, projection blocks included (33 / 96 / 139 tensors for resnet50).  BatchNorm
    stays folded: ``bn_batch_stats=True`` raises ValueError with them, and ints, "tail" and "full" keep raising for ResNet
    backbones.  ``backbone_grads="stem"`` (where ``feat_extra.trainable_sections`` offers it: resnet50 / resnet101): the same with
    ``feat_extra.train_from("stem")`` - the whole backbone, ``conv1`` / ``bn1`` / ``relu`` and ``layer1`` included (DESIGN.md section
    4.23; 176 tensors for resnet50); that forward runs the stem and ``layer1`` as per-layer launches.  The identity Bottlenecks at the end of ``layer4`` alone (``layer4.1``, ``layer4.2``) train through the
    ``features=`` path, whose map may carry any autograd history - here the backbone's own node (``ResNet.train_blocks``,
    DESIGN.md section 4.21):

        tr = FasterRCNNTrainer("train", nc, backbone="resnet50", head_grads=True).eval()
        tr.feat_extra.requires_grad_(False); tr.feat_extra.train_blocks(2)
        for p in tr.feat_extra.trainable_parameters(): p.requires_grad_(True)
        losses = tr(x, bboxes, labels, features=tr.feat_extra(x))[0]; (losses[-1] / 32).backward()

    Train-mode BatchNorm for a ResNet section reaches the trainer through the same path - the keyword
    ``bn_batch_stats`` keeps its refusal for ResNet backbones; the trainer stays in ``.eval()``, the backbone alone goes to
    ``.train()``:

        tr = FasterRCNNTrainer("train", nc, backbone="resnet50", head_grads=True).eval()
        tr.feat_extra.requires_grad_(False); tr.feat_extra.train_from("layer4", batch_stats=True).train()
        for p in tr.feat_extra.trainable_parameters(): p.requires_grad_(True)
        losses = tr(x, bboxes, labels, features=tr.feat_extra(x))[0]; (losses[-1] / 32).backward()

    Not provided: the rest of the ResNet backbones' backward - BasicBlock,
    ResNeXt's grouped 3x3 (``head_grads`` fine-tunes the heads
    on a frozen backbone, ``backbone_grads="tail"`` adds the backbone's tail, an int its last HarDBlocks, ``"full"`` the whole
    HarDNet; ``features=`` trains a
    backbone that has autograd of its own); gradients w.r.t. RoI coordinates; graph capture (the forward's one host read
    is what is left in its way) and tuning (the forward runs whatever plan the backbone holds).  ``eval_fn`` / ``calculate_metrics``: see there."""

    def __init__(self, mode, num_classes, feat_stride=16, anchor_scales=[8, 16, 32], ratios=[0.5, 1, 2], *,
                 backbone="hardnet39", roi_op="pool", head_img_size="chw", head_grads=False, backbone_grads=None,
                 bn_batch_stats=False, dropout=False):
        super().__init__()
        if head_img_size not in ("chw", "hw"):
            raise ValueError(f"head_img_size must be 'chw' (the reference's) or 'hw', got {head_img_size!r}")
        n_blocks = backbone_grads if isinstance(backbone_grads, int) and not isinstance(backbone_grads, bool) else None
        hardnet = str(backbone).startswith("hardnet")
        # a ResNet stage name ("layer4" ...): checked against the backbone's trainable_stages once it is built
        stage = backbone_grads if isinstance(backbone_grads, str) and backbone_grads not in ("tail", "full") and not hardnet else None
        if stage is None and backbone_grads not in (None, "tail", "full") and (n_blocks is None or n_blocks < 1):
            raise ValueError(f"backbone_grads must be None, 'tail', 'full' or a number of HarDBlocks >= 1, got {backbone_grads!r}")
        if stage is None and backbone_grads is not None and not hardnet:
            raise ValueError(f"backbone_grads={backbone_grads!r} trains the HarDNet tail (the last four modules of "
                             f"feat_extra.base) and the HarDBlocks before it; backbone {backbone!r} has none (a ResNet backbone "
                             "takes a stage name of feat_extra.trainable_stages)")
        if stage is not None and bn_batch_stats:
            raise ValueError(f"bn_batch_stats=True: backbone {backbone!r} trains with BatchNorm folded only (backbone_grads={stage!r})")
        self.feat_extra, feat_ch, native_stride = _make_extractor(backbone)
        if stage is not None and stage not in getattr(self.feat_extra, "trainable_sections", ()):
            raise ValueError(f"backbone_grads={stage!r}: backbone {backbone!r} offers the stages "
                             f"{getattr(self.feat_extra, 'trainable_stages', ())} (feat_extra.trainable_stages; with \"stem\": "
                             f"{getattr(self.feat_extra, 'trainable_sections', ())}, feat_extra.trainable_sections)")
        if n_blocks is not None and n_blocks > self.feat_extra.n_blocks:
            raise ValueError(f"backbone_grads={n_blocks}: backbone {backbone!r} has {self.feat_extra.n_blocks} HarDBlocks")
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
        self.head_grads = bool(head_grads)
        self.backbone_grads = backbone_grads
        if bn_batch_stats and backbone_grads in (None, "tail"):
            raise ValueError("bn_batch_stats=True needs backbone_grads = a number of HarDBlocks or 'full' (the tail has no "
                             f"BatchNorm), got backbone_grads={backbone_grads!r}")
        self.bn_batch_stats = bool(bn_batch_stats)
        if dropout and not self.bn_batch_stats:
            raise ValueError("dropout=True needs bn_batch_stats=True: only the batch-statistics variant runs under .train()")
        self.dropout = bool(dropout)
        self.__dict__["_uid"] = next(_UID)          # scratch ownership, as FasterRCNN's
        self.__dict__["_head_versions"] = None

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__["_uid"] = next(_UID)
        self.__dict__["_head_versions"] = None

    def _head_params(self):
        named = dict(self.named_parameters())
        return [named[k] for k in HEAD_PARAMS]

    def _refresh_packs(self):
        """Rebuild the RPN's and head's packed weights when one of the eight head parameters changed in place since they
        were packed (``_version`` moves on every in-place update: ``optimizer.step()``, ``p.data.mul_()`` ...)."""
        versions = tuple(p._version for p in self._head_params())
        if self._head_versions is not None and versions != self._head_versions:
            self.rpn.invalidate_packed()
            self.head.invalidate_packed()
        self.__dict__["_head_versions"] = versions

    def raise_if_error(self):
        """Surface the deferred IndexError of the proposal padding and a range violation of the fp16x2 conv arithmetic."""
        self.rpn.raise_if_error()
        self.feat_extra.raise_if_error()

    def _check_features(self, features, B):
        if not isinstance(features, torch.Tensor):
            raise TypeError(f"FasterRCNNTrainer.forward: features must be a tensor, got {type(features).__name__}")
        if features.dtype != torch.float32:
            raise TypeError(f"FasterRCNNTrainer.forward: features must be float32, got {features.dtype}")
        require_cuda(features, "FasterRCNNTrainer.forward(features=)")
        C = self.rpn.score.in_channels
        if features.dim() != 4 or features.shape[0] != B or features.shape[1] != C:
            raise ValueError(f"FasterRCNNTrainer.forward: features must be [B={B}, C={C}, h, w] (the RPN's in_channels), got "
                             f"{tuple(features.shape)}")

    def _targets(self, bboxes, labels, gt_counts, anchor, rois, dev, want_src):
        """Both target assignments of one forward -> (gt_loc [B,A,4], gt_label [B,A], sample_roi [B,n,4], gt_roi_loc [B,n,4],
        gt_roi_label [B,n], sample_src [B,n] or None, counts [B,4] on the device or None).

        When both creators offer ``batch`` the ground truth is packed once and each creator is called once for the whole batch:
        six launches, nothing read back - ``counts`` is returned for the forward's one host read.  Otherwise (a creator replaced
        by a plain callable) every image goes through the creators on its own, the host synchronising once per image where
        ProposalTargetCreator does, and the exceptions are raised here; ``counts`` is then None."""
        B, n_sample = len(bboxes), self.proposal_target_creator.n_sample
        a_batch = getattr(self.anchor_target_creator, "batch", None)
        p_batch = getattr(self.proposal_target_creator, "batch", None)
        if a_batch is not None and p_batch is not None:
            gt = pack_targets(bboxes, labels, gt_counts, dev, "FasterRCNNTrainer.forward")
            gt_loc_all, gt_label_all = a_batch(gt, anchor)
            s_roi, s_loc, s_label, counts, s_src = p_batch(rois, gt, None, with_sources=want_src)
            return gt_loc_all, gt_label_all, s_roi, s_loc, s_label, s_src, counts
        gt_locs, gt_labels, s_rois, s_locs, s_labels, s_srcs = [], [], [], [], [], []
        for i in range(B):
            g = bboxes[i].shape[0] if gt_counts is None else int(gt_counts[i])
            bbox = bboxes[i][:g].to(dev, torch.float32)
            label = labels[i][:g].to(dev)
            gt_loc, gt_label = self.anchor_target_creator(bbox, anchor)
            gt_locs.append(gt_loc)
            gt_labels.append(gt_label)
            if want_src:
                s_roi, s_loc, s_label, s_src = self.proposal_target_creator.with_sources(rois[i], bbox, label)
                s_srcs.append(s_src)
            else:
                s_roi, s_loc, s_label = self.proposal_target_creator(rois[i], bbox, label, self.loc_normalize_std)
            if s_roi.shape[0] < n_sample:
                raise RuntimeError(Q5_TOO_FEW.format(s_roi.shape[0], i, n_sample))
            s_rois.append(s_roi)
            s_locs.append(s_loc)
            s_labels.append(s_label)
        return (torch.stack(gt_locs), torch.stack(gt_labels), torch.stack(s_rois), torch.stack(s_locs), torch.stack(s_labels),
                torch.stack(s_srcs) if want_src else None, None)

    def forward(self, imgs, bboxes, labels, scale=1, *, features=None, gt_counts=None):
        if self.training and not self.bn_batch_stats:
            raise TsodError("the HIP path implements the inference forward only: call .eval() first")
        if features is None:
            x = torch.stack(list(imgs)) if isinstance(imgs, (list, tuple)) else imgs
            require_cuda(x, "FasterRCNNTrainer.forward")
            shape, dev = tuple(x.shape), x.device
        else:                                                            # imgs: only its shape is used
            shape = ((len(imgs),) + tuple(imgs[0].shape)) if isinstance(imgs, (list, tuple)) else tuple(imgs.shape)
            self._check_features(features, shape[0])
            dev = features.device
        B = shape[0]
        if len(bboxes) != B or len(labels) != B:
            raise ValueError(f"FasterRCNNTrainer.forward: {B} images, {len(bboxes)} box sets, {len(labels)} label sets")
        if gt_counts is not None:                                        # on the host, before anything is launched
            gt_counts = host_gt_counts(gt_counts, bboxes, "FasterRCNNTrainer.forward")
        img_size = shape[1:]                                             # (C,H,W): quirk Q1 (RPN), Q2 (head)
        head_size = img_size if self.head_img_size == "chw" else shape[2:]
        n_sample = self.proposal_target_creator.n_sample
        grads = self.head_grads and torch.is_grad_enabled()
        tail = self.backbone_grads is not None and features is None and torch.is_grad_enabled()
        if tail or (grads and features is None):                         # what the mode does not reach must be frozen
            stage = isinstance(self.backbone_grads, str) and self.backbone_grads not in ("tail", "full")       # a ResNet stage
            mode_args = (self.backbone_grads,) if stage else (self.backbone_grads, self.bn_batch_stats, self.dropout)
            ours = {id(p) for p in self.feat_extra.set_train_mode(*mode_args).trainable_parameters()} if tail else ()
            frozen = [k for k, p in self.feat_extra.named_parameters() if p.requires_grad and id(p) not in ours]
            if frozen:
                why = ("(head_grads=True) computes the head parameters' gradients on a frozen backbone, but" if not tail else
                       "(backbone_grads='tail') reaches the six tail tensors of the backbone only (feat_extra.tail_parameters()); "
                       "every other backbone parameter must be frozen, but" if self.backbone_grads == "tail" else
                       "(backbone_grads='stem') reaches the backbone's section \"stem\" only: conv1, bn1, relu and the blocks of layer1 "
                       "to layer4 (feat_extra.trainable_parameters()); every other backbone parameter must be frozen, but"
                       if self.backbone_grads == "stem" else
                       f"(backbone_grads={self.backbone_grads!r}) reaches the backbone's blocks from {self.backbone_grads}.0 to the end "
                       "of layer4 only (feat_extra.trainable_parameters()); every other backbone parameter must be frozen, but"
                       if stage else
                       f"(backbone_grads={self.backbone_grads}) reaches the backbone's tail and last {self.backbone_grads} HarDBlocks "
                       "only (feat_extra.trainable_parameters()); every other backbone parameter must be frozen, but")
                raise TsodError(f"FasterRCNNTrainer{why} feat_extra.{frozen[0]} (and {len(frozen) - 1} more) requires grad"
                                + ("" if tail else ": call trainer.feat_extra.requires_grad_(False)"))
        self._refresh_packs()
        if tail:                     # the map with the backbone's autograd node; from here on the features= path
            features = self.feat_extra(x)
        feat_grad = features is not None and torch.is_grad_enabled() and features.requires_grad
        with hip_ops.ARENA.scope((self._uid, 0)):
            if features is None:
                feat = self.feat_extra.forward_nhwc(x, 0)
                plan = self.feat_extra._plan_for(x, 0)
                feat_amax, flag = (getattr(plan, "output_amax", 0) or None), getattr(plan, "range_flag", None)
            else:                    # the caller's map, once to NHWC (an fp16x2 GEMM choice scales it by a tsod_absmax_f32 pass)
                feat = hip_ops.nchw_to_nhwc(features.detach())
                feat_amax, flag = None, None
            proposed = self.rpn.propose(feat, img_size, scale, want_anchors=True, feat_amax=feat_amax, range_flag=flag,
                                        want_index=grads or feat_grad)
            rpn_out, rois, anchor = proposed[:3]
            (gt_loc_all, gt_label_all, sample_rois, s_locs_all, s_labels_all, sample_src, counts) = self._targets(
                bboxes, labels, gt_counts, anchor, rois, dev, grads or feat_grad)
            rpn_loss, rpn_status = hip_ops.rpn_losses(rpn_out, self.rpn.anchor_base.shape[0], gt_loc_all, gt_label_all,
                                                      self.rpn_sigma)
            roi_indices = torch.arange(B, dtype=torch.int32, device=dev)
            fc7, both, n_loc, n_sc = self.head.forward_fused(feat, sample_rois, roi_indices, head_size, feat_amax=feat_amax,
                                                             range_flag=flag)
            roi_cls_locs, roi_scores = both[:, :n_loc].view(B, -1, n_loc), both[:, n_loc:n_loc + n_sc].view(B, -1, n_sc)
            anchors_pred, classes_pred, classes_score_pred, roi_loss, roi_status = hip_ops.roi_losses(
                roi_cls_locs, roi_scores, sample_rois, s_locs_all, s_labels_all, self.roi_sigma)
            if grads or feat_grad:
                saved = dict(feat=feat.clone() if features is None else feat,   # (the plan's buffer: the next forward
                             rpn_out=rpn_out, anchor=anchor, sort_idx=proposed[3], keep_idx=proposed[4],  # overwrites it)
                             gt_loc=gt_loc_all, gt_label=gt_label_all, sample_roi=sample_rois, gt_roi_loc=s_locs_all,
                             gt_roi_label=s_labels_all, sample_src=sample_src, fc7=fc7, both=both,
                             A=self.rpn.anchor_base.shape[0], n_class=n_sc, rpn_sigma=self.rpn_sigma,
                             roi_sigma=self.roi_sigma, inv_B=1.0 / B, clamp_x=img_size[1], clamp_y=img_size[2])
                if feat_grad:
                    saved.update(rpn=self.rpn, head=self.head, rpn_wt=self.rpn._dgrad_weight(dev),
                                 head_wt=self.head._dgrad_weight(dev), roi_indices=roi_indices, head_size=head_size)
            if features is None:
                self.feat_extra.publish_range_word(plan)
        # the one host read of the forward, after the last launch: the creators' count words (batched route) and the two loss
        # kernels' status words together; the reference raises per image in the creator, then IndexError in the losses
        if counts is None:
            bad = int(rpn_status.sum() + roi_status.sum())
        else:
            host = torch.cat([counts.view(-1), rpn_status, roi_status]).tolist()
            raise_for_counts([host[4 * i:4 * i + 4] for i in range(B)], n_sample)
            bad = sum(host[4 * B:])
        if bad:
            raise IndexError("a target class index is out of bounds for the logits it indexes "
                             "(the reference raises IndexError at nets/frcnn_training.py:274 / 313-331)")
        per = torch.cat([rpn_loss, roi_loss], dim=1).sum(0) / B        # [rpn_loc, rpn_cls, roi_loc, roi_cls]
        if grads or feat_grad:
            params = self._head_params() if grads else ()
            losses = list(_HeadLosses.apply(per, saved, features if feat_grad else None, *params).unbind(0))
        else:
            losses = list(per.unbind(0))
            losses = losses + [sum(losses)]
        g0 = bboxes[0].shape[0] if gt_counts is None else int(gt_counts[0])    # (a host value: the cut costs no synchronisation)
        return (losses, anchors_pred, classes_pred, classes_score_pred, torch.unsqueeze(bboxes[0][:g0], dim=0),
                torch.unsqueeze(labels[0][:g0] + 1, dim=0))

    # ------------------------------------------------------------------------------------------------------- evaluation
    def _records(self, anchors_pred, classes_pred, classes_score_pred, nms_iou_threshold):
        """The head's per-RoI predictions as [B,S,6] detection rows, through the reference's per-class NMS
        (``hip_ops.filter_detections(per_class=True)``, class 0 = background dropped) -> (det_sorted, keep, n_kept)."""
        det = torch.cat([anchors_pred.float(), classes_score_pred.float().unsqueeze(-1), classes_pred.float().unsqueeze(-1)],
                        dim=-1)
        return hip_ops.filter_detections(det, iou_thr=nms_iou_threshold, per_class=True, background_class=0)

    def eval_fn(self, eval_dataloader, scale=1, nms_iou_threshold=0.7, map_iou_threshold=0.7):
        """The reference's evaluation leg (nets/frcnn_training.py:347-369, called by train/train.py under
        ``torch.inference_mode()``) -> (avg_eval_loss, avg_mAP).

        Every batch ``(imgs, bboxes, labels)`` (CPU batches of a reference-style DataLoader are moved to the module's device)
        runs through ``forward``; its (anchors_pred, classes_score_pred, classes_pred) rows go through the reference's
        per-class NMS at ``nms_iou_threshold`` and into one ``DetectionEvaluator(n_classes + 1, (map_iou_threshold,),
        ignore_class=0)`` against each image's own ``labels + 1``.  avg_eval_loss = the mean over batches of ``losses[-1]``
        (summed on the device, read once); avg_mAP = the evaluator's dataset-level mAP (NaN when no image has ground truth).
        Both are 0 for an empty loader, as in the reference.

        Deviations from the reference: the metric is one-to-one COCO matching, not "any GT with
        IoU > t"; classes without ground truth are excluded, not counted as 0; the mAP is over the whole loader, not a mean
        of per-batch values; every image is scored against its own ground truth, not ``bboxes[0]``.  The predictions come
        from the ground-truth-conditioned samples of ``forward`` (the reference's design), so the score sees the ground truth
        it is measured against: ``FasterRCNN.predict`` + ``DetectionEvaluator`` is the honest score of a detector."""
        ev = DetectionEvaluator(self.n_classes + 1, iou_thresholds=(map_iou_threshold,), ignore_class=0)
        loss = self._evaluate(ev, eval_dataloader, scale, nms_iou_threshold)
        if loss is None:
            return 0, 0
        return loss, ev.compute()["mAP"]

    def _evaluate(self, ev, eval_dataloader, scale, nms_iou_threshold, per_gt=False):
        """The evaluation loop of ``eval_fn`` / ``eval_coco``: every batch through ``forward`` and ``_records`` into ``ev`` ->
        the mean over batches of ``losses[-1]`` (summed on the device, read once), None for an empty loader.  ``per_gt``: a
        batch may carry per-image crowd flags and areas as a fourth and fifth element, passed to ``ev.update``."""
        self.eval()
        dev = next(self.parameters()).device
        loss_total, batches = None, 0
        for imgs, bboxes, labels, *extra in eval_dataloader:
            if len(extra) > (2 if per_gt else 0):
                raise ValueError(f"a batch of {3 + len(extra)} elements: (imgs, bboxes, labels"
                                 + ("[, crowd[, area]])" if per_gt else ")") + " expected")
            imgs = [im.to(dev) for im in imgs] if isinstance(imgs, (list, tuple)) else imgs.to(dev)
            bboxes = [bb.to(dev, torch.float32) for bb in bboxes]
            labels = [lb.to(dev) for lb in labels]
            kw = {}
            if len(extra) > 0 and extra[0] is not None:
                kw["gt_crowd"] = [c.to(dev) for c in extra[0]]
            if len(extra) > 1 and extra[1] is not None:
                kw["gt_area"] = [a.to(dev, torch.float32) for a in extra[1]]
            losses, anchors_pred, classes_pred, classes_score_pred = self.forward(imgs, bboxes, labels, scale)[:4]
            loss = losses[-1].detach()
            loss_total = loss if loss_total is None else loss_total + loss
            det_sorted, keep, n_kept = self._records(anchors_pred, classes_pred, classes_score_pred, nms_iou_threshold)
            ev.update(det_sorted, bboxes, [lb.to(torch.int64) + 1 for lb in labels], keep=keep, n_kept=n_kept, **kw)
            batches += 1
        return float(loss_total) / batches if batches else None

    def eval_coco(self, eval_dataloader, scale=1, nms_iou_threshold=0.7):
        """``eval_fn``'s loop run once for the whole COCO table -> (avg_eval_loss, stats).

        Every batch runs through ``forward`` and the reference's per-class NMS exactly as in ``eval_fn``; the rows go into one
        ``COCOEvaluator(n_classes + 1, ignore_class=0)``: COCO's ten thresholds, four area ranges and
        caps (1, 10, 100) at once, where the reference's training loop calls ``eval_fn`` once per threshold.  A batch is
        ``(imgs, bboxes, labels)``, or carries per-image ``crowd`` flags as a fourth and ``area`` values as a fifth element
        (lists of [G_i] tensors).  ``stats`` is ``COCOEvaluator.compute()``'s dict; (0, {}) for an empty loader.  What
        ``eval_fn`` says about predictions conditioned on the ground truth holds here too."""
        ev = COCOEvaluator(self.n_classes + 1, ignore_class=0)
        loss = self._evaluate(ev, eval_dataloader, scale, nms_iou_threshold, per_gt=True)
        if loss is None:
            return 0, {}
        return loss, ev.compute()

    def calculate_metrics(self, anchors_pred, classes_pred, classes_score_pred, anchors_gt, classes_gt,
                          nms_iou_threshold: float = 0.7, map_iou_threshold: float = 0.7):
        """One batch at one threshold, in the layout of the ``results`` dict the reference builds
        (nets/frcnn_training.py:372-565): ``{'mAP': float, 'class_metrics': {c: {'AP', 'Recall', 'Precision', 'TP', 'FP',
        'FN'}}}`` for c = 1..n_classes.  anchors_pred [B,S,4], classes_pred [B,S], classes_score_pred [B,S]; anchors_gt
        [B,G,4], classes_gt [B,G] (already + 1; pad with -1).  CPU inputs are moved to the module's device.  The metric is
        ``DetectionEvaluator``'s (``eval_fn`` lists how it deviates from the reference); a class without ground truth has
        AP and Recall -1 and does not enter the mAP; Precision = TP / (TP + FP) (0 without detections)."""
        dev = next(self.parameters()).device
        anchors_pred, classes_pred, classes_score_pred = (t.to(dev) for t in (anchors_pred, classes_pred, classes_score_pred))
        ev = DetectionEvaluator(self.n_classes + 1, iou_thresholds=(map_iou_threshold,), ignore_class=0)
        det_sorted, keep, n_kept = self._records(anchors_pred, classes_pred, classes_score_pred, nms_iou_threshold)
        ev.update(det_sorted, anchors_gt.to(dev, torch.float32), classes_gt.to(dev, torch.int64), keep=keep, n_kept=n_kept)
        r = ev.compute()
        results = {"mAP": r["mAP"], "class_metrics": {}}
        for c in range(1, self.n_classes + 1):
            tp, fp, fn = int(r["TP"][c, 0]), int(r["FP"][c, 0]), int(r["FN"][c, 0])
            results["class_metrics"][c] = {"AP": float(r["AP"][c, 0]), "Recall": float(r["recall"][c, 0]),
                                           "Precision": tp / (tp + fp) if tp + fp > 0 else 0.0, "TP": tp, "FP": fp, "FN": fn}
        return results
