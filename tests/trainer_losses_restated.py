"""The float64 torch statement of FasterRCNNTrainer's four losses (nets/frcnn_training.py:220-238, 262-274, 300-331) with
``sigma`` as a parameter, their gradients by autograd in the batch semantics the kernels document, and the seeded case
generators of tests/test_trainer_loss_sweep.py.

Batch semantics (include/tsod.h): per-image means; loss k of every image is weighted by (up[k] + up[4]) * inv_B, the f32 values
the kernel receives taken to f64; an image without a positive / without a counted row has a NaN loss and gives zero gradient
from that term.  Every reference takes the kernel's own f32 inputs to f64 and never rounds in between.
"""
import math

import torch
import torch.nn.functional as F

F32_EPS = torch.finfo(torch.float32).eps
SIGMAS = (1.0, 3.0, 0.5)                              # all exact in f32; so are their squares


# ------------------------------------------------------------------------------------------- the reference's arithmetic
def loc_loss(pred, gt, label, sigma=1.0):
    """_fast_rcnn_loc_loss (nets/frcnn_training.py:220-238)."""
    pos = label > 0
    d = (gt[pos] - pred[pos]).abs()
    s2 = sigma ** 2
    return torch.where(d < 1. / s2, 0.5 * s2 * d ** 2, d - 0.5 / s2).sum() / d.numel()


def loc2bbox(src, loc):
    w, h = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    cx, cy = src[:, 0] + 0.5 * w, src[:, 1] + 0.5 * h
    ncx, ncy = loc[:, 0] * w + cx, loc[:, 1] * h + cy
    nw, nh = torch.exp(loc[:, 2]) * w, torch.exp(loc[:, 3]) * h
    return torch.stack([ncx - 0.5 * nw, ncy - 0.5 * nh, ncx + 0.5 * nw, ncy + 0.5 * nh], dim=1)


def bbox2loc(src, dst, given=None):
    """utils/loc_bbox_iou.py:63-88.  ``given`` [n,4]: the values the result must have (a target that was computed and rounded
    elsewhere, e.g. in f32): the two centre differences and the two logs take those values - detached corrections, so the
    graph, and with it every derivative w.r.t. ``src``, stays bbox2loc's own, evaluated at the given target."""
    w, h = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    cx, cy = src[:, 0] + 0.5 * w, src[:, 1] + 0.5 * h
    bw, bh = dst[:, 2] - dst[:, 0], dst[:, 3] - dst[:, 1]
    bcx, bcy = dst[:, 0] + 0.5 * bw, dst[:, 1] + 0.5 * bh
    w = torch.maximum(w, torch.tensor(F32_EPS, dtype=w.dtype))
    h = torch.maximum(h, torch.tensor(F32_EPS, dtype=h.dtype))
    ux, uy, lw, lh = bcx - cx, bcy - cy, torch.log(bw / w), torch.log(bh / h)
    if given is not None:
        ux = ux + (given[:, 0] * w - ux).detach()
        uy = uy + (given[:, 1] * h - uy).detach()
        lw = lw + (given[:, 2] - lw).detach()
        lh = lh + (given[:, 3] - lh).detach()
    return torch.stack([ux / w, uy / h, lw, lh], dim=1)


def clamp_boxes(roi, clamp_x, clamp_y):
    xs = roi[:, 0::2].clamp(min=0, max=clamp_x)
    ys = roi[:, 1::2].clamp(min=0, max=clamp_y)
    return torch.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], dim=1)


def chain_losses(rpn_locs, rpn_scores, gt_rpn_loc, gt_rpn_label, cls_locs, scores, gt_roi_label, anchor, roi_anchor,
                 sample_src, sample_gt, bbox, img_size, detach_rois=False, rpn_sigma=1.0, roi_sigma=1.0):
    """One image's four losses with autograd through everything the reference differentiates: the RPN outputs directly, and
    rpn_locs again through roi = clamp(loc2bbox(anchor, loc))[chain] -> cat(roi, bbox)[keep_index] -> bbox2loc's target."""
    S = gt_roi_label.shape[0]
    a = roi_anchor.long()
    roi = clamp_boxes(loc2bbox(anchor[a].to(rpn_locs.dtype), rpn_locs[a]), img_size[1], img_size[2])
    if detach_rois:
        roi = roi.detach()
    cand = torch.cat([roi, bbox.to(roi.dtype)])
    sample_roi = cand[sample_src.long()]
    gt_roi_loc = bbox2loc(sample_roi, bbox.to(roi.dtype)[sample_gt.long()])
    roi_loc = cls_locs.view(S, -1, 4)[torch.arange(S), gt_roi_label]
    return [loc_loss(rpn_locs, gt_rpn_loc.to(rpn_locs.dtype), gt_rpn_label, rpn_sigma),
            F.cross_entropy(rpn_scores, gt_rpn_label, ignore_index=-1),
            loc_loss(roi_loc, gt_roi_loc, gt_roi_label, roi_sigma),
            F.cross_entropy(scores, gt_roi_label)]


def restated_on_run(sv, W, bbox, weights=(0, 0, 0, 0, 1), n_class=81, rpn_sigma=1.0, roi_sigma=1.0):
    """float64 autograd on a GPU run's own intermediates (what its autograd node kept): d rpn_out / d both from the
    restated losses of the kept outputs, then dW = dY^T X in float64."""
    A_ = sv["A"]
    rpn_out, both = sv["rpn_out"].cpu().double(), sv["both"].cpu().double()
    rl = rpn_out[:, :4 * A_].clone().requires_grad_(True)
    rs = rpn_out[:, 4 * A_:6 * A_].clone().requires_grad_(True)
    cl = both[:, :4 * n_class].clone().requires_grad_(True)
    sc = both[:, 4 * n_class:5 * n_class].clone().requires_grad_(True)
    sort_idx, keep_idx = sv["sort_idx"][0].cpu().long(), sv["keep_idx"][0].cpu().long()
    roi_anchor = sort_idx[keep_idx]
    src = sv["sample_src"][0].cpu()
    sroi = sv["sample_roi"][0].cpu().double()
    b = bbox.double()
    tl = torch.maximum(sroi[:, None, :2], b[:, :2])
    br = torch.minimum(sroi[:, None, 2:], b[:, 2:])
    inter = (br - tl).clamp(min=0).prod(2)
    iou = inter / ((sroi[:, 2:] - sroi[:, :2]).prod(1)[:, None] + (b[:, 2:] - b[:, :2]).prod(1) - inter)
    sample_gt = iou.argmax(1)
    losses = chain_losses(rl.reshape(-1, 4), rs.reshape(-1, 2), sv["gt_loc"][0].cpu(), sv["gt_label"][0].cpu(), cl, sc,
                          sv["gt_roi_label"][0].cpu(), sv["anchor"].cpu(), roi_anchor, src, sample_gt, bbox,
                          (3, sv["clamp_x"], sv["clamp_y"]), rpn_sigma=rpn_sigma, roi_sigma=roi_sigma)
    losses.append(sum(losses))
    sum(w * l for w, l in zip(weights, losses) if w).backward()
    C = W["rpn.loc.weight"].shape[1]
    X = sv["feat"].cpu().double().reshape(-1, sv["feat"].shape[-1])[:, :C]
    fc7 = sv["fc7"].cpu().double()
    g = {"rpn.loc.weight": rl.grad.T @ X, "rpn.loc.bias": rl.grad.sum(0), "rpn.score.weight": rs.grad.T @ X,
         "rpn.score.bias": rs.grad.sum(0), "head.cls_loc.weight": cl.grad.T @ fc7, "head.cls_loc.bias": cl.grad.sum(0),
         "head.score.weight": sc.grad.T @ fc7, "head.score.bias": sc.grad.sum(0)}
    return {k: v.reshape(W[k].shape) for k, v in g.items()}


# --------------------------------------------------------------------------------------------- per-kernel references
def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def upstream(up, k, inv_B):
    """(up[k] + up[4]) * inv_B as the kernels form it: the f32 values, combined in f64."""
    u = torch.as_tensor(up, dtype=torch.float32).double()
    return float((u[k] + u[4]) * f32(inv_B))


def _backward(obj, leaves):
    if torch.is_tensor(obj) and obj.requires_grad:
        obj.backward()
    return [torch.zeros_like(x) if x.grad is None else x.grad for x in leaves]


def ref_rpn(fused, A, gt_loc, gt_label, sigma, up, inv_B):
    """fused [B*n_pix, >= 6A] f32 (anchor t = pixel*A + a: loc at columns 4a..4a+3, (bg, fg) logits at 4A+2a..), gt_loc [B,n,4],
    gt_label [B,n] -> losses [B,2], d fused [B*n_pix, 6A], counts [B,2] = (n_pos, n_counted), status [B] (labels outside
    {-1,0,1}: counted nowhere), all float64 / int64."""
    B, n = gt_label.shape
    x = fused[:, :6 * A].detach().cpu().double().clone().requires_grad_(True)
    xb = x.reshape(B, n // A, 6 * A)
    w_loc, w_ce = upstream(up, 0, inv_B), upstream(up, 1, inv_B)
    losses = torch.full((B, 2), float("nan"), dtype=torch.float64)
    counts = torch.zeros((B, 2), dtype=torch.int64)
    status = torch.zeros((B,), dtype=torch.int64)
    obj = 0.0
    for b in range(B):
        lab = gt_label[b]
        locs, sc = xb[b, :, :4 * A].reshape(-1, 4), xb[b, :, 4 * A:].reshape(-1, 2)
        pos, cnt = lab == 1, (lab == 0) | (lab == 1)
        counts[b, 0], counts[b, 1], status[b] = int(pos.sum()), int(cnt.sum()), int((~cnt & (lab != -1)).sum())
        if pos.any():
            l = loc_loss(locs, gt_loc[b].double(), pos.long(), sigma)
            losses[b, 0] = l.detach()
            obj = obj + w_loc * l
        if cnt.any():
            l = F.cross_entropy(sc[cnt], lab[cnt])
            losses[b, 1] = l.detach()
            obj = obj + w_ce * l
    return losses, _backward(obj, [x])[0], counts, status


def ref_roi(both, n_class, sample_roi, gt_box, gt_roi_label, sigma, up, inv_B, gt_roi_loc=None):
    """both [B*S, >= 5 n_class] f32, sample_roi / gt_box [B,S,4], gt_roi_label [B,S]; gt_roi_loc = bbox2loc(sample_roi,
    gt_box) inside the graph.  ``gt_roi_loc`` [B,S,4] f32: the kernel's own target input - its values replace the f64
    target's (``bbox2loc(given=)``: the loss, d both and d sample_roi all see exactly the target the kernel was given, and
    d sample_roi still flows through bbox2loc's own graph).  Returns a dict of float64 / int64 tensors."""
    B, S = gt_roi_label.shape
    x = both[:, :5 * n_class].detach().cpu().double().clone().requires_grad_(True)
    sr = sample_roi.detach().cpu().double().reshape(-1, 4).clone().requires_grad_(True)
    t = bbox2loc(sr, gt_box.double().reshape(-1, 4), None if gt_roi_loc is None else gt_roi_loc.double().reshape(-1, 4))
    lab = gt_roi_label.reshape(-1)
    valid = (lab >= 0) & (lab < n_class)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    cl, sc = x[:, :4 * n_class], x[:, 4 * n_class:]
    roi_loc = cl.reshape(B * S, n_class, 4)[torch.arange(B * S), safe]
    w_loc, w_ce = upstream(up, 2, inv_B), upstream(up, 3, inv_B)
    losses = torch.full((B, 2), float("nan"), dtype=torch.float64)
    counts = torch.zeros((B, 2), dtype=torch.int64)
    obj = 0.0
    for b in range(B):
        rows = slice(b * S, (b + 1) * S)
        v = valid[rows]
        pos = v & (lab[rows] > 0)
        counts[b, 0], counts[b, 1] = int(pos.sum()), int(v.sum())
        if pos.any():
            l = loc_loss(roi_loc[rows], t[rows], pos.long(), sigma)
            losses[b, 0] = l.detach()
            obj = obj + w_loc * l
        if v.any():
            l = F.cross_entropy(sc[rows][v], lab[rows][v])
            losses[b, 1] = l.detach()
            obj = obj + w_ce * l
    d_both, d_sr = _backward(obj, [x, sr])
    with torch.no_grad():
        ap = loc2bbox(sr, roi_loc)
        ap[~valid] = float("nan")
        best, bi = first_max(sc)
    return dict(losses=losses, d_both=d_both, d_sample_roi=d_sr.reshape(B, S, 4), anchors_pred=ap.reshape(B, S, 4),
                classes_pred=bi.reshape(B, S), classes_score_pred=best.reshape(B, S), counts=counts,
                status=(~valid).reshape(B, S).sum(1))


def first_max(sc):
    """torch.max over the rows: the first maximum's column; a NaN is the maximum (the first NaN's column)."""
    m = torch.max(sc.detach(), dim=1)
    return m.values, m.indices


def chain_anchor(sample_src, keep_idx, sort_idx, n):
    """Per sample row the anchor at the end of sample_src -> keep_idx -> sort_idx, or -1 where the chain leaves a range."""
    R, n_pre = keep_idx.shape[-1], sort_idx.shape[-1]
    p = sample_src.long()
    ok = (p >= 0) & (p < R)
    q = torch.where(ok, keep_idx.long()[p.clamp(0, R - 1)], torch.full_like(p, -1))
    ok = ok & (q >= 0) & (q < n_pre)
    t = torch.where(ok, sort_idx.long()[q.clamp(0, n_pre - 1)], torch.full_like(p, -1))
    return torch.where(ok & (t >= 0) & (t < n), t, torch.full_like(p, -1))


def ref_scatter(d_sample_roi, sample_src, keep_idx, sort_idx, fused, anchors, A, clamp_x, clamp_y):
    """autograd of sum(d_sample_roi * clamp(loc2bbox(anchor[t], loc[t]))) along the chain, for an arbitrary d_sample_roi
    [B,S,4]: (d loc columns [B*n_pix, 4A], the f64 sum of the absolute per-row terms in the same layout)."""
    B, S = sample_src.shape
    n = anchors.shape[0]
    n_pix = n // A
    total = torch.zeros((B, n, 4), dtype=torch.float64)
    absum = torch.zeros((B, n, 4), dtype=torch.float64)
    for b in range(B):
        t = chain_anchor(sample_src[b], keep_idx[b], sort_idx[b], n)
        rows = torch.nonzero(t >= 0)[:, 0]
        if rows.numel() == 0:
            continue
        locs = fused[b * n_pix:(b + 1) * n_pix, :4 * A].detach().cpu().double().reshape(n, 4)
        leaf = locs[t[rows]].clone().requires_grad_(True)                 # one leaf row per sample row: its own term
        roi = clamp_boxes(loc2bbox(anchors.double()[t[rows]], leaf), clamp_x, clamp_y)
        (d_sample_roi[b].double()[rows] * roi).sum().backward()
        total[b].index_add_(0, t[rows], leaf.grad)
        absum[b].index_add_(0, t[rows], leaf.grad.abs())
    return total.reshape(B * n_pix, 4 * A), absum.reshape(B * n_pix, 4 * A)


def decoded(fused, anchors, A, t, b, n_pix, dtype):
    """The unclamped decode of anchor t of image b in ``dtype`` (rows of 4)."""
    locs = fused[b * n_pix:(b + 1) * n_pix, :4 * A].reshape(-1, 4).to(dtype)
    return loc2bbox(anchors.to(dtype)[t], locs[t])


# ------------------------------------------------------------------------------------------------- case generators
def knee_pair(sigma):
    """(gt, pred) f32 values whose f64 difference is the knee 1/sigma^2: exactly for sigma = 1 and 0.5 (knees 1 and 4); for
    sigma = 3 the knee 1/9 has no finite binary expansion, and gt - pred = hi + lo (two f32 pieces) is the nearest a
    difference of two f32 values comes to fl64(1/9): within 2^-47 of it, relative."""
    knee = 1.0 / sigma ** 2
    hi = f32(knee)
    lo = f32(knee - hi)
    return hi + 0.25 if lo == 0 else hi, 0.25 if lo == 0 else -lo


def rpn_pitches(A, kind):
    return (6 * A, (6 * A // 4 + 1) * 4, 6 * A + 5)[kind]


def roi_pitches(n_class, kind):
    w = 5 * n_class
    return (w, (w // 8 + 1) * 8, w + 2 if w % 2 else w + 3)[kind]


def pitched(rows, pitch, view=None):
    """rows [M, width] inside a NaN [M, pitch] buffer; returned as the column view [:, :view] (stride(0) = pitch)."""
    buf = torch.full((rows.shape[0], pitch), float("nan"))
    buf[:, :rows.shape[1]] = rows
    return buf if view is None or view == pitch else buf[:, :view]


def to_dev(v, dev):
    """A column view of a wider buffer keeps its row pitch on the device (a plain .to() would pack it)."""
    return v.to(dev) if v._base is None else v._base.to(dev)[:, :v.shape[1]]


def image_kind(b, B):
    """ordinary / no positive / all ignored, so that a batch's images differ; image 0 is always ordinary."""
    return ("ordinary", "no_positive", "all_ignored")[b % 3] if B > 1 else "ordinary"


def spread_d(g, shape, sigma):
    """|d| uniform over [0, 2.5 / sigma^2]: both sides of the knee, with a random sign."""
    d = torch.rand(shape, generator=g) * (2.5 / sigma ** 2)
    return d * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def make_rpn_case(A, pitch_kind, d_diff, n_pix, B, sigma, seed, scale=1.0):
    """A seeded RPN loss case.  ``fused`` is a column view [B*n_pix, d_pitch] of a NaN-padded buffer of row pitch ``pitch``
    (d_diff: d_pitch = pitch - 1 where there is a pad column to drop, so stride(0) != shape[1]).  Image 0's first positive
    anchor holds |d| = (0.5, 2) / sigma^2, the knee itself (``knee_pair``) and 0."""
    g = torch.Generator().manual_seed(seed)
    n = n_pix * A
    pitch = rpn_pitches(A, pitch_kind)
    d_pitch = max(6 * A, pitch - 1) if d_diff else pitch
    locs = torch.randn((B, n, 4), generator=g) * 0.5
    scores = torch.randn((B, n, 2), generator=g) * scale
    label = torch.multinomial(torch.tensor([0.5, 0.3, 0.2]), B * n, replacement=True, generator=g).reshape(B, n) - 1
    gt_loc = locs + spread_d(g, (B, n, 4), sigma)
    for b in range(B):
        kind = image_kind(b, B)
        if kind == "no_positive":
            label[b][label[b] == 1] = 0
        elif kind == "all_ignored":
            label[b] = -1
        else:
            first = int(torch.randint(0, n, (1,), generator=g))
            label[b, first] = 1
            if n > 1:
                label[b, (first + 1) % n] = 0
            kg, kp = knee_pair(sigma)
            locs[b, first] = torch.tensor([0.25, -0.5, kp, 0.375])
            gt_loc[b, first] = torch.tensor([0.25 + 0.5 / sigma ** 2, -0.5 - 2.0 / sigma ** 2, kg, 0.375])
    rows = torch.cat([locs.reshape(B * n_pix, 4 * A), scores.reshape(B * n_pix, 2 * A)], 1)
    return dict(A=A, n_pix=n_pix, B=B, sigma=sigma, pitch=pitch, d_pitch=d_pitch, fused=pitched(rows, pitch, d_pitch),
                gt_loc=gt_loc, gt_label=label, up=(0.5, -1.0, 2.0, 0.25, 1.0 / 32), inv_B=f32(1.0 / B))


def rpn_abs_d(c, b=0):
    """|gt - pred| in f64 of image b's positives, [n_pos, 4]."""
    A, n_pix = c["A"], c["n_pix"]
    locs = c["fused"][b * n_pix:(b + 1) * n_pix, :4 * A].reshape(-1, 4).double()
    pos = c["gt_label"][b] == 1
    return (c["gt_loc"][b].double()[pos] - locs[pos]).abs()


def make_roi_case(n_class, S, pitch_kind, B, sigma, seed, scale=1.0, floor=False):
    """A seeded RoI loss case: ``both`` [B*S, pitch] NaN-padded; sample boxes, their ground-truth boxes and
    gt_roi_loc = the f32 bbox2loc of the two, as ProposalTargetCreator hands it to the kernel.  Image 0's row 0 is the exact
    row: sample (0,0,32,32), gt (8,8,40,40) -> target (0.25, 0.25, 0, 0) exactly, with |d| = (0.5, 2) / sigma^2, the knee (to
    f32's nearest for sigma = 3) and 0.  ``floor``: rows 1.. of image 0 get sample boxes of width / height 0, f32 eps
    exactly (x1 = 0, x2 = eps) and an ordinary one, all positive (bbox2loc's max(w, eps) branches)."""
    g = torch.Generator().manual_seed(seed)
    pitch = roi_pitches(n_class, pitch_kind)
    xy = torch.rand((B, S, 2), generator=g) * 300
    wh = 8 + torch.rand((B, S, 2), generator=g) * 92
    sample_roi = torch.cat([xy, xy + wh], 2)
    gxy = xy + (torch.rand((B, S, 2), generator=g) - 0.5) * 0.5 * wh
    gwh = wh * (0.6 + 0.8 * torch.rand((B, S, 2), generator=g))
    gt_box = torch.cat([gxy, gxy + gwh], 2)
    label = torch.randint(0, n_class, (B, S), generator=g)
    label[torch.rand((B, S), generator=g) < 0.5] = 0
    cl = torch.randn((B, S, 4 * n_class), generator=g) * 0.5
    sc = torch.randn((B, S, n_class), generator=g) * scale
    exact = n_class > 1
    for b in range(B):
        if image_kind(b, B) != "ordinary":
            label[b] = 0
        elif exact:
            label[b, 0] = 1 + int(torch.randint(0, n_class - 1, (1,), generator=g))
            sample_roi[b, 0] = torch.tensor([0., 0., 32., 32.])
            gt_box[b, 0] = torch.tensor([8., 8., 40., 40.])
    n_floor = 0
    if floor and exact:
        eps = F32_EPS
        boxes = [(5., 7., 5., 30.), (5., 7., 40., 7.), (0., 3., eps, 40.), (2., 0., 50., eps), (0., 0., eps, eps), (9., 9., 9., 9.)]
        n_floor = min(len(boxes), S - 1)
        for i in range(n_floor):
            sample_roi[0, 1 + i] = torch.tensor(boxes[i])
            label[0, 1 + i] = 1 + (i % (n_class - 1))
    gt_roi_loc = bbox2loc(sample_roi.reshape(-1, 4), gt_box.reshape(-1, 4)).reshape(B, S, 4)
    d = spread_d(g, (B, S, 4), sigma)
    d[:, :, 2:] = d[:, :, 2:].clamp(-0.7, 0.7)                   # exp(dw) stays O(1): anchors_pred stays at image scale
    rows = torch.arange(S)
    for b in range(B):
        cols = 4 * label[b][:, None] + torch.arange(4)[None]
        keep = cl[b][rows[:, None], cols].clone()
        cl[b][rows[:, None], cols] = gt_roi_loc[b] - d[b]
        if b == 0 and n_floor:                                   # targets of ~1e9 there: keep the O(1) predictions
            cl[b][rows[1:1 + n_floor, None], cols[1:1 + n_floor]] = keep[1:1 + n_floor]
        if exact and image_kind(b, B) == "ordinary":
            k = int(label[b, 0])
            cl[b, 0, 4 * k:4 * k + 4] = torch.tensor([0.25 - 0.5 / sigma ** 2, 0.25 + 2.0 / sigma ** 2, -f32(1.0 / sigma ** 2), 0.])
    both = pitched(torch.cat([cl.reshape(B * S, -1), sc.reshape(B * S, -1)], 1), pitch)
    return dict(n_class=n_class, S=S, B=B, sigma=sigma, pitch=pitch, both=both, sample_roi=sample_roi, gt_box=gt_box,
                gt_roi_loc=gt_roi_loc, gt_roi_label=label, up=(0.5, -1.0, 2.0, 0.25, 1.0 / 32), inv_B=f32(1.0 / B),
                n_floor=n_floor)


def roi_abs_d(c, b=0):
    S, n_class = c["S"], c["n_class"]
    lab = c["gt_roi_label"][b]
    pos = (lab > 0) & (lab < n_class)
    cl = c["both"][b * S:(b + 1) * S, :4 * n_class].reshape(S, n_class, 4).double()
    pred = cl[torch.arange(S), lab.clamp(0, n_class - 1)]
    return (c["gt_roi_loc"][b].double() - pred).abs()[pos]


MARGIN = 1e-2                                          # px: no chained coordinate this near a clamp bound, exact rows apart


def grid_anchors(h, w, A, g):
    """[h*w*A, 4] anchors of a stride-16 map: A sizes per pixel, as the detector's (sizes 24..~400 px, three aspect ratios)."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    cx, cy = (xs.reshape(-1, 1) * 16 + 8), (ys.reshape(-1, 1) * 16 + 8)
    a = torch.arange(A, dtype=torch.float32)[None]
    size = 24.0 * 2 ** (a % 4) * (1 + 0.25 * (a // 4))
    ratio = torch.tensor([1.0, 0.5, 2.0])[(torch.arange(A) % 3)][None]
    bw, bh = size * ratio.sqrt(), size / ratio.sqrt()
    return torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 2).reshape(-1, 4)


def near_bound(box, clamp_x, clamp_y):
    """Per row: some coordinate within MARGIN of 0 or of its clamp."""
    bx = torch.minimum(box[:, 0::2].abs(), (box[:, 0::2] - clamp_x).abs())
    by = torch.minimum(box[:, 1::2].abs(), (box[:, 1::2] - clamp_y).abs())
    return (torch.minimum(bx, by) < MARGIN).any(1)


def make_scatter_case(S, R, n_pre, A, hw, B, seed, pitch_kind=1, d_diff=False, mode="random"):
    """A seeded case of the indirect term alone: an arbitrary d_sample_roi pushed along sample_src -> keep_idx -> sort_idx ->
    anchor into a pre-filled d_rpn_out.  sort_idx: a random order of distinct anchors, -1 after them; keep_idx: random sorted
    rows with the Q4 padding tail 0, 1, 2, ...; sample_src: rows of cat(roi, 3 gt boxes), so some are >= R.
    mode "one_anchor": every sample row reaches one anchor.  mode "edges": hand-built anchors (returned in ``edge_rows``)
    that decode exactly onto 0 / the clamp, clearly inside and clearly outside on each side, plus out-of-range chain
    entries and a zero d_sample_roi row."""
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    n_pix, n = h * w, h * w * A
    clamp_x, clamp_y = float(max(16 * w, 64)), float(max(16 * h, 48))
    pitch = rpn_pitches(A, pitch_kind)
    d_pitch = pitch + 3 if d_diff else pitch                     # d_rpn_out: a view of a wider buffer
    anchors = grid_anchors(h, w, A, g)
    locs = torch.randn((B, n, 4), generator=g) * 0.2
    n_sorted = min(n, n_pre)
    sort_idx = torch.full((B, n_pre), -1, dtype=torch.int32)
    keep_idx = torch.zeros((B, R), dtype=torch.int32)
    sample_src = torch.zeros((B, S), dtype=torch.int32)
    for b in range(B):
        sort_idx[b, :n_sorted] = torch.randperm(n, generator=g)[:n_sorted].int()
        n_keep = max(1, (2 * R) // 3)                            # the NMS kept n_keep rows; the rest is the Q4 padding
        keep_idx[b, :n_keep] = torch.randint(0, min(n_sorted, n_keep), (n_keep,), generator=g).int()
        keep_idx[b, n_keep:] = torch.arange(R - n_keep, dtype=torch.int32) % n_sorted
        sample_src[b] = torch.randint(0, R, (S,), generator=g).int()
        from_gt = torch.rand((S,), generator=g) < 0.1           # rows of the appended ground-truth boxes: no gradient
        sample_src[b][from_gt] = R + torch.randint(0, 3, (int(from_gt.sum()),), generator=g).int()
        if S >= 2:
            sample_src[b, S - 1] = R + 1
    d_sample_roi = torch.randn((B, S, 4), generator=g)
    edge_rows = {}
    if mode == "one_anchor":
        sample_src[:] = torch.randint(0, R, (B, S), generator=g).int()
        keep_idx[:] = 0                                          # every proposal row is sorted row 0
    elif mode == "edges":
        # image 0: anchors 0..5 replaced by hand-built boxes with zero offsets (exact decodes: the sums below are exact in
        # f32 and f64), sample row i -> proposal row i -> sorted row i -> anchor i
        cx, cy = clamp_x, clamp_y
        boxes = {"at_zero": (0., 0., 32., 32.), "at_clamp": (cx - 32, cy - 32, cx, cy),
                 "inside": (8., 8., 40., 40.), "out_left_top": (-24., -16., 40., 32.),
                 "out_right_bottom": (cx - 40, cy - 32, cx + 24, cy + 16), "all_out": (-64., -48., -8., -8.)}
        assert n >= len(boxes) + 2 and S >= len(boxes) + 5 and R >= S and n_pre >= S
        for i, (k, box) in enumerate(boxes.items()):
            anchors[i] = torch.tensor(box)
            locs[0, i] = 0
            sort_idx[0, i] = i
            keep_idx[0, i] = i
            sample_src[0, i] = i
            edge_rows[k] = i
        i = len(boxes)
        sort_idx[0, i:i + 2] = torch.tensor([n - 1, n - 2], dtype=torch.int32)
        keep_idx[0, i:i + 2] = torch.tensor([i, i + 1], dtype=torch.int32)
        sample_src[0, i] = -1                                    # out of range: ignored
        sample_src[0, i + 1] = R + 7
        keep_idx[0, i + 2] = -3
        sample_src[0, i + 2] = i + 2                             # -> keep_idx out of range
        keep_idx[0, i + 3] = n_pre + 5
        sample_src[0, i + 3] = i + 3
        sample_src[0, i + 4] = 2                                 # a second row onto "inside", with a zero d_sample_roi row
        # no other row reaches the hand-built anchors: their gradient is then one row's, known in closed form
        first = i + 5
        assert n >= 24 and n_sorted >= 24 and R >= 24
        n_keep = max(1, (2 * R) // 3)
        rest = keep_idx[0, 12:n_keep]
        rest[rest < 12] += 12
        rest = sample_src[0, first:]                             # (the Q4 tail still points at sorted rows 0, 1, 2, ...)
        p = rest.long().clamp(0, R - 1)
        rest[(rest < R) & ((rest < 12) | (keep_idx[0].long()[p] < 12))] = 12
        rest = sort_idx[0, 12:n_sorted]
        rest[(rest >= 0) & (rest < 6)] += 6
        d_sample_roi[0, i + 4] = 0
        edge_rows["zero_row"] = i + 4
    exact = torch.zeros((B, n), dtype=torch.bool)
    if mode == "edges":
        exact[0, :2] = True
    # redraw the offsets of chained anchors whose f64 decode has a coordinate within MARGIN of a bound (the mask is a step)
    for b in range(B):
        for _ in range(100):
            t = chain_anchor(sample_src[b], keep_idx[b], sort_idx[b], n)
            t = t[t >= 0].unique()
            t = t[~exact[b][t]]
            box = loc2bbox(anchors.double()[t], locs[b].double()[t])
            bad = t[near_bound(box, clamp_x, clamp_y)]
            if bad.numel() == 0:
                break
            locs[b, bad] = torch.randn((bad.numel(), 4), generator=g) * 0.2
        else:
            raise AssertionError("redraw did not converge")
    rows = torch.cat([locs.reshape(B * n_pix, 4 * A), torch.randn((B * n_pix, 2 * A), generator=g)], 1)
    d_out = torch.randn((B * n_pix, d_pitch), generator=g)
    return dict(S=S, R=R, n_pre=n_pre, A=A, n_pix=n_pix, B=B, pitch=pitch, d_pitch=d_pitch, clamp_x=clamp_x, clamp_y=clamp_y,
                fused=pitched(rows, pitch), anchors=anchors, sort_idx=sort_idx, keep_idx=keep_idx, sample_src=sample_src,
                d_sample_roi=d_sample_roi, d_out=d_out if d_pitch == pitch else d_out[:, :pitch], exact=exact, edge_rows=edge_rows, mode=mode)


def ulp_bound(want, bits, scale=None):
    """2^-bits |want| + 1e-12 max |want|: one f32 rounding of an f64 result with slack, plus f64 cancellation."""
    scale = float(want.abs().max()) if scale is None else scale
    return want.abs() * math.ldexp(1.0, -bits) + 1e-12 * scale
