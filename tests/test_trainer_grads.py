"""FasterRCNNTrainer(head_grads=True): the backward of the four losses into the eight head parameters on a frozen backbone.

tests/golden/trainer_grads_ref.npz was made by the REFERENCE's own FasterRCNNTrainer on CPU
(tests/golden/make_golden_trainer_grads.py): the same weights, image and seed as trainer_ref.npz, the backbone frozen,
``losses[-1].backward()``, for both head img_size variants, plus a run with the proposals detached (the size of the
indirect term) and the index chain of the forward.  ``restated_grads`` is the float64 torch-autograd statement of the
gradients - direct terms and the indirect term through the proposals - that the GPU tests measure the kernels against; the
CPU tests pin it to the fixture first.
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: F401

from trainer_losses_restated import F32_EPS, bbox2loc, chain_losses, loc2bbox, loc_loss, restated_on_run  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLASS = 81
A = 9
PARAMS = ("rpn.loc.weight", "rpn.loc.bias", "rpn.score.weight", "rpn.score.bias",
          "head.cls_loc.weight", "head.cls_loc.bias", "head.score.weight", "head.score.bias")


@pytest.fixture(scope="module")
def zg(golden_dir):
    return np.load(os.path.join(golden_dir, "trainer_grads_ref.npz"))


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "trainer_ref.npz"))


def t(z, k):
    return torch.from_numpy(z[k])


def reference_state_dict():
    from two_stage_object_detection_amd.testing import synthetic_detector
    _, sd = synthetic_detector("hardnet39", conditioned=True)
    return {("feat_extra." + k[len("extractor."):] if k.startswith("extractor.") else k): v for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------ the restatement
# loc_loss, loc2bbox, bbox2loc, chain_losses, restated_on_run: tests/trainer_losses_restated.py (shared with the loss sweep)
def restated_grads(X, fc7, W, gt_rpn_loc, gt_rpn_label, gt_roi_label, anchor, roi_anchor, sample_src, sample_gt, bbox,
                   img_size, weights=(0, 0, 0, 0, 1), detach_rois=False, dtype=torch.float64):
    """The eight gradients of sum_k weights[k] * loss_k (loss 4 = the total) for one image in ``dtype``: X [h*w, C] the
    feature map's pixel rows (NHWC order), fc7 [S, C], W the eight parameters by name."""
    P = {k: W[k].detach().to(dtype).reshape(W[k].shape[0], -1).squeeze(-1).clone().requires_grad_(True) for k in PARAMS}
    X, fc7 = X.to(dtype), fc7.to(dtype)
    rpn_locs = (X @ P["rpn.loc.weight"].T + P["rpn.loc.bias"]).reshape(-1, 4)
    rpn_scores = (X @ P["rpn.score.weight"].T + P["rpn.score.bias"]).reshape(-1, 2)
    cls_locs = fc7 @ P["head.cls_loc.weight"].T + P["head.cls_loc.bias"]
    scores = fc7 @ P["head.score.weight"].T + P["head.score.bias"]
    losses = chain_losses(rpn_locs, rpn_scores, gt_rpn_loc, gt_rpn_label, cls_locs, scores, gt_roi_label, anchor, roi_anchor,
                          sample_src, sample_gt, bbox, img_size, detach_rois)
    losses.append(sum(losses))
    sum(w * l for w, l in zip(weights, losses) if w).backward()
    return {k: P[k].grad.reshape(W[k].shape) for k in PARAMS}


def anchors(z):
    """The [h*w*A, 4] anchors of the fixture's 320x448 image (stride 16), as the reference enumerates them."""
    from oracle import box
    H, W = z["img_u8"].shape[1:]
    return box.enumerate_shifted_anchor(box.generate_basic_anchor(), 16, H // 16, W // 16).float()


@pytest.fixture(scope="module")
def trunk(z):
    """The reference's feature map [1,C,h,w] of the fixture's image and the head's pooled features fc7 [S,C] per variant,
    from the CPU oracle (identical to the reference's tensors; they are not stored in the fixture to keep it small)."""
    from oracle import box
    from oracle.detector import extractor_forward
    sd = {("extractor." + k[len("feat_extra."):] if k.startswith("feat_extra.") else k): v for k, v in reference_state_dict().items()}
    with torch.no_grad():
        feat = extractor_forward(sd, torch.from_numpy(z["img_u8"]).float()[None] / 255, "hardnet39")
        rois = t(z, "sample_roi")
        hf, wf = feat.shape[2:]
        C, H, W = z["img_u8"].shape
        fc7 = {}
        for variant, size in (("chw", (C, H, W)), ("hw", (H, W))):        # the head's img_size (quirk Q2): x by [1], y by [0]
            fm = torch.zeros_like(rois)
            fm[:, [0, 2]] = rois[:, [0, 2]] / size[1] * wf
            fm[:, [1, 3]] = rois[:, [1, 3]] / size[0] * hf
            pooled = box.roi_pool(feat, torch.cat([torch.zeros(len(rois), 1), fm], 1), (7, 7), 1.0)
            fc7[variant] = pooled.mean((2, 3))
    return feat, fc7


def fixture_inputs(z, zg, trunk, variant):
    feat = trunk[0][0]                                                   # [C,h,w]
    return dict(X=feat.permute(1, 2, 0).reshape(-1, feat.shape[0]), fc7=trunk[1][variant],
                gt_rpn_loc=t(z, "gt_rpn_loc"), gt_rpn_label=t(z, "gt_rpn_label"), gt_roi_label=t(z, "gt_roi_label"),
                anchor=anchors(z), roi_anchor=t(zg, "roi_anchor"), sample_src=t(zg, "sample_src"),
                sample_gt=t(zg, "sample_gt"), bbox=t(z, "bbox"), img_size=(3,) + tuple(z["img_u8"].shape[1:]))


def close(got, want, frac, what=""):
    scale = float(want.abs().max())
    err = float((got.double() - want.double()).abs().max())
    assert err <= frac * max(scale, 1e-30), (what, err, scale)


# ----------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_restated_grads_reproduce_the_reference(z, zg, trunk, variant):
    """float64 autograd over the fixture's features and index chain gives the reference's eight gradients - including
    rpn.loc's indirect term through the proposals - to the reference's own f32 noise."""
    assert int(zg["seed"]) == int(z["seed"])
    W = reference_state_dict()
    g = restated_grads(W=W, **fixture_inputs(z, zg, trunk, variant))
    for k in PARAMS:
        close(g[k], t(zg, f"{variant}.grad.{k}"), 1e-4, k)
    gd = restated_grads(W=W, detach_rois=True, **fixture_inputs(z, zg, trunk, variant))
    for k in ("rpn.loc.weight", "rpn.loc.bias"):
        close(gd[k], t(zg, f"{variant}.grad_detached.{k}"), 1e-4, k)


@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_indirect_term_is_material(zg, variant):
    """Detaching the proposals moves rpn.loc's gradient by far more than any tolerance used here (1e-3 of max |g|)."""
    for k in ("rpn.loc.weight", "rpn.loc.bias"):
        g, gd = t(zg, f"{variant}.grad.{k}"), t(zg, f"{variant}.grad_detached.{k}")
        assert float((g - gd).abs().max()) >= 0.05 * float(g.abs().max()), k
    assert int((t(zg, "sample_src") < 600).sum()) >= 4


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(tsod_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text)}


NEW_ENTRY_POINTS = ("tsod_proposal_targets_src_f32", "tsod_rpn_losses_grad_f32", "tsod_roi_losses_grad_f32",
                    "tsod_rpn_roi_scatter_f32", "tsod_wgrad_workspace_bytes", "tsod_wgrad_f32")


def test_head_grad_entry_points_abi():
    """The new entry points: declared in include/tsod.h, bound with as many arguments as declared, exported by the library;
    the version and the existing proposal-target entry point are unchanged."""
    import ctypes
    from two_stage_object_detection_amd import _ffi
    decl = _declarations()
    for name in NEW_ENTRY_POINTS:
        assert name in decl and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(decl[name].split(",")) == len(_ffi._SIGNATURES[name][1]), name
    assert len(decl["tsod_proposal_targets_f32"].split(",")) == 17
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(raw, name), name
    lib = _ffi.lib()
    assert lib.tsod_version() == 242
    assert lib.tsod_wgrad_workspace_bytes(0, 56, 1024) == 0
    assert lib.tsod_wgrad_workspace_bytes(33600, 56, 1024) > 0


def test_head_grads_flag_defaults_off():
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    assert FasterRCNNTrainer(mode="train", num_classes=80).head_grads is False
    assert FasterRCNNTrainer(mode="train", num_classes=80, head_grads=True).head_grads is True


# ----------------------------------------------------------------------------------------------------------------- GPU
def ab_bound(a, b):
    """sum_m |a[m,n]| |b[m,k]| in float64: the scale of f32 MFMA round-off (cdna_hip_programming.md, FP32-input MFMA)."""
    return np.abs(a).T @ np.abs(b)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,pitch", [(1000, 56, 512, 56), (333, 408, 1024, 408), (257, 56, 1024, 61),
                                         (128, 408, 512, 408), (33600, 56, 1024, 56)])
def test_wgrad_kernel_vs_float64(dev, M, N, K, pitch):
    from two_stage_object_detection_amd import hip_ops
    g = torch.Generator().manual_seed(M + N + K)
    dy_full = torch.randn((M, pitch), generator=g)
    dy = dy_full[:, :N]
    x = torch.randn((M, K), generator=g)
    want = dy.double().numpy().T @ x.double().numpy()
    want_b = dy.double().sum(0).numpy()
    bound = ab_bound(dy.double().numpy(), x.double().numpy())
    bound_b = dy.double().abs().sum(0).numpy()
    n0 = N * 2 // 3
    n1 = N - n0 - 3 if N > 60 else N - n0 - 2                   # trailing rows dropped, as the fused pad rows
    dyd, xd = dy_full.to(dev)[:, :N], x.to(dev)
    outs = [torch.full((n0, K), float("nan"), device=dev), torch.full((n0,), float("nan"), device=dev),
            torch.full((n1, K), float("nan"), device=dev), torch.full((n1,), float("nan"), device=dev)]
    hip_ops.wgrad(dyd, xd, *outs)
    first = [o.clone() for o in outs]
    hip_ops.wgrad(dyd, xd, *outs)
    assert all(torch.equal(a, b) for a, b in zip(first, outs)), "two runs differ"
    dw = torch.cat([outs[0], outs[2]]).double().cpu().numpy()
    db = torch.cat([outs[1], outs[3]]).double().cpu().numpy()
    rows = n0 + n1
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    assert (np.abs(dw - want[:rows]) <= 4e-6 * bound[:rows] + 1e-30).all(), float((np.abs(dw - want[:rows]) / bound[:rows]).max())
    assert (np.abs(db - want_b[:rows]) <= 4e-6 * bound_b[:rows] + 1e-30).all()
    # accumulate: adds to what is there
    base = [torch.randn(o.shape, generator=g).to(dev) for o in outs]
    acc = [b.clone() for b in base]
    hip_ops.wgrad(dyd, xd, *acc, accumulate=True)
    for a, b, o in zip(acc, base, first):
        assert torch.equal(a, b + o)


def pitched(rows, width, pitch, dev):
    buf = torch.full((rows.shape[0], pitch), float("nan"))
    buf[:, :width] = rows
    return buf.to(dev)


def kernel_chain_grads(dev, rpn_locs, rpn_scores, gt_rpn_loc, gt_rpn_label, cls_locs, scores, gt_roi_label, anchor,
                       sort_idx, keep_idx, sample_src, sample_roi, gt_roi_loc, img_size, up):
    """d rpn_out and d both from the three loss-gradient kernels, for one image."""
    from two_stage_object_detection_amd import hip_ops
    P = rpn_locs.shape[0] // A
    fused = torch.full((P, 56), float("nan"))
    fused[:, :4 * A] = rpn_locs.reshape(P, 4 * A)
    fused[:, 4 * A:6 * A] = rpn_scores.reshape(P, 2 * A)
    fused = fused.to(dev)
    both = torch.full((cls_locs.shape[0], 408), float("nan"))
    both[:, :4 * N_CLASS] = cls_locs
    both[:, 4 * N_CLASS:5 * N_CLASS] = scores
    both = both.to(dev)
    upd = torch.tensor(up, dtype=torch.float32, device=dev)
    d_rpn, _ = hip_ops.rpn_losses_grad(fused, A, gt_rpn_loc[None].to(dev), gt_rpn_label[None].to(dev), 1.0, upd, 1.0)
    d_both, d_roi = hip_ops.roi_losses_grad(both, N_CLASS, sample_roi[None].to(dev), gt_roi_loc[None].to(dev),
                                            gt_roi_label[None].to(dev), 1.0, upd, 1.0)
    hip_ops.rpn_roi_scatter(d_rpn, d_roi, sample_src[None].int().to(dev), keep_idx[None].int().to(dev),
                            sort_idx[None].int().to(dev), fused, anchor.to(dev), A, img_size[1], img_size[2])
    return d_rpn.cpu(), d_both.cpu()


def f64_chain_grads(rpn_locs, rpn_scores, gt_rpn_loc, gt_rpn_label, cls_locs, scores, gt_roi_label, anchor, roi_anchor,
                    sample_src, sample_gt, bbox, img_size, up):
    v = [x.double().clone().requires_grad_(True) for x in (rpn_locs, rpn_scores, cls_locs, scores)]
    losses = chain_losses(v[0], v[1], gt_rpn_loc, gt_rpn_label, v[2], v[3], gt_roi_label, anchor, roi_anchor, sample_src,
                          sample_gt, bbox, img_size)
    losses.append(sum(losses))
    sum(w * l for w, l in zip(up, losses) if w).backward()
    return [x.grad for x in v], losses


def chain_case(z, zg, variant, dup=False):
    """The fixture's intermediates, with the index chain written as the GPU path's sort_idx / keep_idx.  ``dup``: the last
    100 rows of keep_idx replaced by 0, 1, 2, ... (quirk Q4's padding: duplicates of earlier sorted rows), and three positive
    samples' proposal rows pointed at one sorted row, so that one anchor receives three sample rows."""
    roi_anchor = t(zg, "roi_anchor").long()
    uniq = []
    for a in roi_anchor.tolist():
        if a not in uniq:
            uniq.append(a)
    sort_idx = torch.tensor(uniq + [-1] * 8, dtype=torch.int32)
    keep_idx = torch.tensor([uniq.index(a) for a in roi_anchor.tolist()], dtype=torch.int32)
    if dup:
        keep_idx[-100:] = torch.arange(100, dtype=torch.int32)
        src, lab = t(zg, "sample_src").long(), t(z, "gt_roi_label")
        pos_rows = src[(lab > 0) & (src < 600)]
        keep_idx[pos_rows[1:3]] = int(keep_idx[pos_rows[0]])
    roi_anchor = sort_idx.long()[keep_idx.long()]
    c = dict(rpn_locs=t(z, "rpn_locs")[0], rpn_scores=t(z, "rpn_scores")[0], gt_rpn_loc=t(z, "gt_rpn_loc"),
             gt_rpn_label=t(z, "gt_rpn_label"), cls_locs=t(z, f"{variant}.roi_cls_locs")[0],
             scores=t(z, f"{variant}.roi_scores")[0], gt_roi_label=t(z, "gt_roi_label"), anchor=anchors(z),
             sample_src=t(zg, "sample_src"), sample_gt=t(zg, "sample_gt"), bbox=t(z, "bbox"),
             img_size=(3,) + tuple(z["img_u8"].shape[1:]))
    with torch.no_grad():                                          # the f32 forward of the chain: sample_roi, gt_roi_loc
        roi = loc2bbox(c["anchor"][roi_anchor], c["rpn_locs"][roi_anchor])
        xs = roi[:, 0::2].clamp(min=0, max=c["img_size"][1])
        ys = roi[:, 1::2].clamp(min=0, max=c["img_size"][2])
        roi = torch.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], dim=1)
        sample_roi = torch.cat([roi, c["bbox"]])[c["sample_src"].long()]
        gt_roi_loc = bbox2loc(sample_roi, c["bbox"][c["sample_gt"].long()])
    return c, roi_anchor, sort_idx, keep_idx, sample_roi, gt_roi_loc


def compare_chain(dev, c, roi_anchor, sort_idx, keep_idx, sample_roi, gt_roi_loc, up, frac=2e-5):
    d_rpn, d_both = kernel_chain_grads(dev, c["rpn_locs"], c["rpn_scores"], c["gt_rpn_loc"], c["gt_rpn_label"], c["cls_locs"],
                                       c["scores"], c["gt_roi_label"], c["anchor"], sort_idx, keep_idx, c["sample_src"],
                                       sample_roi, gt_roi_loc, c["img_size"], up)
    (gl, gs, gc, gsc), losses = f64_chain_grads(c["rpn_locs"], c["rpn_scores"], c["gt_rpn_loc"], c["gt_rpn_label"],
                                                c["cls_locs"], c["scores"], c["gt_roi_label"], c["anchor"], roi_anchor,
                                                c["sample_src"], c["sample_gt"], c["bbox"], c["img_size"], up)
    P = gl.shape[0] // A
    assert torch.isfinite(d_rpn).all() and torch.isfinite(d_both).all()
    assert (d_rpn[:, 6 * A:] == 0).all() and (d_both[:, 5 * N_CLASS:] == 0).all()
    for got, want, what in ((d_rpn[:, :4 * A], gl.reshape(P, 4 * A), "rpn loc"), (d_rpn[:, 4 * A:6 * A], gs.reshape(P, 2 * A), "rpn score"),
                            (d_both[:, :4 * N_CLASS], gc, "head loc"), (d_both[:, 4 * N_CLASS:5 * N_CLASS], gsc, "head score")):
        if float(want.abs().max()) == 0:
            assert (got == 0).all(), what
        else:
            close(got, want, frac, what)
    return losses


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_loss_grad_kernels_on_reference_intermediates(dev, z, zg, variant):
    """rpn_losses_grad + roi_losses_grad + the indirect scatter vs float64 autograd, with the fixture's chain and with
    padded duplicate rows (the sample rows that reach one anchor twice sum)."""
    for dup in (False, True):
        case = chain_case(z, zg, variant, dup)
        if dup:
            c, roi_anchor = case[0], case[1]
            src, lab = c["sample_src"].long(), c["gt_roi_label"]
            reached = roi_anchor[src[(lab > 0) & (src < 600)]]
            assert reached.unique().numel() <= reached.numel() - 2
        for up in ((0, 0, 0, 0, 1), (0.5, -1.0, 2.0, 0.25, 1 / 32)):
            compare_chain(dev, *case, up=up)


@pytest.mark.gpu
def test_loss_grad_kernel_edge_cases(dev, z, zg):
    """No positive anchor, all-background samples, d == 0: the losses are NaN (torch's 0/0) and the gradients finite and
    equal to torch's autograd."""
    c, roi_anchor, sort_idx, keep_idx, sample_roi, gt_roi_loc = chain_case(z, zg, "hw")
    up = (0.3, 0.7, 1.1, 0.9, 1.0)
    e = dict(c, gt_rpn_label=torch.where(c["gt_rpn_label"] == 1, torch.zeros_like(c["gt_rpn_label"]), c["gt_rpn_label"]),
             gt_roi_label=torch.zeros_like(c["gt_roi_label"]))
    losses = compare_chain(dev, e, roi_anchor, sort_idx, keep_idx, sample_roi, gt_roi_loc, up)
    assert torch.isnan(losses[0]) and torch.isnan(losses[2])
    e = dict(c, gt_rpn_label=torch.full_like(c["gt_rpn_label"], -1))                 # every anchor ignored: CE is NaN
    losses = compare_chain(dev, e, roi_anchor, sort_idx, keep_idx, sample_roi, gt_roi_loc, up)
    assert torch.isnan(losses[1]) and torch.isnan(losses[0])
    # d == 0 on one positive anchor and one positive sample's offsets: abs's zero subgradient
    pos = int(torch.nonzero(c["gt_rpn_label"] == 1)[0])
    gl = c["gt_rpn_loc"].clone()
    gl[pos] = c["rpn_locs"][pos]
    rpos = int(torch.nonzero(c["gt_roi_label"] > 0)[0])
    cl = c["cls_locs"].clone()
    lab = int(c["gt_roi_label"][rpos])
    cl[rpos, 4 * lab:4 * lab + 4] = gt_roi_loc[rpos]
    e = dict(c, gt_rpn_loc=gl, cls_locs=cl)
    compare_chain(dev, e, roi_anchor, sort_idx, keep_idx, sample_roi, gt_roi_loc, up)
    d_rpn, d_both = kernel_chain_grads(dev, e["rpn_locs"], e["rpn_scores"], gl, e["gt_rpn_label"], cl, e["scores"],
                                       e["gt_roi_label"], e["anchor"], sort_idx, keep_idx, e["sample_src"], sample_roi,
                                       gt_roi_loc, e["img_size"], up)
    pix, a = divmod(pos, A)
    assert (d_rpn[pix, 4 * a:4 * a + 4] == 0).all()
    assert (d_both[rpos, 4 * lab:4 * lab + 4] == 0).all()


def grad_trainer(dev, variant="chw"):
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    tr = FasterRCNNTrainer(mode="train", num_classes=80, head_img_size=variant, head_grads=True)
    tr.load_state_dict(reference_state_dict(), strict=True)
    tr = tr.to(dev).eval()
    tr.feat_extra.requires_grad_(False)
    return tr


def image(z):
    return torch.from_numpy(z["img_u8"]).float() / 255


def head_grads(tr):
    named = dict(tr.named_parameters())
    return {k: named[k].grad.detach().clone() for k in PARAMS}


def zero_grads(tr):
    for p in tr.parameters():
        p.grad = None


def run(tr, dev, z, gts=None, weights=(0, 0, 0, 0, 1)):
    x = image(z)[None].to(dev)
    bbox, label = t(z, "bbox").to(dev), t(z, "label").to(dev)
    losses = tr(x, [bbox], [label])[0]
    sum(w * l for w, l in zip(weights, losses) if w).backward()
    return losses


def saved_node(losses):
    node = losses[-1].grad_fn
    while not hasattr(node, "saved"):
        node = node.next_functions[0][0]
    return node.saved


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_trainer_head_grads_end_to_end(dev, z, zg, variant):
    """losses[-1].backward() fills the eight .grad tensors with the reference's gradients: within 1e-3 of each tensor's
    max |g| of the fixture (the f32 noise of two different trunks and RPN GEMMs moves the RPN outputs by ~1e-6 relative,
    which the loss gradients carry), and within 2e-5 of float64 autograd on the run's own intermediates."""
    tr = grad_trainer(dev, variant)
    losses = run(tr, dev, z)
    assert all(l.requires_grad for l in losses)
    torch.testing.assert_close(torch.stack([l.detach() for l in losses]).cpu(), t(z, f"{variant}.losses"), rtol=1e-4, atol=0)
    got = head_grads(tr)
    for k in PARAMS:
        assert torch.isfinite(got[k]).all(), k
        close(got[k].cpu(), t(zg, f"{variant}.grad.{k}"), 1e-3, k)
    want = restated_on_run(saved_node(losses), {k: v for k, v in reference_state_dict().items() if k in PARAMS}, t(z, "bbox"))
    for k in PARAMS:
        close(got[k].cpu(), want[k], 2e-5, k)


@pytest.mark.gpu
def test_trainer_head_grads_linearity(dev, z):
    tr = grad_trainer(dev)
    per = []
    for k in range(4):
        zero_grads(tr)
        run(tr, dev, z, weights=tuple(1 if i == k else 0 for i in range(5)))
        per.append(head_grads(tr))
    zero_grads(tr)
    run(tr, dev, z, weights=(0.5, 0, 0, 2, 1 / 32))
    got = head_grads(tr)
    for k in PARAMS:
        want = 0.5 * per[0][k] + 2 * per[3][k] + (per[0][k] + per[1][k] + per[2][k] + per[3][k]) / 32
        close(got[k], want, 1e-5, k)
    # accumulation: a second backward adds
    run(tr, dev, z, weights=(0.5, 0, 0, 2, 1 / 32))
    for k in PARAMS:
        close(head_grads(tr)[k], 2 * got[k], 1e-6, k)


@pytest.mark.gpu
def test_trainer_head_grads_batch_mean(dev, z):
    tr = grad_trainer(dev)
    x = image(z).to(dev)
    bbox, label = t(z, "bbox").to(dev), t(z, "label").to(dev)
    gts = [(bbox, label), (bbox[:2].clone(), label[:2].clone())]
    singles = []
    for b, l in gts:
        zero_grads(tr)
        tr(x[None], [b], [l])[0][-1].backward()
        singles.append(head_grads(tr))
    zero_grads(tr)
    tr(torch.stack([x, x]), [b for b, _ in gts], [l for _, l in gts])[0][-1].backward()
    got = head_grads(tr)
    for k in PARAMS:
        close(got[k], (singles[0][k] + singles[1][k]) / 2, 1e-3, k)


@pytest.mark.gpu
def test_trainer_head_grads_saved_state(dev, z):
    """The backward of forward #1 issued after forward #2 gives forward #1's gradients (the node keeps its own copies)."""
    tr = grad_trainer(dev)
    x = image(z)[None].to(dev)
    bbox, label = t(z, "bbox").to(dev), t(z, "label").to(dev)
    zero_grads(tr)
    tr(x, [bbox], [label])[0][-1].backward()
    want = head_grads(tr)
    zero_grads(tr)
    first = tr(x, [bbox], [label])[0]
    second = tr(x * 0.5, [bbox[:2].clone()], [label[:2].clone()])[0]
    first[-1].backward()
    got = head_grads(tr)
    for k in PARAMS:
        assert torch.equal(got[k], want[k]), k
    assert second[-1].requires_grad


@pytest.mark.gpu
def test_trainer_repacks_after_optimizer_step(dev, z):
    """After SGD steps the head parameters in place, the next forward runs the new weights: its losses are a fresh trainer's
    loaded with the stepped state_dict (with stale packed weights they would be the old losses)."""
    tr = grad_trainer(dev)
    heads = [p for n, p in tr.named_parameters() if n in PARAMS]
    opt = torch.optim.SGD(heads, lr=0.5)
    before = run(tr, dev, z)
    opt.step()
    x, bbox, label = image(z)[None].to(dev), t(z, "bbox").to(dev), t(z, "label").to(dev)
    with torch.no_grad():
        after = torch.stack(tr(x, [bbox], [label])[0])
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    fresh = FasterRCNNTrainer(mode="train", num_classes=80)
    fresh.load_state_dict({k: v.cpu() for k, v in tr.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = torch.stack(fresh(x, [bbox], [label])[0])
    assert not torch.equal(after, torch.stack([l.detach() for l in before]))
    torch.testing.assert_close(after, want, rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_trainer_head_grads_opt_in(dev, z):
    from two_stage_object_detection_amd._ffi import TsodError
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    x, bbox, label = image(z)[None].to(dev), t(z, "bbox").to(dev), t(z, "label").to(dev)
    tr = FasterRCNNTrainer(mode="train", num_classes=80)
    tr.load_state_dict(reference_state_dict(), strict=True)
    tr = tr.to(dev).eval()
    losses = tr(x, [bbox], [label])[0]
    assert not any(l.requires_grad for l in losses)
    g = grad_trainer(dev)
    next(g.feat_extra.parameters()).requires_grad_(True)
    with pytest.raises(TsodError, match=r"requires_grad_\(False\)"):
        g(x, [bbox], [label])
    with torch.no_grad():                                           # grad mode off: the default forward, no check
        assert not g(x, [bbox], [label])[0][0].requires_grad
