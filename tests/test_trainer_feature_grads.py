"""FasterRCNNTrainer(features=...): d losses / d feature map through autograd.

tests/golden/trainer_feature_grads_ref.npz was made by the REFERENCE's own FasterRCNNTrainer on CPU
(tests/golden/make_golden_trainer_feature_grads.py): d losses[-1] / d base_feature for both head img_size variants, plus a run
with the proposals detached - as a fixed eighth of the elements, the whole map's max |g| and its float64 sums over channels and
over pixels (``match_fixture``; the full maps would be 3 MB).  ``restated_feature_grad`` is its float64 torch-autograd statement: the RPN's 1x1 convs, a RoIPool
by gather (differentiable; the arg-max chosen on the f32 map with torchvision's rule), the classifier's mean, the head's two
Linear layers and test_trainer_grads.chain_losses (the losses with the indirect term through the proposals).  The CPU tests
pin it to the fixture; the GPU tests measure the kernels and the trainer against it.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_trainer_grads import (A, N_CLASS, PARAMS, anchors, chain_losses, close, fixture_inputs, image,  # noqa: E402
                                reference_state_dict, t, trunk, z, zg)  # noqa: F401  (fixtures)

from feature_grads_restated import (FLT_MAX, _f32, _roundf, align_avg_grad_f64, pool_argmax, pool_avg_by_gather,  # noqa: E402,F401
                                    pool_avg_grad_f64, pool_bins, pool_bar, pool_grad_ref, roi_to_map)


@pytest.fixture(scope="module")
def zf(golden_dir):
    return np.load(os.path.join(golden_dir, "trainer_feature_grads_ref.npz"))


def match_fixture(g, zf, variant, frac, what="", detached=False):
    """g [1,C,h,w] against the fixture's record of d base_feature: the sampled elements within ``frac`` of the whole map's max
    |g|, the max itself, and the sums over channels / over pixels within ``frac`` of the matching sums of |g|."""
    g = g.detach().cpu().double()
    scale = float(zf[f"{variant}.d_feat_max"])
    key = f"{variant}.d_feat_detached_sample" if detached else f"{variant}.d_feat_sample"
    got = g.reshape(-1)[torch.from_numpy(zf["index"]).long()]
    err = float((got - torch.from_numpy(zf[key]).double()).abs().max())
    assert err <= frac * scale, (what, "sampled elements", err, scale)
    if detached:
        return
    assert abs(float(g.abs().max()) - scale) <= frac * scale, (what, "max |g|", float(g.abs().max()), scale)
    for key, dims in (("pixel_sum", 1), ("channel_sum", (2, 3))):
        want = torch.from_numpy(zf[f"{variant}.d_feat_{key}"])
        bound = frac * g.abs().sum(dims) + 1e-30
        assert ((g.sum(dims) - want).abs() <= bound).all(), (what, key, float(((g.sum(dims) - want).abs() / bound).max()))


# ------------------------------------------------------------------------------------------------------ the restatement
def restated_feature_grad(X, W, rois, img_hw, gt_rpn_loc, gt_rpn_label, gt_roi_label, anchor, roi_anchor, sample_src,
                          sample_gt, bbox, img_size, weights=(0, 0, 0, 0, 1), detach_rois=False):
    """float64 d (sum_k weights[k] loss_k) / d X for one image: X [1,C,h,w] the f32 feature map, W the reference parameters,
    rois [S,4] the sampled RoIs (image coords), img_hw the head's img_size (quirk Q2)."""
    C = X.shape[1]
    Xd = X.double().clone().requires_grad_(True)
    P = {k: W[k].detach().double().reshape(W[k].shape[0], -1).squeeze(-1) for k in PARAMS}
    rows = Xd[0].permute(1, 2, 0).reshape(-1, C)
    rpn_locs = (rows @ P["rpn.loc.weight"].T + P["rpn.loc.bias"]).reshape(-1, 4)
    rpn_scores = (rows @ P["rpn.score.weight"].T + P["rpn.score.bias"]).reshape(-1, 2)
    am = pool_argmax(X.float(), rois[None], [0], img_hw[0], img_hw[1])
    fc7 = pool_avg_by_gather(Xd, am)
    cls_locs = fc7 @ P["head.cls_loc.weight"].T + P["head.cls_loc.bias"]
    scores = fc7 @ P["head.score.weight"].T + P["head.score.bias"]
    losses = chain_losses(rpn_locs, rpn_scores, gt_rpn_loc, gt_rpn_label, cls_locs, scores, gt_roi_label, anchor, roi_anchor,
                          sample_src, sample_gt, bbox, img_size, detach_rois)
    losses.append(sum(losses))
    sum(w * l for w, l in zip(weights, losses) if w).backward()
    return Xd.grad


def head_hw(z, variant):
    C, H, W = z["img_u8"].shape
    return (C, H, W) if variant == "chw" else (H, W)


def fixture_case(z, zg, trunk, variant):
    f = fixture_inputs(z, zg, trunk, variant)
    f.pop("X")
    f.pop("fc7")
    return dict(X=trunk[0], W=reference_state_dict(), rois=t(z, "sample_roi"), img_hw=head_hw(z, variant), **f)


# ----------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_restated_feature_grad_reproduces_the_reference(z, zg, zf, trunk, variant):
    """float64 autograd over the oracle's feature map (the reference's, bit for bit) gives the reference's d base_feature."""
    assert int(zf["seed"]) == int(z["seed"])
    g = restated_feature_grad(**fixture_case(z, zg, trunk, variant))
    match_fixture(g, zf, variant, 1e-4, variant)
    if variant == "chw":
        gd = restated_feature_grad(detach_rois=True, **fixture_case(z, zg, trunk, variant))
        match_fixture(gd, zf, variant, 1e-4, "detached", detached=True)


def test_indirect_term_is_material_in_d_features(zf):
    """Detaching the proposals moves d base_feature by far more than the tolerance (1e-4 of max |g|): over the whole map (the
    generator's measure) and on the sampled elements alone."""
    for variant in ("chw", "hw"):
        assert float(zf[f"{variant}.indirect"]) >= 1e-3
    g, gd = t(zf, "chw.d_feat_sample"), t(zf, "chw.d_feat_detached_sample")
    assert float((g - gd).abs().max()) >= 1e-3 * float(zf["chw.d_feat_max"])


FEATURE_ENTRY_POINTS = ("tsod_roi_pool_avg_grad_workspace_bytes", "tsod_roi_pool_avg_grad_f32",
                        "tsod_roi_align_avg_grad_workspace_bytes", "tsod_roi_align_avg_grad_f32")


def test_feature_grad_entry_points_abi():
    """Declared in include/tsod.h, bound with as many arguments as declared, exported by the library."""
    import ctypes
    import re
    from two_stage_object_detection_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "tsod.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(tsod_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text)}
    for name in FEATURE_ENTRY_POINTS:
        assert name in decl and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(decl[name].split(",")) == len(_ffi._SIGNATURES[name][1]), name
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in FEATURE_ENTRY_POINTS:
        assert hasattr(raw, name), name
    lib = _ffi.lib()
    assert lib.tsod_roi_pool_avg_grad_workspace_bytes(2, 128, 512, 7, 7) == 2 * 128 * 16 + 2 * 128 * 49 * 512 * 2
    assert lib.tsod_roi_align_avg_grad_workspace_bytes(2, 128) == 2 * 128 * 16
    assert lib.tsod_roi_pool_avg_grad_workspace_bytes(0, 128, 512, 7, 7) == 0


def test_features_argument_is_keyword_only():
    import inspect
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    p = inspect.signature(FasterRCNNTrainer.forward).parameters["features"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


# ----------------------------------------------------------------------------------------------------------------- GPU
def random_case(B, C, Hf, Wf, R, img_hw, seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn((B, C, Hf, Wf), generator=g)
    H, W = img_hw
    xy = torch.rand((B, R, 2), generator=g) * torch.tensor([W * 1.1, H * 1.1]) - torch.tensor([W * 0.1, H * 0.1])
    wh = torch.rand((B, R, 2), generator=g) * torch.tensor([W * 0.6, H * 0.6]) + 1
    rois = torch.cat([xy, xy + wh], 2)
    d_out = torch.randn((B * R, C), generator=g)
    return feat, rois, d_out


def gpu_pool_grad(dev, feat, rois, roi_indices, img_hw, d_out, op="pool", pitch=None, **kw):
    from two_stage_object_detection_amd import hip_ops
    fn = hip_ops.nchw_to_nhwc(feat.to(dev), pitch)
    ri = torch.tensor(roi_indices, dtype=torch.int32, device=dev)
    if op == "pool":
        d = hip_ops.roi_pool_avg_grad_nhwc(fn, rois.to(dev), ri, img_hw[0], img_hw[1], d_out.to(dev), **kw)
    else:
        d = hip_ops.roi_align_avg_grad_nhwc(feat.shape[:1] + feat.shape[2:] + feat.shape[1:2], rois.to(dev), ri, img_hw[0],
                                            img_hw[1], d_out.to(dev), **kw)
    return d


def check_grad_kernel(dev, feat, rois, roi_indices, img_hw, d_out, op="pool", frac=2e-5):
    from two_stage_object_detection_amd import hip_ops
    got = gpu_pool_grad(dev, feat, rois, roi_indices, img_hw, d_out, op)
    again = gpu_pool_grad(dev, feat, rois, roi_indices, img_hw, d_out, op)
    assert torch.equal(got, again), "two runs differ"
    got = hip_ops.nhwc_to_nchw(got).cpu()
    if op == "pool":
        want = pool_avg_grad_f64(feat, rois, roi_indices, img_hw[0], img_hw[1], d_out)
    else:
        want = align_avg_grad_f64(tuple(feat.shape), rois, roi_indices, img_hw[0], img_hw[1], d_out)
    assert torch.isfinite(got).all()
    if float(want.abs().max()) == 0:
        assert (got == 0).all()
    else:
        close(got, want, frac, op)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["pool", "align"])
@pytest.mark.parametrize("C,Hf,Wf,img_hw", [(512, 20, 28, (320, 448)), (2048, 50, 84, (800, 1333))])
def test_pool_grad_kernels_random(dev, op, C, Hf, Wf, img_hw):
    """HarDNet (C = 512) and ResNet-50 (C = 2048) geometries, B = 2, roi_indices = [1, 0] (image 1's RoIs come first)."""
    R = 12 if op == "align" else 24
    feat, rois, d_out = random_case(2, C, Hf, Wf, R, img_hw, seed=C + Hf)
    check_grad_kernel(dev, feat, rois, [1, 0], img_hw, d_out, op)


def hand_rois(Hf, Wf, img_hw):
    """RoIs in image coords of a 16 x 16 map on a 48 x 64 image (3 px per map row, 4 per column): tiny (one pixel, Q2's y/3),
    partly and wholly off the map, one repeated, one whose bins share rows and columns."""
    H, W = img_hw
    sy, sx = H / Hf, W / Wf
    return torch.tensor([[0, 0, 0.4 * sx, 0.4 * sy],                          # one pixel
                         [-5 * sx, -5 * sy, 3 * sx, 2 * sy],                   # partly off the map
                         [20 * sx, 20 * sy, 30 * sx, 30 * sy],                 # wholly off: every bin empty
                         [2 * sx, 3 * sy, 12.4 * sx, 13.4 * sy],               # 11 px bins of 7: shared rows / columns
                         [2 * sx, 3 * sy, 12.4 * sx, 13.4 * sy],               # the same RoI again
                         [5 * sx, 5 * sy, 7 * sx, 6 * sy],                     # 3 x 2 px: bins repeat pixels
                         [14 * sx, 14 * sy, 17 * sx, 17 * sy],                 # over the far edge
                         [-3 * sx, 4 * sy, 1 * sx, 9 * sy]], dtype=torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["pool", "align"])
def test_pool_grad_kernels_hand_cases(dev, op):
    Hf, Wf, img_hw, C = 16, 16, (48, 64), 8
    g = torch.Generator().manual_seed(5)
    rois = torch.stack([hand_rois(Hf, Wf, img_hw), hand_rois(Hf, Wf, img_hw).flip(0)])
    d_out = torch.randn((2 * rois.shape[1], C), generator=g)
    # exact ties: a map of few distinct values (first maximum wins), plus -inf pixels (no arg-max where a bin has only them)
    feat = torch.randint(0, 3, (2, C, Hf, Wf), generator=g).float()
    feat[:, 0] = 1.0                                                           # channel 0: all tied
    feat[:, 1, :4, :4] = -float("inf")
    got, want = check_grad_kernel(dev, feat, rois, [0, 1], img_hw, d_out, op)
    if op == "pool":
        # channel 0: every non-empty bin sends its gradient to its top-left pixel
        am = pool_argmax(feat, rois, [0, 1], *img_hw)
        for k, b, idx in am:
            for ph, pw, hs, he, ws, we in pool_bins(roi_to_map(rois.reshape(-1, 4)[k].tolist(), *img_hw, Hf, Wf), Hf, Wf):
                if he > hs and we > ws:
                    assert int(idx[ph * 7 + pw, 0]) == hs * Wf + ws
        # the wholly-off RoI (k = 2) adds nothing: drop it and the gradient is unchanged
        d2 = d_out.clone()
        d2[2] = 0
        got2 = gpu_pool_grad(dev, feat, rois, [0, 1], img_hw, d2)
        from two_stage_object_detection_amd import hip_ops
        assert torch.equal(hip_ops.nhwc_to_nchw(got2).cpu(), got)


@pytest.mark.gpu
def test_pool_grad_accumulates_and_pitches(dev):
    """accumulate adds to d_feat in place; a pitched feature map and pitched d_out rows read the right channels."""
    from two_stage_object_detection_amd import hip_ops
    feat, rois, d_out = random_case(2, 64, 12, 14, 8, (96, 112), seed=3)
    ri = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    fpitched = hip_ops.nchw_to_nhwc(feat.to(dev), 72)
    dpitched = torch.zeros((16, 68), device=dev)
    dpitched[:, :64] = d_out.to(dev)
    base = torch.randn((2, 12, 14, 64), generator=torch.Generator().manual_seed(9)).to(dev)
    acc = base.clone()
    hip_ops.roi_pool_avg_grad_nhwc(fpitched, rois.to(dev), ri, 96, 112, dpitched[:, :64], d_feat=acc, accumulate=True)
    plain = gpu_pool_grad(dev, feat, rois, [1, 0], (96, 112), d_out)
    assert torch.equal(acc, base + plain)
    # Wf = 14 is no multiple of the 4-pixel strip: the ragged row end against the float64 restatement under its derived bar
    want, T, N = pool_grad_ref(feat, rois, [1, 0], 96, 112, d_out)
    got = hip_ops.nhwc_to_nchw(plain).cpu().double()
    assert bool(((got - want).abs() <= pool_bar(T, N)).all()) and bool((got[N == 0] == 0).all())
    acc = base.clone()
    hip_ops.roi_align_avg_grad_nhwc((2, 12, 14, 64), rois.to(dev), ri, 96, 112, dpitched[:, :64], d_feat=acc, accumulate=True)
    assert torch.equal(acc, base + gpu_pool_grad(dev, feat, rois, [1, 0], (96, 112), d_out, op="align"))


def feature_trainer(dev, variant="chw", roi_op="pool", head_grads=False):
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    tr = FasterRCNNTrainer(mode="train", num_classes=80, head_img_size=variant, roi_op=roi_op, head_grads=head_grads)
    tr.load_state_dict(reference_state_dict(), strict=True)
    return tr.to(dev).eval()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [56, 408])
def test_dgrad_gemms_vs_float64(dev, K):
    """d feat_rpn = d rpn_out . W_rpn (K = 56: 54 columns + 2 zero pad columns) and d fc7 = d both . W_head (K = 408)."""
    tr = feature_trainer(dev)
    g = torch.Generator().manual_seed(K)
    M = 1000 if K == 56 else 256
    n_real = 6 * A if K == 56 else 5 * N_CLASS
    dy = torch.zeros((M, K))
    dy[:, :n_real] = torch.randn((M, n_real), generator=g)
    W = reference_state_dict()
    if K == 56:
        Wf = torch.cat([W["rpn.loc.weight"].reshape(4 * A, -1), W["rpn.score.weight"].reshape(2 * A, -1)]).double()
        got = tr.rpn.input_grad(dy.to(dev), 1, 25, 40).reshape(M, -1).cpu()
    else:
        Wf = torch.cat([W["head.cls_loc.weight"], W["head.score.weight"]]).double()
        got = tr.head.fc7_grad(dy.to(dev)).cpu()
    want = dy[:, :n_real].double() @ Wf
    bound = dy[:, :n_real].double().abs() @ Wf.abs()
    assert ((got.double() - want).abs() <= 4e-6 * bound + 1e-30).all()
    again = tr.head.fc7_grad(dy.to(dev)).cpu() if K == 408 else tr.rpn.input_grad(dy.to(dev), 1, 25, 40).reshape(M, -1).cpu()
    assert torch.equal(got, again)


def oracle_features(trunk, dev):
    return trunk[0].clone().to(dev).requires_grad_(True)


def run_features(tr, z, feats, weights=(0, 0, 0, 0, 1), imgs=None):
    x = image(z)[None] if imgs is None else imgs
    bbox, label = t(z, "bbox").to(feats.device), t(z, "label").to(feats.device)
    losses = tr(x, [bbox] * x.shape[0], [label] * x.shape[0], features=feats)[0]
    return losses, sum(w * l for w, l in zip(weights, losses) if w)


def saved_of(losses):
    node = losses[-1].grad_fn
    while not hasattr(node, "saved"):
        node = node.next_functions[0][0]
    return node.saved


def restated_on_run(sv, W, z, variant, weights=(0, 0, 0, 0, 1), roi_op="pool"):
    """float64 d features on the GPU run's own intermediates: the restated losses of the kept rpn_out / both give d rpn_out /
    d both in float64 (test_trainer_grads.restated_on_run's chain), then d X = d rpn_out . W_rpn + pool backward(d both . W)."""
    import test_trainer_grads as tg
    Wd = {k: v.double() for k, v in W.items() if k in PARAMS}
    A_ = sv["A"]
    rpn_out, both = sv["rpn_out"].cpu().double(), sv["both"].cpu().double()
    rl = rpn_out[:, :4 * A_].clone().requires_grad_(True)
    rs = rpn_out[:, 4 * A_:6 * A_].clone().requires_grad_(True)
    cl = both[:, :4 * N_CLASS].clone().requires_grad_(True)
    sc = both[:, 4 * N_CLASS:5 * N_CLASS].clone().requires_grad_(True)
    roi_anchor = sv["sort_idx"][0].cpu().long()[sv["keep_idx"][0].cpu().long()]
    sroi = sv["sample_roi"][0].cpu().double()
    b = t(z, "bbox").double()
    tl = torch.maximum(sroi[:, None, :2], b[:, :2])
    br = torch.minimum(sroi[:, None, 2:], b[:, 2:])
    inter = (br - tl).clamp(min=0).prod(2)
    iou = inter / ((sroi[:, 2:] - sroi[:, :2]).prod(1)[:, None] + (b[:, 2:] - b[:, :2]).prod(1) - inter)
    losses = tg.chain_losses(rl.reshape(-1, 4), rs.reshape(-1, 2), sv["gt_loc"][0].cpu(), sv["gt_label"][0].cpu(), cl, sc,
                             sv["gt_roi_label"][0].cpu(), sv["anchor"].cpu(), roi_anchor, sv["sample_src"][0].cpu(),
                             iou.argmax(1), t(z, "bbox"), (3, sv["clamp_x"], sv["clamp_y"]))
    losses.append(sum(losses))
    sum(w * l for w, l in zip(weights, losses) if w).backward()
    feat = sv["feat"].cpu()                                                    # [1,h,w,C] NHWC, the run's own map
    n, h, w, C = feat.shape
    d_rows = rl.grad @ Wd["rpn.loc.weight"].reshape(4 * A_, C) + rs.grad @ Wd["rpn.score.weight"].reshape(2 * A_, C)
    d_x = d_rows.reshape(n, h, w, C).permute(0, 3, 1, 2)
    d_fc7 = cl.grad @ Wd["head.cls_loc.weight"] + sc.grad @ Wd["head.score.weight"]
    featc = feat.permute(0, 3, 1, 2).contiguous()
    hw = sv["head_size"]
    rois = sv["sample_roi"].cpu()
    if roi_op == "pool":
        return d_x + pool_avg_grad_f64(featc, rois, [0], hw[0], hw[1], d_fc7)
    return d_x + align_avg_grad_f64(tuple(featc.shape), rois, [0], hw[0], hw[1], d_fc7)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_trainer_feature_grad_end_to_end(dev, z, zg, zf, trunk, variant):
    """features = the oracle's map (the reference's bit for bit): torch.autograd.grad gives the reference's d base_feature
    within 1e-4 of max |g| (same f32 map: the arg-max choices are the reference's), and float64 autograd on the run's own
    intermediates within 2e-5."""
    tr = feature_trainer(dev, variant)
    feats = oracle_features(trunk, dev)
    losses, total = run_features(tr, z, feats)
    torch.testing.assert_close(torch.stack([l.detach() for l in losses]).cpu(), t(z, f"{variant}.losses"), rtol=1e-4, atol=0)
    (g,) = torch.autograd.grad(total, feats)
    assert g.shape == feats.shape and g.dtype == torch.float32
    match_fixture(g, zf, variant, 1e-4, "fixture")
    want = restated_on_run(saved_of(losses), reference_state_dict(), z, variant)
    close(g.cpu(), want, 2e-5, "float64")
    assert all(p.grad is None for p in tr.parameters())


@pytest.mark.gpu
def test_trainer_feature_grad_align(dev, z, trunk):
    tr = feature_trainer(dev, "hw", roi_op="align")
    feats = oracle_features(trunk, dev)
    losses, total = run_features(tr, z, feats)
    (g,) = torch.autograd.grad(total, feats)
    close(g.cpu(), restated_on_run(saved_of(losses), reference_state_dict(), z, "hw", roi_op="align"), 2e-5, "align")


@pytest.mark.gpu
def test_trainer_feature_grad_linearity_and_saved_state(dev, z, trunk):
    tr = feature_trainer(dev)
    feats = oracle_features(trunk, dev)
    per = []
    for k in range(4):
        _, tot = run_features(tr, z, feats, weights=tuple(1 if i == k else 0 for i in range(5)))
        per.append(torch.autograd.grad(tot, feats)[0])
    first, tot = run_features(tr, z, feats, weights=(0.5, 0, 0, 2, 1 / 32))
    run_features(tr, z, (feats.detach() * 0.5).requires_grad_(True))          # a later forward before the backward
    got = torch.autograd.grad(tot, feats)[0]
    want = 0.5 * per[0] + 2 * per[3] + (per[0] + per[1] + per[2] + per[3]) / 32
    close(got, want, 1e-5, "linearity")
    _, tot = run_features(tr, z, feats, weights=(0.5, 0, 0, 2, 1 / 32))
    assert torch.equal(torch.autograd.grad(tot, feats)[0], got)               # bit-identical run to run


@pytest.mark.gpu
def test_trainer_feature_grad_batch_mean(dev, z, trunk):
    tr = feature_trainer(dev)
    f1 = trunk[0].to(dev)
    f2 = (trunk[0] * 0.9).to(dev)
    singles = []
    for f in (f1, f2):
        x = f.clone().requires_grad_(True)
        singles.append(torch.autograd.grad(run_features(tr, z, x)[1], x)[0])
    both = torch.cat([f1, f2]).requires_grad_(True)
    imgs = torch.stack([image(z), image(z)])
    g = torch.autograd.grad(run_features(tr, z, both, imgs=imgs)[1], both)[0]
    close(g[0:1], singles[0] / 2, 1e-5, "image 0")
    close(g[1:2], singles[1] / 2, 1e-5, "image 1")


@pytest.mark.gpu
def test_trainer_features_head_grads_flag(dev, z, trunk):
    """head_grads=False: d features only, no .grad written.  head_grads=True: the eight .grad tensors are the ones the
    same features give through the frozen-backbone path's node (section 4.12), and d features is still returned."""
    import test_trainer_grads as tg
    tr = feature_trainer(dev)
    feats = oracle_features(trunk, dev)
    losses, tot = run_features(tr, z, feats)
    tot.backward()
    assert feats.grad is not None and all(p.grad is None for p in tr.parameters())
    sv = saved_of(losses)
    assert "rpn_wt" in sv and sv["feat"].shape[-1] == 512
    trh = feature_trainer(dev, head_grads=True)
    f2 = oracle_features(trunk, dev)
    losses, tot = run_features(trh, z, f2)
    tot.backward()
    assert torch.equal(f2.grad, feats.grad)
    got = tg.head_grads(trh)
    want = tg.restated_on_run(saved_of(losses), {k: v for k, v in reference_state_dict().items() if k in PARAMS}, t(z, "bbox"))
    for k in PARAMS:
        close(got[k].cpu(), want[k], 2e-5, k)


@pytest.mark.gpu
def test_trainer_features_trains_a_torch_backbone(dev, z):
    """A torch nn.Conv2d producing the features from the image gets the float64 chain's .weight.grad."""
    tr = feature_trainer(dev)
    g = torch.Generator().manual_seed(11)
    conv = torch.nn.Conv2d(3, 512, 16, stride=16).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.02)
        conv.bias.zero_()
    x = image(z)[None].to(dev)
    feats = conv(x)
    losses, tot = run_features(tr, z, feats)
    tot.backward()
    got = conv.weight.grad.cpu().double()
    d_feat = restated_on_run(saved_of(losses), reference_state_dict(), z, "chw")
    w64 = conv.weight.detach().cpu().double().requires_grad_(True)
    y = torch.nn.functional.conv2d(x.cpu().double(), w64, conv.bias.detach().cpu().double(), stride=16)
    (y * d_feat).sum().backward()
    close(got, w64.grad, 1e-4, "conv weight")


@pytest.mark.gpu
def test_trainer_features_none_is_unchanged(dev, z):
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    tr = FasterRCNNTrainer(mode="train", num_classes=80)
    tr.load_state_dict(reference_state_dict(), strict=True)
    tr = tr.to(dev).eval()
    x, bbox, label = image(z)[None].to(dev), t(z, "bbox").to(dev), t(z, "label").to(dev)
    a = tr(x, [bbox], [label])[0]
    b = tr(x, [bbox], [label], features=None)[0]
    assert not any(l.requires_grad for l in b)
    assert torch.equal(torch.stack(a), torch.stack(b))
    torch.testing.assert_close(torch.stack(b).cpu(), t(z, "chw.losses"), rtol=1e-4, atol=0)


@pytest.mark.gpu
def test_trainer_features_validation(dev, z, trunk):
    tr = feature_trainer(dev)
    x, bbox, label = image(z)[None], t(z, "bbox").to(dev), t(z, "label").to(dev)
    f = trunk[0].to(dev)
    with pytest.raises(ValueError, match="features must be"):
        tr(x, [bbox], [label], features=f[:, :256])
    with pytest.raises(ValueError, match="features must be"):
        tr(torch.stack([x[0], x[0]]), [bbox, bbox], [label, label], features=f)
    with pytest.raises(TypeError, match="float32"):
        tr(x, [bbox], [label], features=f.double())
    with pytest.raises(Exception):
        tr(x, [bbox], [label], features=trunk[0])                              # CPU tensor
    # any strides: a channels-last view gives the same losses as the contiguous map
    cl = f.to(memory_format=torch.channels_last)
    with torch.no_grad():
        assert torch.equal(torch.stack(tr(x, [bbox], [label], features=cl)[0]), torch.stack(tr(x, [bbox], [label], features=f)[0]))
