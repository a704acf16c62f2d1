"""FasterRCNNTrainer (nets/frcnn_training.py:179-342): the ground-truth-conditioned forward and its four losses.

tests/golden/trainer_ref.npz was made by the REFERENCE's own FasterRCNNTrainer on CPU (tests/golden/make_golden_trainer.py):
seeded HarDNet-39 weights with conditioned BatchNorm, one 3x320x448 image, three ground-truth boxes, run once as the
reference wires it (head img_size = (C,H,W), quirk Q2) and once with the head given (H,W).  ``restated_losses`` below is
the torch-CPU statement of the reference's loss arithmetic the GPU tests measure against; the CPU tests pin it to the
fixture first.
"""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from trainer_losses_restated import loc_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLASS = 81
A = 9


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "trainer_ref.npz"))


def t(z, k):
    return torch.from_numpy(z[k])


def image(z):
    return torch.from_numpy(z["img_u8"]).float() / 255


def reference_state_dict():
    """The fixture's weights under the reference trainer's key names (``feat_extra.`` for the backbone)."""
    from two_stage_object_detection_amd.testing import synthetic_detector
    _, sd = synthetic_detector("hardnet39", conditioned=True)
    return {("feat_extra." + k[len("extractor."):] if k.startswith("extractor.") else k): v for k, v in sd.items()}


def restated_losses(rpn_locs, rpn_scores, gt_rpn_loc, gt_rpn_label, roi_cls_locs, roi_scores, gt_roi_loc, gt_roi_label,
                    dtype=torch.float64):
    """One image: [rpn_loc, rpn_cls, roi_loc, roi_cls] (nets/frcnn_training.py:262-274, 300-331) in ``dtype``."""
    c = lambda v: v.to(dtype)                                                          # noqa: E731
    S = roi_scores.shape[0]
    roi_loc = c(roi_cls_locs).view(S, -1, 4)[torch.arange(S), gt_roi_label]
    return [loc_loss(c(rpn_locs), c(gt_rpn_loc), gt_rpn_label),
            F.cross_entropy(c(rpn_scores), gt_rpn_label, ignore_index=-1),
            loc_loss(roi_loc, c(gt_roi_loc), gt_roi_label),
            F.cross_entropy(c(roi_scores), gt_roi_label)]


def fixture_losses(z, variant, dtype=torch.float64):
    return restated_losses(t(z, "rpn_locs")[0], t(z, "rpn_scores")[0], t(z, "gt_rpn_loc"), t(z, "gt_rpn_label"),
                           t(z, f"{variant}.roi_cls_locs")[0], t(z, f"{variant}.roi_scores")[0], t(z, "gt_roi_loc"),
                           t(z, "gt_roi_label"), dtype)


def rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-30)


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_state_dict_is_the_reference_trainers(z):
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    sd = FasterRCNNTrainer(mode="train", num_classes=80).state_dict()
    got = [(k, tuple(v.shape)) for k, v in sd.items()]
    want = [(str(k), ast.literal_eval(str(s))) for k, s in zip(z["sd_names"], z["sd_shapes"])]
    assert sorted(got) == sorted(want)


def test_reference_weights_load_strict_without_renaming(z):
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    from two_stage_object_detection_amd.testing import weights_checksum
    sd = reference_state_dict()
    assert abs(weights_checksum({"extractor." + k[len("feat_extra."):]: v for k, v in sd.items()
                                 if k.startswith("feat_extra.")}) - float(z["weights_checksum"])) <= 1e-6 * float(z["weights_checksum"])
    FasterRCNNTrainer(mode="train", num_classes=80).load_state_dict(sd, strict=True)


@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_restated_losses_reproduce_the_reference(z, variant):
    want = t(z, f"{variant}.losses")
    f32 = fixture_losses(z, variant, torch.float32)
    f64 = fixture_losses(z, variant, torch.float64)
    for i in range(4):
        assert rel(f32[i], want[i]) <= 1e-6, (i, float(f32[i]), float(want[i]))
        assert rel(f64[i], want[i]) <= 1e-6, (i, float(f64[i]), float(want[i]))
    assert rel(sum(f32), want[4]) <= 1e-6
    # the predictions: loc2bbox of the gt class's offsets, arg-max / max of the raw logits
    import oracle
    S = 128
    sc = t(z, f"{variant}.roi_scores")[0]
    roi_loc = t(z, f"{variant}.roi_cls_locs")[0].view(S, -1, 4)[torch.arange(S), t(z, "gt_roi_label")]
    assert torch.equal(oracle.loc2bbox(t(z, "sample_roi"), roi_loc), t(z, f"{variant}.anchors_pred")[0])
    assert torch.equal(sc.argmax(1), t(z, f"{variant}.classes_pred")[0])
    assert torch.equal(sc.max(1).values, t(z, f"{variant}.classes_score_pred")[0])
    for k in ("sample_roi", "gt_roi_loc", "gt_roi_label", "rpn_locs"):
        assert np.isfinite(z[k]).all() if z[k].dtype.kind == "f" else True


def test_dropin_resolves_the_hip_trainer():
    code = ("import two_stage_object_detection_amd as p; p.install_dropin()\n"
            "from nets.frcnn_training import FasterRCNNTrainer\n"
            "from two_stage_object_detection_amd.nets import frcnn_training\n"
            "assert FasterRCNNTrainer is frcnn_training.FasterRCNNTrainer\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_training_mode_raises():
    from two_stage_object_detection_amd._ffi import TsodError
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    tr = FasterRCNNTrainer(mode="train", num_classes=80)
    with pytest.raises(TsodError, match="eval"):
        tr(torch.zeros(1, 3, 64, 64), [torch.zeros(0, 4)], [torch.zeros(0, dtype=torch.int64)])
    with pytest.raises(ValueError):
        FasterRCNNTrainer(mode="train", num_classes=80, head_img_size="wh")


# ----------------------------------------------------------------------------------------------------------------- GPU
def pitched_rpn(z, dev):
    """The fixture's RPN outputs laid out like the fused conv's output: [h*w, 56], loc in [0,36), logits in [36,54), the
    two pad columns NaN (a read of them would poison the losses)."""
    locs, scores = t(z, "rpn_locs")[0], t(z, "rpn_scores")[0]
    P = locs.shape[0] // A
    buf = torch.full((P, 56), float("nan"))
    buf[:, :4 * A] = locs.reshape(P, 4 * A)
    buf[:, 4 * A:6 * A] = scores.reshape(P, 2 * A)
    return buf.to(dev)


def pitched_head(z, variant, dev, rows=None):
    """The fixture's head outputs as column views of one [S, 408] matrix, pad columns NaN."""
    cl, sc = t(z, f"{variant}.roi_cls_locs")[0], t(z, f"{variant}.roi_scores")[0]
    S = cl.shape[0]
    buf = torch.full((S, 408), float("nan"))
    buf[:, :4 * N_CLASS] = cl
    buf[:, 4 * N_CLASS:5 * N_CLASS] = sc
    buf = buf.to(dev)
    return buf[:, :4 * N_CLASS].view(1, S, 4 * N_CLASS), buf[:, 4 * N_CLASS:5 * N_CLASS].view(1, S, N_CLASS)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_loss_kernels_on_reference_intermediates(dev, z, variant):
    from two_stage_object_detection_amd import hip_ops
    want = t(z, f"{variant}.losses")
    f64 = fixture_losses(z, variant)
    rpn, st = hip_ops.rpn_losses(pitched_rpn(z, dev), A, t(z, "gt_rpn_loc")[None].to(dev), t(z, "gt_rpn_label")[None].to(dev))
    cl, sc = pitched_head(z, variant, dev)
    assert cl.stride(1) == 408
    ap, cp, csp, roi, st2 = hip_ops.roi_losses(cl, sc, t(z, "sample_roi")[None].to(dev), t(z, "gt_roi_loc")[None].to(dev),
                                               t(z, "gt_roi_label")[None].to(dev))
    got = torch.cat([rpn[0], roi[0]]).cpu()
    assert int(st.item()) == 0 and int(st2.item()) == 0
    for i in range(4):
        assert rel(got[i], want[i]) <= 1e-6, (i, float(got[i]), float(want[i]))
        assert rel(got[i], f64[i]) <= 1e-6, (i, float(got[i]), float(f64[i]))
    S = 128
    lab = t(z, "gt_roi_label")
    gathered = t(z, f"{variant}.roi_cls_locs")[0].view(S, -1, 4)[torch.arange(S), lab].contiguous()
    same_decode = hip_ops.loc2bbox(t(z, "sample_roi").to(dev), gathered.to(dev))
    assert torch.equal(ap[0], same_decode)
    assert float((ap[0].cpu() - t(z, f"{variant}.anchors_pred")[0]).abs().max()) <= 1e-3
    assert cp.dtype == torch.int64 and torch.equal(cp[0].cpu(), t(z, f"{variant}.classes_pred")[0])
    assert torch.equal(csp[0].cpu(), t(z, f"{variant}.roi_scores")[0][torch.arange(S), cp[0].cpu()])


@pytest.mark.gpu
def test_loss_kernel_edge_cases(dev, z):
    from two_stage_object_detection_amd import hip_ops
    fused = pitched_rpn(z, dev)
    gl = t(z, "gt_rpn_loc")[None].to(dev)
    lab = t(z, "gt_rpn_label")[None].to(dev)
    out, _ = hip_ops.rpn_losses(fused, A, gl, torch.where(lab == 1, torch.zeros_like(lab), lab))      # no positive
    assert torch.isnan(out[0, 0]) and torch.isfinite(out[0, 1])
    out, _ = hip_ops.rpn_losses(fused, A, gl, torch.full_like(lab, -1))                             # every anchor ignored
    assert torch.isnan(out[0, 0]) and torch.isnan(out[0, 1])
    cl, sc = pitched_head(z, "hw", dev)
    s_roi, s_loc = t(z, "sample_roi")[None].to(dev), t(z, "gt_roi_loc")[None].to(dev)
    rlab = t(z, "gt_roi_label")[None].to(dev)
    out = hip_ops.roi_losses(cl, sc, s_roi, s_loc, torch.zeros_like(rlab))[3]                       # no positive RoI
    assert torch.isnan(out[0, 0]) and torch.isfinite(out[0, 1])
    # an out-of-range class: counted, never used as an index; the other rows are untouched
    for bad in (N_CLASS, -1, 1 << 40):
        lab_bad = rlab.clone()
        lab_bad[0, 5] = bad
        ap, cp, _, out, st = hip_ops.roi_losses(cl, sc, s_roi, s_loc, lab_bad)
        ap_ok = hip_ops.roi_losses(cl, sc, s_roi, s_loc, rlab)[0]
        assert int(st.item()) == 1
        assert torch.isnan(ap[0, 5]).all()
        keep = torch.arange(128, device=dev) != 5
        assert torch.equal(ap[0, keep], ap_ok[0, keep])
    lab_bad = lab.clone()
    lab_bad[0, 3] = 2
    assert int(hip_ops.rpn_losses(fused, A, gl, lab_bad)[1].item()) == 1
    # B = 2, different inputs per image: each image's result is its B = 1 result, bit for bit
    g = torch.Generator().manual_seed(5)
    lab2 = torch.randint(-1, 2, lab.shape, generator=g).to(dev)
    gl2 = (torch.randn(gl.shape, generator=g) * 0.3).to(dev)
    fused2 = torch.cat([fused, fused.flip(0) * 0.5])
    both, _ = hip_ops.rpn_losses(fused2, A, torch.cat([gl, gl2]), torch.cat([lab, lab2]))
    one0, _ = hip_ops.rpn_losses(fused, A, gl, lab)
    one1, _ = hip_ops.rpn_losses(fused2[fused.shape[0]:], A, gl2, lab2)
    assert torch.equal(both, torch.cat([one0, one1]))
    buf = torch.cat([cl.reshape(128, -1), sc.reshape(128, -1)], 1)
    buf2 = torch.cat([buf, buf.flip(0)])
    rlab2 = torch.randint(0, N_CLASS, rlab.shape, generator=g).to(dev)
    args2 = (buf2[:, :4 * N_CLASS].reshape(2, 128, -1), buf2[:, 4 * N_CLASS:].reshape(2, 128, -1), torch.cat([s_roi, s_roi.flip(1)]),
             torch.cat([s_loc, s_loc]), torch.cat([rlab, rlab2]))
    r2 = hip_ops.roi_losses(*args2)
    for b in range(2):
        r1 = hip_ops.roi_losses(*(a[b:b + 1] for a in args2))
        for x2, x1 in zip(r2, r1):
            assert torch.equal(x2[b:b + 1], x1)
    again = hip_ops.roi_losses(*args2)                                                               # two runs: same bits
    for x, y in zip(r2, again):
        assert torch.equal(x, y)
    assert torch.equal(hip_ops.rpn_losses(fused2, A, torch.cat([gl, gl2]), torch.cat([lab, lab2]))[0], both)


class Capture:
    """Keeps what the trainer's target creators returned (per image)."""

    def __init__(self, tr):
        self.gt_rpn_label, self.gt_roi_label, self.sample_roi = [], [], []
        atc, ptc = tr.anchor_target_creator, tr.proposal_target_creator

        def a(bbox, anchor):
            loc, label = atc(bbox, anchor)
            self.gt_rpn_label.append(label)
            return loc, label

        def p(roi, bbox, label, std):
            out = ptc(roi, bbox, label, std)
            self.sample_roi.append(out[0])
            self.gt_roi_label.append(out[2])
            return out
        a.n_sample, p.n_sample = atc.n_sample, ptc.n_sample
        tr.anchor_target_creator, tr.proposal_target_creator = a, p


def make_trainer(dev, head_img_size="chw"):
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    tr = FasterRCNNTrainer(mode="train", num_classes=80, head_img_size=head_img_size)
    tr.load_state_dict(reference_state_dict(), strict=True)
    return tr.to(dev).eval()


def oracle_composition(z, variant):
    """The reference's forward composed from the CPU oracle's functions and ``restated_losses`` (f32)."""
    from oracle import box, targets
    from oracle.detector import extractor_forward
    sd = {("extractor." + k[len("feat_extra."):] if k.startswith("feat_extra.") else k): v for k, v in reference_state_dict().items()}
    x = image(z)[None]
    bbox, label = t(z, "bbox"), t(z, "label")
    with torch.inference_mode():
        feat = extractor_forward(sd, x, "hardnet39")
        locs, scores, rois, anchor = box.rpn_forward(sd, feat, tuple(x.shape[1:]), mode="train", prefix="rpn.")
        gt_loc, gt_label = targets.anchor_targets(bbox, anchor[0])
        s_roi, s_loc, s_lab = targets.proposal_targets(rois[0], bbox, label)
        size = tuple(x.shape[1:]) if variant == "chw" else tuple(x.shape[2:])
        cl, sc = box.roi_head_forward(sd, feat, s_roi[None], torch.zeros(1, dtype=torch.int32), size, prefix="head.")
        losses = restated_losses(locs[0], scores[0], gt_loc, gt_label, cl[0], sc[0], s_loc, s_lab, torch.float32)
        S = s_roi.shape[0]
        ap = box.loc2bbox(s_roi, cl[0].view(S, -1, 4)[torch.arange(S), s_lab])
    return dict(losses=torch.stack(losses + [sum(losses)]), gt_rpn_label=gt_label, gt_roi_label=s_lab,
                anchors_pred=ap, classes_pred=sc[0].argmax(1))


def check_against(got, want, cap=None):
    if cap is not None:
        assert torch.equal(cap.gt_rpn_label[0].cpu(), want["gt_rpn_label"])
        assert torch.equal(cap.gt_roi_label[0].cpu(), want["gt_roi_label"])
    losses, ap, cp = got
    assert torch.equal(cp[0].cpu(), want["classes_pred"])
    assert float((ap[0].cpu() - want["anchors_pred"]).abs().max()) <= 1e-3
    for i in range(5):
        assert rel(losses[i], want["losses"][i]) <= 1e-4, (i, float(losses[i]), float(want["losses"][i]))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["chw", "hw"])
def test_trainer_end_to_end(dev, z, variant):
    tr = make_trainer(dev, variant)
    cap = Capture(tr)
    bbox, label = t(z, "bbox"), t(z, "label")
    with torch.inference_mode():
        losses, ap, cp, csp, bb0, lab0 = tr(image(z)[None].to(dev), [bbox.to(dev)], [label.to(dev)])
    torch.cuda.synchronize()
    assert len(losses) == 5 and all(l.dim() == 0 and l.is_cuda for l in losses)
    assert ap.shape == (1, 128, 4) and cp.shape == (1, 128) and cp.dtype == torch.int64 and csp.shape == (1, 128)
    assert torch.equal(bb0.cpu(), bbox[None]) and torch.equal(lab0.cpu(), (label + 1)[None])
    fixture = {"losses": t(z, f"{variant}.losses"), "gt_rpn_label": t(z, "gt_rpn_label"), "gt_roi_label": t(z, "gt_roi_label"),
               "anchors_pred": t(z, f"{variant}.anchors_pred")[0], "classes_pred": t(z, f"{variant}.classes_pred")[0]}
    check_against((losses, ap, cp), fixture, cap)
    check_against((losses, ap, cp), oracle_composition(z, variant), cap)
    # a list of [3,H,W] images is the same call
    with torch.inference_mode():
        again = tr([image(z).to(dev)], [bbox.to(dev)], [label.to(dev)])
    assert all(torch.equal(a, b) for a, b in zip(again[0], losses)) and torch.equal(again[1], ap)


@pytest.mark.gpu
def test_trainer_errors(dev, z):
    tr = make_trainer(dev)
    x, bbox = image(z)[None].to(dev), t(z, "bbox").to(dev)
    with torch.inference_mode():
        with pytest.raises(IndexError):                      # class 80 + 1 = 81 is outside the head's 81 logits
            tr(x, [bbox], [torch.tensor([3, 80, 7], device=dev)])
        tr.proposal_target_creator.n_sample = 1000           # more than the 600 proposals + 3 boxes can give
        with pytest.raises(RuntimeError, match="n_sample"):
            tr(x, [bbox], [t(z, "label").to(dev)])


@pytest.mark.gpu
def test_checkpoint_round_trip(dev, z, tmp_path):
    tr = make_trainer(dev)
    x, bbox, label = image(z)[None].to(dev), t(z, "bbox").to(dev), t(z, "label").to(dev)
    with torch.inference_mode():
        out1 = tr(x, [bbox], [label])
    path = tmp_path / "FasterRCNNTrainer_best.pth"
    torch.save({"model_state_dict": tr.state_dict(), "epoch": 0}, path)
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    fresh = FasterRCNNTrainer(mode="train", num_classes=80, feat_stride=16, anchor_scales=[8, 16, 32], ratios=[0.5, 1, 2]).to(dev)
    fresh.load_state_dict(torch.load(path, map_location=dev, weights_only=True)["model_state_dict"], strict=True)
    fresh.eval()
    with torch.inference_mode():
        out2 = fresh(x, [bbox], [label])
    assert all(torch.equal(a, b) for a, b in zip(out1[0], out2[0]))
    for a, b in zip(out1[1:], out2[1:]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_batch_of_two_is_two_single_images(dev, z):
    tr = make_trainer(dev)
    x = image(z).to(dev)
    bbox, label = t(z, "bbox").to(dev), t(z, "label").to(dev)
    gts = [(bbox, label), (bbox[:2].clone(), label[:2].clone())]          # same image, another ground truth (G = 3, 2)
    with torch.inference_mode():
        singles = [tr(x[None], [b], [l]) for b, l in gts]
        both = tr(torch.stack([x, x]), [b for b, _ in gts], [l for _, l in gts])
    for i in range(5):
        mean = (float(singles[0][0][i]) + float(singles[1][0][i])) / 2
        assert rel(both[0][i], mean) <= 1e-4, (i, float(both[0][i]), mean)
    for b in range(2):
        assert torch.equal(both[2][b], singles[b][2][0])
        assert float((both[1][b] - singles[b][1][0]).abs().max()) <= 1e-3
