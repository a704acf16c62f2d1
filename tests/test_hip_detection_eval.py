"""The HIP detection evaluator (csrc/eval_metrics.hip, utils/metrics.py, FasterRCNNTrainer.eval_fn) against the numpy
restatement of tests/test_detection_eval.py."""
import numpy as np
import pytest
import torch

import oracle
from test_detection_eval import evaluate_np
from test_trainer import image, make_trainer, t, z  # noqa: F401 (z: the trainer fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ radix sort
@pytest.mark.parametrize("n", [1, 63, 4097, 100_003, 4_000_000])
def test_radix_sort_is_numpys_stable_argsort(dev, n):
    from two_stage_object_detection_amd import hip_ops
    rng = np.random.default_rng(n)
    few = (rng.integers(0, 7, n, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 3, n, dtype=np.uint64)   # many equal keys
    full = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    for keys, bits in ((few, (0, 35)), (full, (0, 64))):
        k_out, v_out = hip_ops.sort_pairs_u64(torch.from_numpy(keys.view(np.int64)).to(dev), None, *bits)
        want = np.argsort(keys, kind="stable")
        assert np.array_equal(v_out.cpu().numpy(), want)
        assert np.array_equal(k_out.cpu().numpy().view(np.uint64), keys[want])


def test_radix_sort_live_count_on_the_device(dev):
    from two_stage_object_detection_amd import hip_ops
    keys = np.random.default_rng(5).integers(0, 1000, 10_000).astype(np.int64)
    n_dev = torch.tensor([6_000], dtype=torch.int64, device=dev)
    _, v = hip_ops.sort_pairs_u64(torch.from_numpy(keys).to(dev), None, 0, 16, n_dev=n_dev)
    assert np.array_equal(v[:6_000].cpu().numpy(), np.argsort(keys[:6_000], kind="stable"))


# ------------------------------------------------------------------------------------------------------- random datasets
def random_dataset(seed, n_images, n_classes, max_gt, max_det, batch_sizes):
    """Batches of images (det [n,6], gt boxes [G,4], gt labels [G]) with quantized scores (ties), degenerate boxes, jittered
    duplicates of the ground truth, NaN scores and out-of-range classes."""
    rng = np.random.default_rng(seed)
    images = []
    for _ in range(n_images):
        G = int(rng.integers(0, max_gt + 1))
        xy = rng.uniform(0, 500, (G, 2)).astype(np.float32)
        wh = rng.uniform(0, 120, (G, 2)).astype(np.float32)
        wh[rng.random(G) < .05] = 0                                           # degenerate ground truth
        gb = np.concatenate([xy, xy + wh], 1)
        gl = rng.integers(0, n_classes, G)
        n = int(rng.integers(0, max_det + 1))
        d = np.zeros((n, 6), np.float32)
        src = rng.integers(0, max(G, 1), n)
        hit = (rng.random(n) < .6) & (G > 0)
        jitter = rng.normal(0, 6, (n, 4)).astype(np.float32)
        xy2 = rng.uniform(0, 500, (n, 2)).astype(np.float32)
        rand_boxes = np.concatenate([xy2, xy2 + rng.uniform(0, 120, (n, 2)).astype(np.float32)], 1)
        d[:, :4] = np.where(hit[:, None], (gb[src] if G else rand_boxes) + jitter, rand_boxes)
        deg = rng.random(n) < .03
        d[deg, 2] = d[deg, 0]                                                 # zero-width detections
        d[:, 4] = np.round(rng.random(n) * 20) / 20                           # quantized: many equal scores
        d[:, 5] = np.where(hit, gl[src] if G else 0, rng.integers(0, n_classes, n))
        d[rng.random(n) < .01, 4] = np.nan
        d[rng.random(n) < .01, 5] = n_classes + 3
        images.append((d, gb, gl))
    batches, i = [], 0
    while i < n_images:
        b = int(batch_sizes[len(batches) % len(batch_sizes)])
        batches.append(images[i:i + b])
        i += b
    return batches


def padded(batch, dev):
    R = max(1, max(d.shape[0] for d, _, _ in batch))
    G = max(1, max(g.shape[0] for _, g, _ in batch))
    det = np.zeros((len(batch), R, 6), np.float32)
    gb = np.zeros((len(batch), G, 4), np.float32)
    gl = np.full((len(batch), G), -1, np.int64)
    for b, (d, g, l) in enumerate(batch):
        det[b, :len(d)], gb[b, :len(g)], gl[b, :len(l)] = d, g, l
    counts = torch.tensor([len(d) for d, _, _ in batch], dtype=torch.int32, device=dev)
    return torch.from_numpy(det).to(dev), counts, torch.from_numpy(gb).to(dev), torch.from_numpy(gl).to(dev)


def run_hip(batches, n_classes, dev, **kw):
    from two_stage_object_detection_amd.utils.metrics import DetectionEvaluator
    ev = DetectionEvaluator(n_classes, **kw)
    for batch in batches:
        det, counts, gb, gl = padded(batch, dev)
        ev.update(det, gb, gl, counts=counts)
    return ev


def check_equal(ev, got, want):
    s, c, m = ev.records()
    assert np.array_equal(c, want["cls"]) and np.array_equal(m, want["mask"])
    assert np.array_equal(s, want["score"])
    assert np.array_equal(got["npig"].numpy(), want["npig"])
    for k in ("TP", "FP", "FN"):
        assert np.array_equal(got[k].numpy(), want[k]), k
    assert np.abs(got["AP"].numpy() - want["AP"]).max() <= 1e-12
    assert np.abs(got["recall"].numpy() - want["recall"]).max() <= 1e-12
    assert abs(got["mAP"] - want["mAP"]) <= 1e-12


@pytest.mark.parametrize("seed,n_images,n_classes,max_gt,max_det,batch_sizes,kw", [
    (0, 40, 3, 6, 30, (16, 7), dict(iou_thresholds=(.5, .75))),
    (1, 64, 5, 70, 300, (16,), dict(max_dets=20)),
    (2, 5000, 80, 12, 40, (64, 16, 33), dict()),                                    # COCO-sized, several update calls
])
def test_evaluator_matches_the_restatement(dev, seed, n_images, n_classes, max_gt, max_det, batch_sizes, kw):
    batches = random_dataset(seed, n_images, n_classes, max_gt, max_det, batch_sizes)
    ev = run_hip(batches, n_classes, dev, **kw)
    got = ev.compute()
    want = evaluate_np(batches, n_classes, kw.get("iou_thresholds", np.linspace(.5, .95, 10)), kw.get("max_dets", 100))
    check_equal(ev, got, want)
    again = run_hip(batches, n_classes, dev, **kw).compute()                          # two runs: identical bits
    assert np.array_equal(got["AP"].numpy().view(np.int64), again["AP"].numpy().view(np.int64))
    assert got["mAP"] == again["mAP"] and (got.get("AP50") == again.get("AP50"))


def test_input_forms_agree(dev):
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.utils.metrics import DetectionEvaluator
    batch = random_dataset(7, 12, 4, 8, 60, (12,))[0]
    det, counts, gb, gl = padded(batch, dev)
    det_sorted, keep, n_kept = hip_ops.filter_detections(det, iou_thr=.6, per_class=True)
    ns = n_kept.tolist()
    rows = [det_sorted[b][keep[b, :ns[b]].long()] for b in range(det.shape[0])]
    gtb = [torch.from_numpy(g).to(dev) for _, g, _ in batch]
    gtl = [torch.from_numpy(l).to(dev) for _, _, l in batch]
    a, b, c = (DetectionEvaluator(4) for _ in range(3))
    a.update(det_sorted, gtb, gtl, keep=keep, n_kept=n_kept)
    b.update(rows, gtb, gtl)
    c.update(torch.nn.utils.rnn.pad_sequence(rows, batch_first=True), gb, gl, counts=n_kept)
    ra, rb, rc = a.compute(), b.compute(), c.compute()
    for k in ("AP", "TP", "FP", "FN", "npig"):
        assert torch.equal(ra[k], rb[k]) and torch.equal(ra[k], rc[k]), k
    assert ra["mAP"] == rb["mAP"] == rc["mAP"]
    assert ra["AP50"] == rb["AP50"] and "AP75" in ra


def test_errors(dev):
    from two_stage_object_detection_amd._ffi import TsodError
    from two_stage_object_detection_amd.utils.metrics import DetectionEvaluator
    ev = DetectionEvaluator(3)
    det = torch.zeros(2, 5, 6, device=dev)
    gb, gl = torch.zeros(2, 1, 4, device=dev), torch.zeros(2, 1, dtype=torch.int64, device=dev)
    with pytest.raises(TsodError):
        ev.update(det.cpu(), gb, gl)
    with pytest.raises(TsodError):
        ev.update(det, gb.cpu(), gl)
    with pytest.raises(ValueError):
        DetectionEvaluator(3, iou_thresholds=[.5] * 33)
    with pytest.raises(TsodError):
        ev.update(det, torch.zeros(2, 1025, 4, device=dev), torch.zeros(2, 1025, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ev.update(torch.zeros(2, 5, 5, device=dev), gb, gl)
    with pytest.raises(ValueError):
        ev.update(det, gb[:1], gl[:1])


# ------------------------------------------------------------------------------------------------------------- eval_fn
def restated_batch(tr, dev, imgs, bboxes, labels, nms_thr):
    """forward's predictions -> per-class NMS with oracle.nms -> the image's rows for evaluate_np."""
    losses, ap, cp, csp = tr(imgs.to(dev), [b.to(dev) for b in bboxes], [l.to(dev) for l in labels])[:4]
    out = []
    for i in range(ap.shape[0]):
        boxes, cls, sc = ap[i].cpu(), cp[i].cpu(), csp[i].cpu()
        rows = []
        for c in torch.unique(cls).tolist():
            if c == 0:
                continue
            idx = torch.nonzero(cls == c).view(-1)
            keep = oracle.nms(boxes[idx], sc[idx], nms_thr)
            rows.append(idx[keep])
        idx = torch.sort(torch.cat(rows)).values if rows else torch.zeros(0, dtype=torch.int64)
        idx = idx[torch.argsort(-sc[idx], stable=True)] if len(idx) else idx      # postprocess's order: score, then row
        d = torch.cat([boxes[idx], sc[idx, None], cls[idx, None].float()], 1).numpy()
        out.append((d, bboxes[i].numpy(), (labels[i] + 1).numpy()))
    return float(losses[-1]), out


def test_eval_fn(dev, z):
    tr = make_trainer(dev)
    img, bbox, label = image(z), t(z, "bbox"), t(z, "label")
    loader = [(img[None], [bbox], [label]), (img[None], [bbox[:2].clone()], [label[:2].clone()])]
    with torch.inference_mode():
        loss, mAP = tr.eval_fn(loader, nms_iou_threshold=0.7, map_iou_threshold=0.5)
        parts = [restated_batch(tr, dev, *b, 0.7) for b in loader]
    assert loss == pytest.approx(sum(p[0] for p in parts) / 2, rel=1e-6)
    want = evaluate_np([p[1] for p in parts], 81, [0.5], ignore_class=0)
    assert mAP == pytest.approx(want["mAP"], abs=1e-12)
    with torch.inference_mode():
        res = tr.calculate_metrics(*[x.cpu() for x in tr(img[None].to(dev), [bbox.to(dev)], [label.to(dev)])[1:4]],
                                   bbox[None], (label + 1)[None], nms_iou_threshold=0.7, map_iou_threshold=0.5)
    assert set(res) == {"mAP", "class_metrics"} and sorted(res["class_metrics"]) == list(range(1, 81))
    assert all(set(v) == {"AP", "Recall", "Precision", "TP", "FP", "FN"} for v in res["class_metrics"].values())
    one = evaluate_np([parts[0][1]], 81, [0.5], ignore_class=0)
    assert res["mAP"] == pytest.approx(one["mAP"], abs=1e-12)
    assert [res["class_metrics"][c]["TP"] for c in range(1, 81)] == one["TP"][1:, 0].tolist()
