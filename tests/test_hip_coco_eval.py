"""The HIP COCO evaluator (csrc/eval_metrics.hip, utils.metrics.COCOEvaluator, FasterRCNNTrainer.eval_coco) against the
section-4.14 evaluator where the two metrics coincide, against the numpy restatement of tests/coco_eval_restated.py, and
through the hand-made cases of tests/test_coco_eval.py."""
import numpy as np
import pytest
import torch

from coco_eval_restated import COCO_AREA_RANGES, COCO_THRESHOLDS, box_area, evaluate_coco_np
from test_coco_eval import CASES, positive_area_only
from test_hip_detection_eval import random_dataset, run_hip as run_hip_plain
from test_trainer import image, make_trainer, t, z  # noqa: F401 (z: the trainer fixture)

pytestmark = pytest.mark.gpu
ONLY_ALL = (("all", 0, 1e10),)


# ------------------------------------------------------------------------------------------------------------- running
def pad_batch(batch, dev):
    """A batch of images -> update()'s padded arguments; crowd / area stay None when no image of the batch carries them."""
    R = max(1, max(len(im[0]) for im in batch))
    G = max(1, max(len(im[2]) for im in batch))
    B = len(batch)
    det = np.zeros((B, R, 6), np.float32)
    gb = np.zeros((B, G, 4), np.float32)
    gl = np.full((B, G), -1, np.int64)
    has_crowd = any(len(im) > 3 and im[3] is not None for im in batch)
    has_area = any(len(im) > 4 and im[4] is not None for im in batch)
    crowd, area = np.zeros((B, G), np.uint8), np.zeros((B, G), np.float32)
    for b, im in enumerate(batch):
        d, g, l = np.asarray(im[0], np.float32).reshape(-1, 6), np.asarray(im[1], np.float32).reshape(-1, 4), np.asarray(im[2])
        det[b, :len(d)], gb[b, :len(l)], gl[b, :len(l)] = d, g, l
        if len(im) > 3 and im[3] is not None:
            crowd[b, :len(l)] = im[3]
        area[b, :len(l)] = im[4] if len(im) > 4 and im[4] is not None else box_area(g)
    up = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    kw = dict(counts=torch.tensor([len(im[0]) for im in batch], dtype=torch.int32, device=dev))
    if has_crowd:
        kw["gt_crowd"] = up(crowd)
    if has_area:
        kw["gt_area"] = up(area)
    return (up(det), up(gb), up(gl)), kw


def to_result(ev):
    """COCOEvaluator's records and compute() in the layout of evaluate_coco_np's result."""
    score, cls, rank, tp, ig = ev.records()
    got = ev.compute()
    stats = {k: v for k, v in got.items() if k.startswith(("AP", "AR")) and isinstance(v, float)}
    out = {k: got[k].numpy() for k in ("precision", "recall", "TP", "FP", "FN", "npig")}
    out.update(score=score, cls=cls, rank=rank, tp=tp, ig=ig, stats=stats)
    return out


def run_hip(updates, num_classes, dev, thresholds=COCO_THRESHOLDS, max_dets=(1, 10, 100), area_ranges=COCO_AREA_RANGES,
            ignore_class=None):
    from two_stage_object_detection_amd.utils.metrics import COCOEvaluator
    ev = COCOEvaluator(num_classes, iou_thresholds=thresholds, max_dets=max_dets, area_ranges=area_ranges,
                       ignore_class=ignore_class)
    for batch in updates:
        args, kw = pad_batch(batch, dev)
        ev.update(*args, **kw)
    return to_result(ev)


def check_equal(got, want):
    assert np.array_equal(got["score"].view(np.int32), want["score"].view(np.int32))
    for k in ("cls", "rank", "tp", "ig", "npig", "TP", "FP", "FN"):                      # every integer: exact
        assert np.array_equal(got[k], want[k]), k
    for k in ("precision", "recall"):
        assert got[k].shape == want[k].shape and np.abs(got[k] - want[k]).max(initial=0) <= 1e-12, k
    assert sorted(got["stats"]) == sorted(want["stats"])
    for k, v in want["stats"].items():
        assert (np.isnan(v) and np.isnan(got["stats"][k])) or abs(got["stats"][k] - v) <= 1e-12, k


def agree(updates, num_classes, dev, **kw):
    got = run_hip(updates, num_classes, dev, **kw)
    check_equal(got, evaluate_coco_np(updates, num_classes, **kw))
    return got


def coco_dataset(seed, n_images, n_classes, max_gt, max_det, batch_sizes):
    """random_dataset with crowd flags at probability 0.1 and, for every third batch, gt_area values around the box areas
    (some exactly on the range bounds)."""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for i, batch in enumerate(random_dataset(seed, n_images, n_classes, max_gt, max_det, batch_sizes)):
        rows = []
        for d, gb, gl in batch:
            crowd = (rng.random(len(gl)) < .1).astype(np.uint8)
            area = None
            if i % 3 == 0:
                area = box_area(gb) * rng.uniform(.3, 1.5, len(gl)).astype(np.float32)
                area[rng.random(len(gl)) < .1] = 32 ** 2
                area[rng.random(len(gl)) < .05] = 96 ** 2
            rows.append((d, gb, gl, crowd, area))
        out.append(rows)
    return out


# ------------------------------------------------------------------------------- agreement with the section-4.14 evaluator
@pytest.mark.parametrize("seed,n_images,n_classes,max_gt,max_det,batch_sizes,max_dets", [
    (0, 40, 3, 6, 30, (16, 7), 100),
    (1, 64, 5, 70, 300, (16,), 20),
])
def test_one_range_one_cap_no_crowd_is_the_detection_evaluator(dev, seed, n_images, n_classes, max_gt, max_det, batch_sizes,
                                                               max_dets):
    raw = random_dataset(seed, n_images, n_classes, max_gt, max_det, batch_sizes)
    batches = positive_area_only(raw)
    assert sum(len(d) for b in batches for d, _, _ in b) < sum(len(d) for b in raw for d, _, _ in b)   # something was filtered
    old = run_hip_plain(batches, n_classes, dev, max_dets=max_dets)
    want, (s, c, m) = old.compute(), old.records()
    got = run_hip(batches, n_classes, dev, max_dets=(max_dets,), area_ranges=ONLY_ALL)
    assert np.array_equal(got["score"].view(np.int32), s.view(np.int32)) and np.array_equal(got["cls"], c)
    assert np.array_equal(got["tp"][:, 0], m) and not got["ig"].any() and not got["tp"][:, 1:].any()
    assert np.array_equal(got["npig"][:, 0], want["npig"].numpy())
    for k in ("TP", "FP", "FN"):
        assert np.array_equal(got[k][:, 0, 0], want[k].numpy()), k
    assert np.abs(got["precision"][:, 0, 0] - want["AP"].numpy()).max() <= 1e-12
    assert np.abs(got["recall"][:, 0, 0] - want["recall"].numpy()).max() <= 1e-12
    assert abs(got["stats"]["AP"] - want["mAP"]) <= 1e-12
    # unfiltered, the detections of negative area that nothing matched are ignored by "all": the restatement's answer
    unfiltered = agree(raw, n_classes, dev, max_dets=(max_dets,), area_ranges=ONLY_ALL)
    assert unfiltered["ig"].any()


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("seed,n_images,n_classes,max_gt,max_det,batch_sizes,kw", [
    (0, 40, 3, 6, 30, (16, 7), dict(thresholds=(.5, .75))),
    (2, 300, 20, 12, 40, (16, 7, 33), dict()),
])
def test_evaluator_matches_the_restatement(dev, seed, n_images, n_classes, max_gt, max_det, batch_sizes, kw):
    batches = coco_dataset(seed, n_images, n_classes, max_gt, max_det, batch_sizes)
    assert any(im[3].any() for b in batches for im in b) and any(im[4] is not None for b in batches for im in b)
    got = agree(batches, n_classes, dev, **kw)
    assert got["ig"].any() and got["tp"].any() and (got["npig"][:, 0] > got["npig"][:, 1]).any()
    again = run_hip(batches, n_classes, dev, **kw)                                         # two runs: identical bits
    for k in ("precision", "recall"):
        assert np.array_equal(got[k].view(np.int64), again[k].view(np.int64)), k
    assert all(np.array_equal(got[k], again[k]) for k in ("tp", "ig", "rank", "TP", "FP", "FN", "npig"))
    assert {k: np.float64(v).view(np.int64) for k, v in got["stats"].items()} == \
           {k: np.float64(v).view(np.int64) for k, v in again["stats"].items()}
    if not kw:
        assert sorted(got["stats"]) == sorted(["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm",
                                               "ARl"])


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_hand_made_cases(dev, case):
    case(lambda updates, num_classes, **kw: run_hip(updates, num_classes, dev, **kw))


# ------------------------------------------------------------------------------------------------------------ input forms
def test_input_forms_agree(dev):
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.utils.metrics import COCOEvaluator
    batch = coco_dataset(6, 12, 4, 8, 60, (12,))[0]
    assert batch[0][4] is not None
    (det, gb, gl), kw = pad_batch(batch, dev)
    det_sorted, keep, n_kept = hip_ops.filter_detections(det, iou_thr=.6, per_class=True)
    ns = n_kept.tolist()
    rows = [det_sorted[b][keep[b, :ns[b]].long()] for b in range(det.shape[0])]
    lists = [[torch.from_numpy(np.asarray(im[k])).to(dev) for im in batch] for k in (1, 2, 3, 4)]
    evs = [COCOEvaluator(4) for _ in range(4)]
    evs[0].update(det_sorted, lists[0], lists[1], gt_crowd=lists[2], gt_area=lists[3], keep=keep, n_kept=n_kept)
    evs[1].update(rows, lists[0], lists[1], gt_crowd=lists[2], gt_area=lists[3])
    evs[2].update(torch.nn.utils.rnn.pad_sequence(rows, batch_first=True), gb, gl, gt_crowd=kw["gt_crowd"],
                  gt_area=kw["gt_area"], counts=n_kept)
    evs[3].update(rows, gb, gl, gt_crowd=kw["gt_crowd"].bool(), gt_area=lists[3])          # padded and list forms mixed
    res = [to_result(ev) for ev in evs]
    assert res[0]["tp"].any() and res[0]["ig"].any()
    for r in res[1:]:
        for k in ("score", "cls", "rank", "tp", "ig", "npig", "TP", "FP", "FN", "precision", "recall"):
            assert np.array_equal(res[0][k], r[k]), k
        assert res[0]["stats"] == r["stats"] or all(np.isnan(v) or v == r["stats"][k] for k, v in res[0]["stats"].items())


def test_errors(dev):
    from two_stage_object_detection_amd._ffi import TsodError
    from two_stage_object_detection_amd.utils.metrics import COCOEvaluator
    ev = COCOEvaluator(3)
    det = torch.zeros(2, 5, 6, device=dev)
    gb, gl = torch.zeros(2, 3, 4, device=dev), torch.zeros(2, 3, dtype=torch.int64, device=dev)
    with pytest.raises(TsodError):
        ev.update(det, gb, gl, gt_crowd=torch.zeros(2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ev.update(det, gb, gl, gt_crowd=torch.zeros(2, 4, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        ev.update(det, gb, gl, gt_area=[torch.zeros(3, device=dev)])
    with pytest.raises(TsodError):
        ev.update(det.cpu(), gb, gl)


# -------------------------------------------------------------------------------------------------------------- size edges
def one_class_image(rng, n_det, n_gt, cls=0, crowd=None):
    xy = rng.uniform(0, 400, (n_gt, 2)).astype(np.float32)
    gb = np.concatenate([xy, xy + rng.uniform(4, 150, (n_gt, 2)).astype(np.float32)], 1)
    d = np.zeros((n_det, 6), np.float32)
    src = rng.integers(0, max(n_gt, 1), n_det)
    base = gb[src] if n_gt else np.tile(np.float32([10, 10, 50, 50]), (n_det, 1))
    d[:, :4] = base + rng.normal(0, 4, (n_det, 4)).astype(np.float32)
    d[:, 4] = np.round(rng.random(n_det) * 50) / 50
    d[:, 5] = cls
    return (d, gb, np.full(n_gt, cls, np.int64), crowd, None)


def test_no_ground_truth_at_all(dev):
    from two_stage_object_detection_amd.utils.metrics import COCOEvaluator
    rng = np.random.default_rng(0)
    d = one_class_image(rng, 5, 0)[0]
    ev = COCOEvaluator(2, iou_thresholds=(.5,))
    ev.update(torch.from_numpy(d[None]).to(dev), torch.zeros(1, 0, 4, device=dev),
              torch.zeros(1, 0, dtype=torch.int64, device=dev))            # G = 0: the library gets NULL for the ground truth
    check_equal(to_result(ev), evaluate_coco_np([[(d, np.zeros((0, 4)), [])]], 2, thresholds=(.5,)))
    assert ev.compute()["FP"][0, 0, -1, 0] == 5 and np.isnan(ev.compute()["AP"])


def test_size_edges(dev):
    rng = np.random.default_rng(1)
    only_crowd = one_class_image(rng, 6, 3, crowd=np.ones(3, np.uint8))
    got = agree([[only_crowd, one_class_image(rng, 4, 2)]], 1, dev)
    assert (got["npig"] <= 2).all() and got["ig"][:6, 0].any()
    wide = one_class_image(rng, 40, 65, crowd=(rng.random(65) < .2).astype(np.uint8))      # G = 65: one past a wave
    got = agree([[wide]], 1, dev, thresholds=(.5, .75))
    assert got["tp"].any()
    agree([[one_class_image(rng, 1, 2)]], 1, dev)                                           # R = 1
    many = one_class_image(rng, 101, 30)                                                    # rank 100 is dropped
    got = agree([[many]], 1, dev, thresholds=(.5,))
    assert len(got["rank"]) == 100 and got["rank"].max() == 99
    small = coco_dataset(3, 10, 3, 8, 30, (4, 6))
    agree(small, 3, dev, thresholds=(.5,))                                                  # T = 1
    got = agree(small, 3, dev, thresholds=np.linspace(.05, .98, 32))                        # T = 32: every bit of the masks
    assert (got["tp"] >> np.uint32(31)).any() or (got["ig"] >> np.uint32(31)).any()
    agree(small, 3, dev, thresholds=(.5, .6), area_ranges=(("medium", 32 ** 2, 96 ** 2),), max_dets=(5,))   # A = 1, M = 1
    agree(small, 3, dev, thresholds=(.5, .6), max_dets=(1, 2, 3, 100))                      # A = 4, M = 4


def test_largest_shapes(dev):
    """G = 1024 and R = 8192, the limits: the match kernel's largest LDS request (143360 bytes of the CU's 160 KB)."""
    rng = np.random.default_rng(4)
    G, R, C = 1024, 8192, 8
    xy = rng.uniform(0, 900, (G, 2)).astype(np.float32)
    gb = np.concatenate([xy, xy + rng.uniform(4, 150, (G, 2)).astype(np.float32)], 1)
    gl = rng.integers(0, C, G)
    src = rng.integers(0, G, R)
    d = np.zeros((R, 6), np.float32)
    d[:, :4] = gb[src] + rng.normal(0, 5, (R, 4)).astype(np.float32)
    d[:, 4] = np.round(rng.random(R) * 1000) / 1000
    d[:, 5] = gl[src]
    got = agree([[(d, gb, gl, (rng.random(G) < .1).astype(np.uint8), None)]], C, dev, thresholds=(.5,))
    assert len(got["rank"]) == 100 * C and got["tp"].any() and got["ig"].any()


# --------------------------------------------------------------------------------------------------------------- eval_coco
def test_eval_coco(dev, z):
    from two_stage_object_detection_amd.utils.metrics import COCOEvaluator
    tr = make_trainer(dev)
    img, bbox, label = image(z), t(z, "bbox"), t(z, "label")
    crowd = torch.zeros(len(label), dtype=torch.uint8)
    crowd[0] = 1
    plain = [(img[None], [bbox], [label]), (img[None], [bbox[:2].clone()], [label[:2].clone()])]
    loader = [(img[None], [bbox], [label], [crowd]), plain[1]]
    with torch.inference_mode():
        loss, stats = tr.eval_coco(loader, nms_iou_threshold=0.7)
        ev = COCOEvaluator(81, ignore_class=0)
        total = 0.0
        for imgs, bboxes, labels, *extra in loader:
            out = tr(imgs.to(dev), [b.to(dev) for b in bboxes], [l.to(dev) for l in labels])
            total += float(out[0][-1])
            det_sorted, keep, n_kept = tr._records(*out[1:4], 0.7)
            ev.update(det_sorted, [b.to(dev) for b in bboxes], [l.to(dev) + 1 for l in labels],
                      gt_crowd=[c.to(dev) for c in extra[0]] if extra else None, keep=keep, n_kept=n_kept)
        want = ev.compute()
        assert loss == pytest.approx(total / 2, rel=1e-6)
        assert stats["AP"] == want["AP"] and torch.equal(stats["precision"], want["precision"])
        assert torch.equal(stats["npig"], want["npig"]) and stats["npig"][:, 0].sum() == len(label) + 2 - 1   # the crowd is out
        assert len([k for k in stats if k[:2] in ("AP", "AR")]) == 12
        # without crowd regions (and with boxes of positive area) threshold 0.7 of the table is eval_fn's one number
        assert (bbox[:, 2] > bbox[:, 0]).all() and (bbox[:, 3] > bbox[:, 1]).all()
        loss_plain, table = tr.eval_coco(plain, nms_iou_threshold=0.7)
        loss_fn, mAP = tr.eval_fn(plain, nms_iou_threshold=0.7, map_iou_threshold=0.7)
    assert table["iou_thresholds"][4] == float(np.float32(0.7)) and table["area_ranges"][0][0] == "all"
    ap = table["precision"][:, 0, -1, 4].numpy()
    assert abs(float(np.mean(ap[ap > -1])) - mAP) <= 1e-12
    assert loss_plain == loss_fn
    assert tr.eval_coco([]) == (0, {})
