"""The COCO metric of DESIGN.md section 4.25: the numpy restatement (tests/coco_eval_restated.py) pinned by hand-made cases
(CPU, no GPU).  Every case is a function of ``run(updates, num_classes, **kw) -> result`` so that
tests/test_hip_coco_eval.py puts the HIP evaluator through the same cases with the same expected outcomes."""
import inspect

import numpy as np
import pytest
import torch

import oracle
from coco_eval_restated import COCO_AREA_RANGES, crowd_iou_f32, evaluate_coco_np, iou_f32
from test_detection_eval import det, evaluate_np

ALL, SMALL, MEDIUM, LARGE = range(4)


# ----------------------------------------------------------------------------------------------------- hand-made cases
def case_crowd_takes_three_detections(run):
    d = det([10, 10, 30, 30, .9, 0], [40, 40, 60, 60, .8, 0], [20, 50, 50, 90, .7, 0])
    r = run([[(d, [[0, 0, 100, 100]], [0], [1], None)]], 1, thresholds=[.5])
    assert r["tp"].tolist() == [[0] * 4] * 3 and r["ig"].tolist() == [[1] * 4] * 3     # matched to the crowd: ignored
    assert not r["TP"].any() and not r["FP"].any() and not r["FN"].any()
    assert r["npig"].tolist() == [[0, 0, 0, 0]]                                           # the crowd is no missed object
    assert (r["precision"] == -1).all() and (r["recall"] == -1).all()


def case_not_ignored_gt_wins_over_a_better_ignored_one(run):
    # index 0: a crowd region at 0.9 (inter / area_det); index 1: a plain GT at IoU 0.6.  The plain one is walked first.
    gts = [[0, 0, 9, 10], [0, 0, 10, 6]]
    assert crowd_iou_f32([0, 0, 10, 10], gts[:1])[0, 0] > iou_f32([0, 0, 10, 10], gts[1:])[0, 0] >= np.float32(.5)
    r = run([[(det([0, 0, 10, 10, .9, 0]), gts, [0, 0], [1, 0], None)]], 1, thresholds=[.5])
    assert r["tp"][0, ALL] == 1 and r["ig"][0, ALL] == 0 and r["tp"][0, SMALL] == 1
    assert r["ig"][0].tolist() == [0, 0, 1, 1]            # "medium" / "large" ignore the 60-pixel GT: the crowd takes it
    assert r["npig"].tolist() == [[1, 1, 0, 0]]
    assert (r["TP"][0, ALL, -1, 0], r["FP"][0, ALL, -1, 0], r["FN"][0, ALL, -1, 0]) == (1, 0, 0)


def case_unmatched_detection_outside_the_range_is_ignored(run):
    r = run([[(det([0, 0, 20, 20, .9, 0]), [[200, 200, 230, 230]], [0])]], 1, thresholds=[.5])
    assert r["tp"].tolist() == [[0] * 4] and r["ig"].tolist() == [[0, 0, 1, 1]]
    assert r["FP"][0, :, -1, 0].tolist() == [1, 1, 0, 0]
    assert r["npig"].tolist() == [[1, 1, 0, 0]] and r["FN"][0, :, -1, 0].tolist() == [1, 1, 0, 0]


def case_area_bounds_are_inclusive(run):
    r = run([[(det([0, 0, 32, 32, .9, 0]), [[0, 0, 32, 32]], [0])]], 1, thresholds=[.5])
    assert r["npig"].tolist() == [[1, 1, 1, 0]]           # area exactly 1024: "small" and "medium"
    assert r["tp"].tolist() == [[1, 1, 1, 0]] and r["ig"].tolist() == [[0, 0, 0, 1]]


def case_gt_area_overrides_the_box(run):
    r = run([[(det([0, 0, 10, 10, .9, 0]), [[0, 0, 10, 10]], [0], None, [5000.])]], 1, thresholds=[.5])
    assert r["npig"].tolist() == [[1, 0, 1, 0]]
    assert r["tp"].tolist() == [[1, 0, 1, 0]] and r["ig"].tolist() == [[0, 1, 0, 1]]


def case_crowd_iou_is_over_the_detection(run):
    assert iou_f32([10, 10, 20, 20], [[0, 0, 100, 100]])[0, 0] < np.float32(.02)
    r = run([[(det([10, 10, 20, 20, .9, 0]), [[0, 0, 100, 100]], [0], [1], None)]], 1, thresholds=[.5, .95])
    assert r["ig"][0, ALL] == 0b11 and r["tp"][0, ALL] == 0


def case_caps(run):
    d = det([50, 50, 60, 60, .9, 0], [0, 0, 10, 10, .8, 0])
    r = run([[(d, [[0, 0, 10, 10]], [0])]], 1, thresholds=[.5], max_dets=(1, 10, 100))
    assert r["rank"].tolist() == [0, 1]
    assert r["TP"][0, ALL, :, 0].tolist() == [0, 1, 1] and r["FP"][0, ALL, :, 0].tolist() == [1, 1, 1]
    s = r["stats"]
    assert (s["AR1"], s["AR10"], s["AR100"]) == (0.0, 1.0, 1.0)
    assert s["AP"] == 0.5                                   # FP first: the envelope is 1/2 at all 101 points


def case_class_with_only_ignored_gt_is_excluded(run):
    d = det([0, 0, 50, 50, .9, 0], [100, 100, 110, 110, .9, 1])
    r = run([[(d, [[0, 0, 50, 50], [100, 100, 110, 110]], [0, 1])]], 2, thresholds=[.5])
    assert r["npig"].tolist() == [[1, 0, 1, 0], [1, 1, 0, 0]]
    assert (r["precision"][1, MEDIUM] == -1).all() and (r["recall"][1, MEDIUM] == -1).all()
    assert r["ig"][1, MEDIUM] == 1 and r["FP"][1, MEDIUM, -1, 0] == 0
    assert r["stats"]["APm"] == 1.0 and r["stats"]["APs"] == 1.0 and r["stats"]["AP"] == 1.0
    assert np.isnan(r["stats"]["APl"])                      # no class has a large ground truth


CASES = [case_crowd_takes_three_detections, case_not_ignored_gt_wins_over_a_better_ignored_one,
         case_unmatched_detection_outside_the_range_is_ignored, case_area_bounds_are_inclusive,
         case_gt_area_overrides_the_box, case_crowd_iou_is_over_the_detection, case_caps,
         case_class_with_only_ignored_gt_is_excluded]


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_restatement(case):
    case(evaluate_coco_np)


# ------------------------------------------------------------------------------------------ the restatement's own footing
def test_restated_iou_is_the_projects_bbox_iou():
    rng = np.random.default_rng(3)
    xy = rng.uniform(0, 300, (2, 200, 2)).astype(np.float32)
    a, b = (np.concatenate([p, p + rng.uniform(0, 120, (200, 2)).astype(np.float32)], 1) for p in xy)
    want = oracle.bbox_iou(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    assert np.array_equal(iou_f32(a, b), want)


def positive_area_only(batches):
    """The images without the detections and ground truth of negative area, which range "all" (lo = 0) ignores."""
    out = []
    for batch in batches:
        rows = []
        for d, gb, gl in batch:
            dk = ~((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1]) < 0)
            gk = ~((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]) < 0)
            rows.append((d[dk], gb[gk], gl[gk]))
        out.append(rows)
    return out


def test_one_range_one_cap_no_crowd_is_the_section_4_14_metric():
    from test_hip_detection_eval import random_dataset
    batches = positive_area_only(random_dataset(0, 40, 3, 6, 30, (16, 7)))
    want = evaluate_np(batches, 3, [.5, .75])
    got = evaluate_coco_np(batches, 3, thresholds=[.5, .75], max_dets=(100,), area_ranges=(("all", 0, 1e10),))
    assert np.array_equal(got["score"], want["score"]) and np.array_equal(got["cls"], want["cls"])
    assert np.array_equal(got["tp"][:, 0], want["mask"]) and not got["ig"].any()
    assert np.array_equal(got["npig"][:, 0], want["npig"])
    for k in ("TP", "FP", "FN"):
        assert np.array_equal(got[k][:, 0, 0], want[k]), k
    assert np.array_equal(got["precision"][:, 0, 0], want["AP"]) and np.array_equal(got["recall"][:, 0, 0], want["recall"])
    assert got["stats"]["AP"] == pytest.approx(want["mAP"], abs=1e-15)


# ------------------------------------------------------------------------------------------------------ the public surface
def test_signatures():
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    from two_stage_object_detection_amd.utils import metrics
    assert metrics.COCO_AREA_RANGES == COCO_AREA_RANGES
    p = inspect.signature(metrics.COCOEvaluator.__init__).parameters
    assert list(p) == ["self", "num_classes", "iou_thresholds", "max_dets", "area_ranges", "ignore_class"]
    assert p["iou_thresholds"].default == metrics.COCO_IOU_THRESHOLDS and p["max_dets"].default == (1, 10, 100)
    assert p["area_ranges"].default == metrics.COCO_AREA_RANGES and p["ignore_class"].default is None
    p = inspect.signature(metrics.COCOEvaluator.update).parameters
    assert list(p) == ["self", "det", "gt_boxes", "gt_labels", "gt_crowd", "gt_area", "counts", "keep", "n_kept", "gt_counts"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in list(p)[4:])
    p = inspect.signature(FasterRCNNTrainer.eval_coco).parameters
    assert list(p) == ["self", "eval_dataloader", "scale", "nms_iou_threshold"]
    assert (p["scale"].default, p["nms_iou_threshold"].default) == (1, 0.7)
    for bad in (dict(max_dets=()), dict(max_dets=(10, 1)), dict(max_dets=(1, 2, 3, 4, 5)), dict(area_ranges=()),
                dict(area_ranges=COCO_AREA_RANGES + (("huge", 0, 1),)), dict(iou_thresholds=[.5] * 33)):
        with pytest.raises(ValueError):
            metrics.COCOEvaluator(3, **bad)
    with pytest.raises(RuntimeError):
        metrics.COCOEvaluator(3).compute()
