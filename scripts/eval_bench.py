"""Time the detection evaluator on the GPU, with the numpy restatement's CPU time beside it.

    python scripts/eval_bench.py [--reps 20]
    python scripts/eval_bench.py --coco [--images 5000] [--reps 5]

update: one DetectionEvaluator.update of a 16-image batch (R = 300 padded rows, up to 50 ground-truth boxes, T = 10),
hipEvent-timed over --reps back-to-back calls after a warm-up (the records buffer is pre-grown, so no allocation is timed).
compute: DetectionEvaluator.compute's kernels (tsod_eval_accumulate_f64: keys, radix sort, segments, AP) at 5e5 and 4e6
records, 80 classes, timed the same way without the host read.  The CPU column is tests/test_detection_eval.py's numpy
restatement of the same work (single run, wall clock) - a reference point, not a tuned CPU implementation.

--coco: one whole evaluation (every ``update`` of a COCO-sized synthetic set - 16-image batches as above, crowd flags at
probability 0.1 - then ``compute`` with its host read) by ``DetectionEvaluator(80)`` and by ``COCOEvaluator(80)`` (DESIGN.md
section 4.25: four area ranges, caps 1 / 10 / 100) on the same device-resident data, host clock around the synchronising
``compute``, the two alternating, the median of --reps passes each after one warm-up pass, and their ratio.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from two_stage_object_detection_amd import hip_ops  # noqa: E402
from two_stage_object_detection_amd.utils.metrics import COCOEvaluator, DetectionEvaluator  # noqa: E402


def gpu_time_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def batch(rng, B=16, R=300, G=50, C=80):
    gb = np.zeros((B, G, 4), np.float32)
    gl = np.full((B, G), -1, np.int64)
    det = np.zeros((B, R, 6), np.float32)
    images = []
    for b in range(B):
        g = int(rng.integers(1, G + 1))
        xy = rng.uniform(0, 600, (g, 2)).astype(np.float32)
        gb[b, :g] = np.concatenate([xy, xy + rng.uniform(8, 150, (g, 2)).astype(np.float32)], 1)
        gl[b, :g] = rng.integers(0, C, g)
        src = rng.integers(0, g, R)
        det[b, :, :4] = gb[b, src] + rng.normal(0, 8, (R, 4)).astype(np.float32)
        det[b, :, 4] = rng.random(R).astype(np.float32)
        det[b, :, 5] = np.where(rng.random(R) < .7, gl[b, src], rng.integers(0, C, R))
        images.append((det[b], gb[b, :g], gl[b, :g]))
    return det, gb, gl, images


def coco_pass(make, data):
    """One evaluation: a fresh evaluator, every update, compute (which reads back: a synchronise) -> (ms, result)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = make()
    for det, gb, gl, crowd in data:
        if isinstance(ev, COCOEvaluator):
            ev.update(det, gb, gl, gt_crowd=crowd)
        else:
            ev.update(det, gb, gl)
    res = ev.compute()
    return (time.perf_counter() - t0) * 1e3, res


def coco_main(args):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    data = []
    for _ in range((args.images + 15) // 16):
        det, gb, gl, _ = batch(rng)
        crowd = ((rng.random(gl.shape) < .1) & (gl >= 0)).astype(np.uint8)
        data.append(tuple(torch.from_numpy(x).to(dev) for x in (det, gb, gl, crowd)))
    makers = {"detection": lambda: DetectionEvaluator(80), "coco": lambda: COCOEvaluator(80)}
    times = {k: [] for k in makers}
    results = {}
    for rep in range(args.reps + 1):                                     # pass 0 warms up both
        for name, make in makers.items():
            ms, results[name] = coco_pass(make, data)
            if rep:
                times[name].append(ms)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"images": 16 * len(data), "reps": args.reps,
                      "detection_evaluator_ms": round(med["detection"], 2), "coco_evaluator_ms": round(med["coco"], 2),
                      "ratio": round(med["coco"] / med["detection"], 3),
                      "detection_evaluator_ms_all": [round(v, 2) for v in times["detection"]],
                      "coco_evaluator_ms_all": [round(v, 2) for v in times["coco"]],
                      "mAP": round(results["detection"]["mAP"], 6), "AP": round(results["coco"]["AP"], 6)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--coco", action="store_true", help="time a whole evaluation by both evaluators on one COCO-sized set")
    ap.add_argument("--images", type=int, default=5000, help="--coco: images of the synthetic set")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench.py measures the GPU: no device found"
    if args.reps is None:
        args.reps = 5 if args.coco else 20
    if args.coco:
        return coco_main(args)
    from test_detection_eval import accumulate_np, evaluate_np
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    det, gb, gl, images = batch(rng)
    d_det, d_gb, d_gl = (torch.from_numpy(x).to(dev) for x in (det, gb, gl))
    ev = DetectionEvaluator(80)
    ev.update(d_det, d_gb, d_gl)
    ev._reserve(16 * 300 * (args.reps + 8))
    upd_us = gpu_time_us(lambda: ev.update(d_det, d_gb, d_gl), args.reps)
    t0 = time.perf_counter()
    evaluate_np([images], 80, np.linspace(.5, .95, 10))
    upd_cpu_ms = (time.perf_counter() - t0) * 1e3
    out = {"update_b16_r300_us": round(upd_us, 1), "update_b16_r300_numpy_ms": round(upd_cpu_ms, 1)}
    for n in (500_000, 4_000_000):
        score = rng.random(n).astype(np.float32)
        score = np.round(score * 1000) / 1000                            # ties
        cls = rng.integers(0, 80, n).astype(np.int32)
        mask = rng.integers(0, 1 << 10, n).astype(np.uint32)
        rec = np.stack([score.view(np.int32), cls, mask.view(np.int32)], 1)
        records = torch.from_numpy(rec).to(dev)
        n_dev = torch.tensor([n], dtype=torch.int64, device=dev)
        npig = torch.from_numpy(np.bincount(cls, minlength=80).astype(np.int64) // 2 + 1).to(dev)
        us = gpu_time_us(lambda: hip_ops.eval_accumulate(records, n_dev, npig, 10), args.reps)
        t0 = time.perf_counter()
        accumulate_np(score, cls, mask, npig.cpu().numpy(), 10)
        out[f"compute_{n}_us"] = round(us, 1)
        out[f"compute_{n}_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
