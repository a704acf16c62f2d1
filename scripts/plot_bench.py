"""Time the training-curve kernels.
    python scripts/plot_bench.py [--iters N] [--warmup N] [--out profiles/plot_mi355x.jsonl]

* ``ema_scan``: ``hip_ops.ema_scan`` over one row of 10^6 samples (the chain is serial: one wave, 64 samples per trip).
* ``figure``: the whole ``utils.draw.plot_training_metrics`` call at 1500x1200 - limits, decorations, the three panels'
  series, legends - for a training series of 10^6 and of 10^3 samples (60 epochs, 6 evaluations), device-resident inputs;
  ``figure_split`` times its launches one by one for the long series.
* ``host_ema``: the reference's own loop (train/train.py:147-153) of ``update_ema`` over 10^5 0-d CPU tensors, for scale.

Every device call is timed on its own between two HIP events, the calls issued back to back; the figures are the median,
minimum and maximum of ``--iters`` calls after ``--warmup`` untimed ones.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import hip_ops  # noqa: E402
from two_stage_object_detection_amd.utils import draw  # noqa: E402
from two_stage_object_detection_amd.utils.utils import update_ema  # noqa: E402

SIZE = (1500, 1200)
EPOCHS, EVALS = 60, 6


def times_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = []
    for _ in range(iters):                                           # back to back: the device does not idle between calls
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        fn()
        e1.record()
        events.append((e0, e1))
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in events)
    return dict(median_us=round(t[len(t) // 2], 2), min_us=round(t[0], 2), max_us=round(t[-1], 2))


def series(n, dev, gen):
    steps = torch.arange(n, dtype=torch.float32)
    return (2.5 * torch.exp(-steps / (n / 3)) + 0.4 + 0.3 * torch.randn(n, generator=gen)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    if args.iters < 10 or args.warmup < 2:
        ap.error("at least 10 timed and 2 warm-up calls")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = []

    def emit(**rec):
        rec.update(iters=args.iters, warmup=args.warmup)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    x = series(10 ** 6, dev, gen)
    out = torch.empty_like(x)
    emit(bench="ema_scan", n=10 ** 6, rows=1, **times_us(lambda: hip_ops.ema_scan(x, 0.01, out=out), args.iters, args.warmup))
    x8 = x.reshape(8, -1)
    out8 = torch.empty_like(x8)
    emit(bench="ema_scan", n=x8.shape[1], rows=8, **times_us(lambda: hip_ops.ema_scan(x8, 0.01, out=out8), args.iters, args.warmup))

    evals = [torch.linspace(1.5, 0.6, EVALS).to(dev), torch.linspace(1.5, 1.4, EVALS).to(dev), torch.linspace(0.1, 0.7, EVALS).to(dev),
             torch.linspace(0.05, 0.45, EVALS).to(dev), torch.linspace(0.0, 0.12, EVALS).to(dev)]
    image = torch.empty((*SIZE, 3), dtype=torch.uint8, device=dev)
    for n in (10 ** 6, 10 ** 3):
        train = x[:n].contiguous() if n < x.numel() else x
        ema = hip_ops.ema_scan(train, 0.01)
        emit(bench="figure", size=f"{SIZE[0]}x{SIZE[1]}", n=n, epochs=EPOCHS, evaluations=EVALS,
             **times_us(lambda: draw.plot_training_metrics(EPOCHS, n, train, ema, *evals, out=image), args.iters, args.warmup))
        if n == 10 ** 6:                                             # where the time goes
            plan = draw.figure_plan(EPOCHS, n, dict(train_loss=n, ema_train_loss=n, eval_loss=EVALS, ema_eval_loss=EVALS,
                                                    mAP50_list=EVALS, mAP50_95_list=EVALS, mAP95_list=EVALS), SIZE)
            limits = torch.zeros(2, device=dev)
            panel = plan["panels"][0]
            background = hip_ops.pack_plot_items([dict(it, limits=limits) if it["kind"] == "number" else it
                                                  for it in plan["background"]]).to(dev)
            curves = [dict(s, y=y) for s, y in zip(panel["series"], (train, ema))]
            emit(bench="figure_split", case="limits_2x1e6", **times_us(lambda: hip_ops.plot_limits([train, ema], out=limits), args.iters, args.warmup))
            emit(bench="figure_split", case=f"background_{len(background)}_items",
                 **times_us(lambda: hip_ops.plot_items(image, background), args.iters, args.warmup))
            emit(bench="figure_split", case="series_2x1e6",
                 **times_us(lambda: hip_ops.plot_series(image, panel["rect"], curves, panel["x_range"], limits), args.iters, args.warmup))

    host = [v for v in x[:10 ** 5].cpu()]                            # 0-d CPU tensors, as the reference's script holds them
    t0 = time.perf_counter()
    ema_host = []
    for i in range(len(host)):
        ema_host.append(host[0] if i == 0 else update_ema(host[i], 0.01, ema_host[i - 1]))
    emit(bench="host_ema", n=len(host), seconds=round(time.perf_counter() - t0, 3))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
