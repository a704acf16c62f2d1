"""Time the JPEG decoder: the host Huffman pass, the upload and the two kernels, beside Pillow and device copies.
    python scripts/jpeg_bench.py [--iters N] [--warmup N] [--out profiles/jpeg_mi355x.jsonl]

640x480 4:2:0 quality-90 files of seeded pictures (smooth shapes plus noise), encoded once with Pillow at start (without Pillow
the script says so and exits).  At batch 1 and 16, one JSON line each:
  * ``huffman_us_per_image_1t`` / ``_16t``: wall time of the host pass of the batch with 1 and with 16 threads, per image;
  * ``upload_us``: the coefficients (all but a few KB of what goes up) from pinned memory to the device, HIP events;
  * ``idct_us`` / ``to_rgb_us``: each kernel, and ``*_copy_us``: a device-to-device copy of the bytes that kernel reads plus
    writes (a copy moves each byte twice, so the copy is of half that sum) - the floor of a memory-bound kernel, in the same run;
  * ``batch_us_per_image``: the whole ``JPEGDecoder.batch`` call, wall time with one synchronize at the end;
  * ``pillow_us_per_image``: ``Image.open(...).convert("RGB")`` on one thread - what is being replaced.
Device figures are the median of ``--iters`` calls timed one by one with HIP events, issued back to back after ``--warmup``
calls; host figures the median of ``--iters`` wall-clock calls."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import hip_ops  # noqa: E402
from two_stage_object_detection_amd.dataset import image_io  # noqa: E402

H, W, QUALITY = 480, 640, 90


def median_us(fn, iters, warmup):
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
    times = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in events)
    return times[len(times) // 2]


def host_median_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e6)
    return sorted(times)[len(times) // 2]


def picture(rng):
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 100 * np.sin(xx / (20 + 15 * c) + rng.uniform(0, 6)) * np.cos(yy / (31 - 7 * c)) for c in range(3)], axis=2)
    for _ in range(12):                                              # hard-edged rectangles
        y, x, h, w = rng.integers(0, H - 40), rng.integers(0, W - 40), rng.integers(10, 200), rng.integers(10, 200)
        img[y:y + h, x:x + w] = rng.integers(0, 256, size=3)
    return np.clip(img + rng.normal(0, 6, size=img.shape), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    if args.iters < 20 or args.warmup < 3:
        ap.error("at least 20 timed and 3 warm-up calls")
    try:
        from PIL import Image
    except ImportError:
        print("scripts/jpeg_bench.py needs Pillow to encode its workload (and as the decoder it is compared with); it is not installed")
        return 1
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    files = []
    for _ in range(16):
        buf = io.BytesIO()
        Image.fromarray(picture(rng)).save(buf, "JPEG", quality=QUALITY, subsampling=2)
        files.append(buf.getvalue())
    pillow = host_median_us(lambda: [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files], max(args.iters // 5, 5), 2) / 16
    pools = {1: None, 16: ThreadPoolExecutor(max_workers=16)}
    lines = []
    for B in (1, 16):
        batch = files[:B]
        raws = [hip_ops.jpeg_bytes(f) for f in batch]
        infos = [hip_ops.jpeg_parse(r)[1] for r in raws]
        plan = hip_ops.jpeg_plan(infos)
        table, idct_work, rgb_work = plan["table"], plan["idct_work"], plan["rgb_work"]
        coef_host = torch.empty(plan["coef_count"], dtype=torch.int16, pin_memory=True)
        coef_np = coef_host.numpy()

        def huffman(i):
            first = table[i].coef_offset[0]
            return hip_ops.jpeg_entropy_decode(raws[i], coef_np[first:first + infos[i].coef_total])

        host = {}
        for threads, pool in pools.items():
            run = (lambda: [huffman(i) for i in range(B)]) if pool is None else (lambda: list(pool.map(huffman, range(B))))
            assert not any(run())
            host[threads] = host_median_us(run, args.iters, args.warmup) / B
        quant_np = np.concatenate([np.ctypeslib.as_array(i.quant)[:i.n_comp].reshape(-1) for i in infos]).view(np.int16)
        table_dev = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
        idct_dev, rgb_dev = torch.from_numpy(idct_work).to(dev), torch.from_numpy(rgb_work).to(dev)
        quant = torch.from_numpy(quant_np.copy()).to(dev)
        coef = torch.empty(plan["coef_count"], dtype=torch.int16, device=dev)
        planes = torch.empty(plan["plane_bytes"], dtype=torch.uint8, device=dev)
        out = torch.empty(plan["out_bytes"], dtype=torch.uint8, device=dev)
        upload = median_us(lambda: coef.copy_(coef_host, non_blocking=True), args.iters, args.warmup)
        idct = median_us(lambda: hip_ops.jpeg_idct(table, table_dev, idct_work, idct_dev, coef, quant, planes), args.iters, args.warmup)
        to_rgb = median_us(lambda: hip_ops.jpeg_to_rgb(table, table_dev, rgb_work, rgb_dev, planes, out), args.iters, args.warmup)
        # the floors: a copy of n bytes reads n and writes n
        idct_bytes = 2 * plan["coef_count"] + plan["plane_bytes"]
        rgb_bytes = plan["plane_bytes"] + 3 * B * H * W
        a = torch.empty(max(idct_bytes, rgb_bytes) // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        idct_copy = median_us(lambda: b[:idct_bytes // 2].copy_(a[:idct_bytes // 2]), args.iters, args.warmup)
        rgb_copy = median_us(lambda: b[:rgb_bytes // 2].copy_(a[:rgb_bytes // 2]), args.iters, args.warmup)
        want = np.asarray(Image.open(io.BytesIO(batch[-1])).convert("RGB"))
        got = out[table[B - 1].out_offset:table[B - 1].out_offset + want.size].view(H, W, 3).cpu().numpy()
        dec = image_io.JPEGDecoder(dev, threads=16)

        def whole():
            dec.batch(batch)
            torch.cuda.synchronize()

        whole_us = host_median_us(whole, args.iters, args.warmup) / B
        dec.close()
        rec = dict(bench="jpeg", batch=B, size=f"{W}x{H}", sampling="4:2:0", quality=QUALITY, iters=args.iters, warmup=args.warmup,
                   file_bytes=int(np.mean([len(f) for f in batch])), huffman_us_per_image_1t=round(host[1], 1),
                   huffman_us_per_image_16t=round(host[16], 1), upload_us=round(upload, 2), upload_bytes=2 * plan["coef_count"],
                   idct_us=round(idct, 2), idct_copy_us=round(idct_copy, 2), idct_over_copy=round(idct / idct_copy, 3),
                   idct_bytes=idct_bytes, to_rgb_us=round(to_rgb, 2), to_rgb_copy_us=round(rgb_copy, 2),
                   to_rgb_over_copy=round(to_rgb / rgb_copy, 3), to_rgb_bytes=rgb_bytes, batch_us_per_image=round(whole_us, 1),
                   pillow_us_per_image=round(pillow, 1), equals_pillow=bool(np.array_equal(got, want)))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    pools[16].shutdown()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
