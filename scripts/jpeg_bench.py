"""Time the JPEG decoder: the host Huffman pass, the upload and the two kernels, beside Pillow and device copies;
and the same batch with the Huffman pass on the device (``entropy="device"``).
    python scripts/jpeg_bench.py [--iters N] [--warmup N] [--out profiles/jpeg_mi355x.jsonl]
                                 [--split S,O ...] [--subseq-bits BITS,BITS,...]

640x480 4:2:0 quality-90 files of seeded pictures (smooth shapes plus noise), encoded once with Pillow at start (without Pillow
the script says so and exits).  At batch 1 and 16, one JSON line each:
  * ``huffman_us_per_image_1t`` / ``_16t``: wall time of the host pass of the batch with 1 and with 16 threads, per image;
  * ``upload_us``: the coefficients (all but a few KB of what goes up) from pinned memory to the device, HIP events;
  * ``idct_us`` / ``to_rgb_us``: each kernel, and ``*_copy_us``: a device-to-device copy of the bytes that kernel reads plus
    writes (a copy moves each byte twice, so the copy is of half that sum) - the floor of a memory-bound kernel, in the same run;
  * ``batch_us_per_image``: the whole ``JPEGDecoder.batch`` call, wall time with one synchronize at the end;
  * ``pillow_us_per_image``: ``Image.open(...).convert("RGB")`` on one thread - what is being replaced;
  * ``scan_prepare_us_per_image_1t`` / ``_16t``: the host sweep that ``entropy="device"`` leaves (unstuffing, restart markers);
  * ``huffman_device_us``: ``tsod_jpeg_huffman_i16`` alone - the fill launch and the Huffman launch with the entry's walk over
    its arguments - at the decoder's default ``subseq_bits``, and ``huffman_device_us_by_bits`` at 256 ... 2048;
  * ``batch_us_per_image`` / ``batch_device_us_per_image``: the whole ``JPEGDecoder.batch`` call of the two modes, timed in
    ONE loop that alternates them, each call ending in a synchronize; ``device_upload_bytes`` is what the device mode stages;
  * ``split``: with ``--split S,O`` (repeatable), one entry per ``--subseq-bits`` value (the decoder's default without the
    option) and (S, O): ``batch_us_per_image`` of ``JPEGDecoder(entropy="device", subseq_bits=.., split=(S, O))`` from that
    same alternating loop, ``chunks`` (the workgroups of the sync and write launches for this batch), ``repaired`` (the sum of
    ``decoder.repaired``: chunks the stitch launch decoded again, one after the other) and ``equals_pillow``;
  * ``fixpoint_iterations``: (median, most) fixpoint iterations per round over the batch's files at the default
    ``subseq_bits``, counted by tests/jpeg_huffman_main.cpp - the kernel's algorithm on the CPU, where the count is exact and
    free - when a C++ compiler is there (``null`` otherwise).
Device figures are the median of ``--iters`` calls timed one by one with HIP events, issued back to back after ``--warmup``
calls; host figures the median of ``--iters`` wall-clock calls."""
import argparse
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import hip_ops  # noqa: E402
from two_stage_object_detection_amd.dataset import image_io  # noqa: E402

H, W, QUALITY = 480, 640, 90
DEVICE = "cuda:0"


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


def alternating_medians_us(fns, iters, warmup):
    """Medians of wall-clock calls of each of `fns`, taken in one loop that alternates them."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e6)
    return [sorted(t)[len(t) // 2] for t in times]


def fixpoint_iterations(files, words):
    """(median, most) fixpoint iterations per round, from the CPU program; None without a C++ compiler."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "jpeg_huffman_main")
        subprocess.check_call([cxx, "-std=c++17", "-O2", os.path.join(root, "tests", "jpeg_huffman_main.cpp"), "-o", exe])
        paths = []
        for i, data in enumerate(files):
            paths.append(os.path.join(tmp, f"f{i}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(data)
        lines = [line.split() for line in subprocess.check_output([exe, str(words)] + paths, text=True).splitlines()]
    assert all(line[:4] == ["0", "0", "0", "1"] for line in lines)
    return int(np.median([int(line[5]) for line in lines])), max(int(line[4]) for line in lines)


def device_pass(dev, raws, infos, plan):
    """What tsod_jpeg_huffman_i16 takes for this batch, on the host and on the device, and the host sweep that makes it."""
    seg_dtype = hip_ops.jpeg_segment_dtype()
    caps = [hip_ops.jpeg_scan_sizes(info, raw.size) for info, raw in zip(infos, raws)]
    streams = [np.zeros(c[0], dtype=np.uint8) for c in caps]
    segs = [np.zeros(c[1], dtype=seg_dtype) for c in caps]
    huff = np.zeros(hip_ops.JPEG_HUFF_BYTES * len(raws), dtype=np.uint8)

    def sweep(i):
        return hip_ops.jpeg_scan_prepare(raws[i], streams[i], segs[i], huff[hip_ops.JPEG_HUFF_BYTES * i:hip_ops.JPEG_HUFF_BYTES * (i + 1)])

    used, at = [], 0
    for i in range(len(raws)):
        status, n_bytes, n_segs = sweep(i)
        assert status == 0
        part = segs[i][:n_segs].copy()
        part["image"], part["stream_offset"] = i, part["stream_offset"] + at
        used.append((part, streams[i][:n_bytes].copy()))
        at += n_bytes
    segments = np.ascontiguousarray(np.concatenate([u[0] for u in used]))
    stream = np.concatenate([u[1] for u in used])
    work = np.zeros((len(segments), 4), dtype=np.int32)
    work[:, 0] = np.arange(len(segments))
    to_dev = lambda a: torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(dev)  # noqa: E731
    return dict(sweep=sweep, segments=segments, work=work, segments_dev=to_dev(segments), work_dev=to_dev(work), stream=to_dev(stream),
                huff=to_dev(huff), status=torch.empty(len(raws), dtype=torch.int32, device=dev), stream_bytes=int(stream.size))


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
    ap.add_argument("--split", action="append", default=[], metavar="S,O",
                    help="also time entropy='device' with split=(S, O) in the alternating loop (repeatable)")
    ap.add_argument("--subseq-bits", default=None, metavar="BITS[,BITS...]", help="the subsequence lengths of the --split rows")
    args = ap.parse_args()
    try:
        splits = [tuple(int(v) for v in text.split(",")) for text in args.split]
        split_bits = [int(v) for v in args.subseq_bits.split(",")] if args.subseq_bits else [image_io.JPEGDecoder(DEVICE).subseq_bits]
        for bits in split_bits:
            for split in splits or [None]:
                image_io.JPEGDecoder(DEVICE, entropy="device", subseq_bits=bits, split=split)
    except ValueError as e:
        ap.error(str(e))
    if args.iters < 20 or args.warmup < 3:
        ap.error("at least 20 timed and 3 warm-up calls")
    try:
        from PIL import Image
    except ImportError:
        print("scripts/jpeg_bench.py needs Pillow to encode its workload (and as the decoder it is compared with); it is not installed")
        return 1
    dev = torch.device(DEVICE)
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
        # the Huffman pass on the device: the host sweep, the entry alone, the whole batch call beside the host mode's
        dp = device_pass(dev, raws, infos, plan)
        sweep_us = {}
        for threads, pool in pools.items():
            run = (lambda: [dp["sweep"](i) for i in range(B)]) if pool is None else (lambda: list(pool.map(dp["sweep"], range(B))))
            sweep_us[threads] = host_median_us(run, args.iters, args.warmup) / B
        coef_dev = torch.empty(plan["coef_count"], dtype=torch.int16, device=dev)

        def huffman_device(bits):
            return median_us(lambda: hip_ops.jpeg_huffman(table, table_dev, dp["segments"], dp["segments_dev"], dp["work"], dp["work_dev"],
                                                          dp["stream"], dp["huff"], coef_dev, dp["status"], bits // 32),
                             args.iters, args.warmup)

        dec = image_io.JPEGDecoder(dev, threads=16)
        dec_device = image_io.JPEGDecoder(dev, threads=16, entropy="device")
        by_bits = {bits: round(huffman_device(bits), 2) for bits in (256, 512, 1024, 2048)}
        huffman_dev_us = huffman_device(dec_device.subseq_bits)
        equals_host_coef = bool(torch.equal(coef_dev, coef)) and not bool(dp["status"].any())

        def whole():
            dec.batch(batch)
            torch.cuda.synchronize()

        def whole_device():
            dec_device.batch(batch)
            torch.cuda.synchronize()

        split_decs = [image_io.JPEGDecoder(dev, threads=16, entropy="device", subseq_bits=bits, split=split)
                      for bits in split_bits for split in splits]

        def whole_split(d):
            def run():
                d.batch(batch)
                torch.cuda.synchronize()
            return run

        medians = alternating_medians_us([whole, whole_device] + [whole_split(d) for d in split_decs], args.iters, args.warmup)
        whole_us, whole_device_us = medians[0] / B, medians[1] / B
        split_rows = []
        for d, t in zip(split_decs, medians[2:]):
            got_split = d.batch(batch)[-1].cpu().numpy()
            d.raise_if_corrupt()
            split_rows.append(dict(subseq_bits=d.subseq_bits, chunk_subseqs=d.split[0], overlap=d.split[1],
                                   batch_us_per_image=round(t / B, 1), repaired=int(d.repaired.sum()),
                                   chunks=int(len(hip_ops.jpeg_split_chunks(dp["segments"], d.subseq_bits // 32, d.split[0])[0])),
                                   equals_pillow=bool(np.array_equal(got_split, want))))
            d.close()
        got_device = dec_device.batch(batch)[-1].cpu().numpy()
        dec_device.raise_if_corrupt()
        dec.close()
        dec_device.close()
        device_upload = dp["stream_bytes"] + dp["segments"].nbytes + dp["work"].nbytes + hip_ops.JPEG_HUFF_BYTES * B
        iterations = fixpoint_iterations(batch, dec_device.subseq_bits // 32)
        rec = dict(bench="jpeg", batch=B, size=f"{W}x{H}", sampling="4:2:0", quality=QUALITY, iters=args.iters, warmup=args.warmup,
                   file_bytes=int(np.mean([len(f) for f in batch])), huffman_us_per_image_1t=round(host[1], 1),
                   huffman_us_per_image_16t=round(host[16], 1), upload_us=round(upload, 2), upload_bytes=2 * plan["coef_count"],
                   idct_us=round(idct, 2), idct_copy_us=round(idct_copy, 2), idct_over_copy=round(idct / idct_copy, 3),
                   idct_bytes=idct_bytes, to_rgb_us=round(to_rgb, 2), to_rgb_copy_us=round(rgb_copy, 2),
                   to_rgb_over_copy=round(to_rgb / rgb_copy, 3), to_rgb_bytes=rgb_bytes, batch_us_per_image=round(whole_us, 1),
                   pillow_us_per_image=round(pillow, 1), equals_pillow=bool(np.array_equal(got, want)),
                   scan_prepare_us_per_image_1t=round(sweep_us[1], 1), scan_prepare_us_per_image_16t=round(sweep_us[16], 1),
                   subseq_bits=dec_device.subseq_bits, huffman_device_us=round(huffman_dev_us, 2), huffman_device_us_by_bits=by_bits,
                   segments=int(len(dp["segments"])), device_upload_bytes=int(device_upload),
                   batch_device_us_per_image=round(whole_device_us, 1), device_equals_host_coefficients=equals_host_coef,
                   device_equals_pillow=bool(np.array_equal(got_device, want)), fixpoint_iterations=iterations)
        if split_rows:
            rec["split"] = split_rows
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
