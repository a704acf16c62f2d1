"""What the dropout launch costs, as JSON lines appended to profiles/dropout_mi355x.jsonl:

    python scripts/dropout_bench.py [--shape 1x600x600] [--reps 50] [--out profiles/dropout_mi355x.jsonl]

tsod_dropout_segs_f32 on the output slices of HarDNet-85's last HarDBlock (the block buffer at stride 4: 150 x 150 pixels of
2 408 channels at 600 x 600, of which the three output slices hold 1 252), out of place (the forward's launch) and in place (the
backward's), beside a device copy (``Tensor.copy_``) of the bytes the launch reads and writes: HIP-event time over ``reps``
launches after three warm-up launches.  A measured line, not a bar."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from two_stage_object_detection_amd import hip_ops  # noqa: E402
from two_stage_object_detection_amd.models.hardnet import HarDBlock, HarDNetFeatureExtraction  # noqa: E402


def event_us(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x600x600")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_mi355x.jsonl"))
    a = ap.parse_args()
    N, H, W = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    blk = [m for m in HarDNetFeatureExtraction(depth_wise=True, arch=85).base if isinstance(m, HarDBlock)][-1]
    real, offs, P = blk.slice_table()
    segs, C = [], 0
    for k in blk.output_slices():
        segs.append((offs[k], real[k], C))
        C += real[k]
    h, w = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    buf, dst = torch.randn(N, h, w, P, device=dev), torch.empty(N, h, w, P, device=dev)
    key = hip_ops.dropout_key(dev, 0x1234, 0x5678)
    flat, flat_dst = torch.randn(N * h * w * C, device=dev), torch.empty(N * h * w * C, device=dev)
    rows = dict(out_of_place_us=event_us(lambda: hip_ops.dropout(buf, 0.1, key, segs=segs, C=C, out=dst), a.reps),
                in_place_us=event_us(lambda: hip_ops.dropout(dst, 0.1, key, segs=segs, C=C, out=dst), a.reps),
                copy_us=event_us(lambda: flat_dst.copy_(flat), a.reps))
    moved = 2 * 4 * N * h * w * C
    line = dict(what="tsod_dropout_segs_f32 on hardnet85's last HarDBlock output", shape=f"{N}x3x{H}x{W}", pixels=N * h * w, pitch=P,
                slices=segs, C=C, p=0.1, bytes_read_and_written=moved, reps=a.reps, device=torch.cuda.get_device_name(0),
                time=time.strftime("%Y-%m-%d %H:%M:%S"), **{k: round(v, 2) for k, v in rows.items()},
                out_of_place_gb_per_s=round(moved / rows["out_of_place_us"] * 1e-3, 1),
                copy_gb_per_s=round(moved / rows["copy_us"] * 1e-3, 1),
                out_of_place_over_copy=round(rows["out_of_place_us"] / rows["copy_us"], 2))
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
