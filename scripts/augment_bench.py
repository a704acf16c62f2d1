"""Time the training transform (TrainTransform) per image against EvalTransform on the same image.
    python scripts/augment_bench.py [--iters N]

Per size (480x640 and 1080x1920 -> 600x600) and setting (every op drawn; every op but contrast; EvalTransform):
  wall   back-to-back ``batch([img], out=NHWC4 buffer)`` calls between two events, per image (host launch cost included)
  kernel the sum of the setting's kernel durations per image from a torch.profiler kernel trace, and the algorithmic
         GB/s over it: u8 source once (twice with contrast: the mean pass), the f32 intermediate written and read, the
         f32 NHWC4 output written.
One JSON line per (size, setting)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd._ffi import NHWC4Images  # noqa: E402
from two_stage_object_detection_amd.dataset.transform import AugmentParams, EvalTransform, TrainTransform  # noqa: E402

ALL_ON = dict(brightness=1.0625, contrast=0.8125, saturation=1.3125, hue=0.03125, contrast_before=False, perm=(2, 0, 1))


def kernel_us(fn, iters):
    """Sum of kernel durations per call of fn() from a profiler trace (device time only)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    total, names = 0.0, {}
    for e in prof.events():
        dt = getattr(e, "device_type", None)
        if dt is None or "CUDA" not in str(dt) or e.device_time_total <= 0:
            continue
        if "Memcpy" in e.name or "Memset" in e.name:
            continue
        total += e.device_time_total
        names[e.name] = names.get(e.name, 0.0) + e.device_time_total
    return total / iters, {k: v / iters for k, v in names.items()}


def wall_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    best = []
    for _ in range(5):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / iters)
    best.sort()
    return best[len(best) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    OH, OW = 600, 600
    buf = NHWC4Images(torch.empty((1, OH, OW, 4), dtype=torch.float32, device=dev))
    for H, W in ((480, 640), (1080, 1920)):
        img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
        r = min(OH / H, OW / W)
        nh, nw = int(H * r), int(W * r)                               # ScaleJitter at scale 1.0
        tf = TrainTransform()
        ev = EvalTransform((OH, OW))
        settings = {
            "all_on": lambda p=AugmentParams(**ALL_ON, flip=True, size=(nh, nw)): tf.batch([img], params=[p], out=buf),
            "no_contrast": lambda p=AugmentParams(**dict(ALL_ON, contrast=None), flip=True, size=(nh, nw)):
                tf.batch([img], params=[p], out=buf),
            "eval_transform": lambda: ev.batch([img], out=buf),
        }
        for name, fn in settings.items():
            wall = wall_us(fn, args.iters)
            kern, per = kernel_us(fn, args.iters)
            src = H * W * 3
            if name == "eval_transform":
                byt = src + OH * OW * 16
            else:
                byt = src * (2 if name == "all_on" else 1) + 2 * 3 * nh * nw * 4 + OH * OW * 16
            rec = dict(size=f"{H}x{W}", setting=name, jitter=f"{nh}x{nw}", wall_us=round(wall, 2), kernel_us=round(kern, 2),
                       gbps=round(byt / kern / 1e3, 1) if kern > 0 else None,
                       kernels={k[:100]: round(v, 2) for k, v in per.items()})
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
