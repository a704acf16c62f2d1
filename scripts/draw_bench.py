"""Time the detection overlay against a device-to-device copy of the same image bytes.
    python scripts/draw_bench.py [--iters N] [--warmup N] [--out profiles/draw_mi355x.jsonl]

600x600 u8 images at batch 1 and 16; per image 8 ground-truth boxes with ``GT: name`` tags and 128 predictions with
``Pred: name`` / ``Conf: d.ddd`` tags (seeded boxes, 2 px outlines), one ``hip_ops.draw_groups`` launch per call.  Every call
is timed on its own between two HIP events, the calls issued back to back; the figure is the median of ``--iters`` calls after
``--warmup`` untimed ones.  The yardstick, timed the same way in the same run, is ``copy_`` of the batch into a second buffer:
the cost of touching every image byte once, which the overlay does not do.  One JSON line per batch size; at batch 16 five more
(``draw_split``): the predictions alone, their outlines alone, their tags alone, all of them outside the image (the cost of
reading the item stream in every tile) and a single box outside it (the cost of the empty launch)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import hip_ops  # noqa: E402
from two_stage_object_detection_amd.utils import overlay  # noqa: E402

H = W = 600
N_PRED, N_GT = 128, 8
NAMES = [f"class{i:02d}" for i in range(80)]


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


def boxes(gen, B, n, lo, hi):
    """Seeded XYXY boxes inside the image with sides in [lo, hi]."""
    wh = torch.rand(B, n, 2, generator=gen) * (hi - lo) + lo
    xy = torch.rand(B, n, 2, generator=gen) * (torch.tensor([W, H], dtype=torch.float32) - wh)
    return torch.cat([xy, xy + wh], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    if args.iters < 20 or args.warmup < 3:
        ap.error("at least 20 timed and 3 warm-up calls")
    dev = torch.device("cuda:0")
    lines = []
    for B in (1, 16):
        gen = torch.Generator().manual_seed(B)
        images = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
        other = torch.empty_like(images)
        pred = torch.cat([boxes(gen, B, N_PRED, 20, 300), torch.rand(B, N_PRED, 1, generator=gen),
                          torch.randint(0, 80, (B, N_PRED, 1), generator=gen).float()], dim=-1).to(dev)
        gt = boxes(gen, B, N_GT, 40, 400).to(dev)
        gt_labels = torch.randint(0, 80, (B, N_GT), generator=gen).to(dev)
        strings = torch.cat([overlay.encode_strings(NAMES, "GT: "), overlay.encode_strings(NAMES, "Pred: ")]).to(dev)
        style = dict(width=2, padding=2, tag_bg=overlay.TAG_BG, tag_alpha=overlay.TAG_ALPHA)
        groups = [dict(boxes=gt, labels=gt_labels, strings=(0, 80), color=overlay.GT_COLOR, tag="above", **style),
                  dict(boxes=pred, strings=(80, 80), color=overlay.PRED_COLOR, tag="below", score_line=True, **style)]
        before = images.clone()
        hip_ops.draw_groups(images, groups, strings)
        touched = int((images != before).any(dim=-1).sum())            # a lower bound: a pixel painted its own colour is not counted
        draw = median_us(lambda: hip_ops.draw_groups(images, groups, strings), args.iters, args.warmup)
        copy = median_us(lambda: other.copy_(images), args.iters, args.warmup)
        rec = dict(bench="draw", batch=B, size=f"{H}x{W}", predictions=N_PRED, ground_truth=N_GT, iters=args.iters,
                   warmup=args.warmup, draw_us=round(draw, 2), copy_us=round(copy, 2), draw_over_copy=round(draw / copy, 3),
                   image_bytes=B * H * W * 3, changed_pixels=touched, changed_fraction=round(touched / (B * H * W), 4))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if B == 16:                                                  # where the time goes: the predictions with parts switched off
            far = pred.clone()
            far[..., :4] += 10000.0
            base = dict(groups[1])
            for case, g in (("predictions", base), ("outlines_only", dict(base, tag="none", score_line=False)),
                            ("tags_only", dict(base, alpha=0)), ("all_outside", dict(base, boxes=far)),
                            ("one_box_outside", dict(base, boxes=far[:, :1].contiguous(), tag="none", score_line=False))):
                t = median_us(lambda: hip_ops.draw_groups(images, [g], strings), args.iters, args.warmup)
                lines.append(json.dumps(dict(bench="draw_split", batch=B, case=case, draw_us=round(t, 2))))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
