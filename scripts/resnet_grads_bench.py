"""The launches of a ResNet identity Bottleneck's backward on tensors of ResNet-50's layer4.2, for a
kernel trace or on their own:

    rocprofv3 --kernel-trace --stats -d OUT -o resnet -- python scripts/resnet_grads_bench.py --shape 1x800x1333 --reps 10
    python scripts/resnet_grads_bench.py --shape 8x800x1333 --reps 10 >> profiles/resnet_grads_mi355x.jsonl

Per launch group of one backward pass (in the autograd node's order) and per forward launch of the same layer (the yardstick)
it prints one JSON line: the HIP-event time per pass (mean of `reps` passes of that group back to back, after two warm-up
passes), the bytes it must move, its FLOPs and the paper bound max(bytes / 6.3 TB/s, FLOPs / 157.3 TFLOP/s).  `--refresh`
adds the host time of one forward after an in-place change of the trained blocks (packs dropped and made again, plan
assembled again) beside a forward that finds everything in place."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import _ffi, hip_ops  # noqa: E402

HBM, MFMA = 6.3e12, 157.3e12


def timed(fn, reps):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def refresh_time(dev):
    from two_stage_object_detection_amd.models.resnet import resnet50
    torch.manual_seed(0)
    m = resnet50(include_top=False).to(dev).eval()
    m.requires_grad_(False)
    m.train_blocks(2)
    for p in m.trainable_parameters():
        p.requires_grad_(True)
    x = torch.rand(1, 3, 800, 1333, device=dev)

    def forward():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m(x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    forward()
    steady = min(forward() for _ in range(3))
    after = []
    for _ in range(3):
        with torch.no_grad():
            for p in m.trainable_parameters():
                p.mul_(1.0)                                        # (what an optimizer step does to ``_version``)
        after.append(forward())
    return dict(launch="host: forward after a step (2 blocks re-packed, plan re-assembled) / steady forward", shape="1x800x1333",
                ms_after_step=round(min(after), 2), ms_steady=round(steady, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x800x1333", help="batch x image height x image width")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=512, help="the block's mid channels (layer4: 512)")
    ap.add_argument("--refresh", action="store_true")
    a = ap.parse_args()
    N, IH, IW = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    H, W = (IH + 31) // 32, (IW + 31) // 32                    # layer4's stride is 32
    M, Cm, Co = N * H * W, a.width, 4 * a.width
    gen = torch.Generator(device=dev).manual_seed(0)

    def rnd(*s):
        return torch.randn(*s, device=dev, generator=gen)
    x, y1, y2, y3, d3 = rnd(N, H, W, Co), rnd(N, H, W, Cm), rnd(N, H, W, Cm), rnd(N, H, W, Co), rnd(N, H, W, Co)
    w1, w2, w3 = rnd(Cm, 1, 1, Co) / Co ** 0.5, rnd(Cm, 3, 3, Cm) / (9 * Cm) ** 0.5, rnd(Co, 1, 1, Cm) / Cm ** 0.5
    s1, s2, s3 = (torch.rand(c, device=dev, generator=gen) + 0.5 for c in (Cm, Cm, Co))
    b1, b2, b3 = (rnd(c) for c in (Cm, Cm, Co))
    rot = hip_ops.rotate_conv3x3_weight(w2, s2)
    g3, g2, g1 = torch.empty_like(y3), torch.empty_like(y2), torch.empty_like(y1)
    d2, dx = torch.empty_like(y2), torch.empty_like(x)
    out1, out3 = torch.empty_like(y1), torch.empty_like(y3)
    L = _ffi.lib()
    ws1, ws3 = L.tsod_pw_wgrad_workspace_bytes(M, Cm, Co), L.tsod_pw_wgrad_workspace_bytes(M, Co, Cm)
    ws2 = L.tsod_conv3x3_dense_wgrad_workspace_bytes(N, H, W, Cm, Cm)
    pw = hip_ops.conv1x1_bn_relu6_grad
    f = 4
    groups = [
        ("prelu_grad on y3 / y1+y2 (3 launches + 3 finishes)", lambda: (hip_ops.prelu_grad(y3, d3, 0.25, g=g3), hip_ops.prelu_grad(y2, d2, 0.25, g=g2),
                                                                        hip_ops.prelu_grad(y1, d2, 0.25, g=g1)), 3 * M * (Co + 2 * Cm) * f, 4 * M * (Co + 2 * Cm)),
        ("conv3: pw_wgrad (partial + finish)", lambda: pw(y2, [(0, Cm)], w3, s3, None, g3, want_dx=False), M * (Co + Cm) * f + 2 * ws3, 2 * M * Co * Cm),
        ("conv3: pw_dgrad", lambda: pw(y2, [(0, Cm)], w3, s3, None, g3, dx=d2, want_dw=False, want_dscale=False, want_dshift=False),
         M * (Co + Cm) * f, 2 * M * Co * Cm),
        ("conv2: conv3x3_dense_wgrad (partial + finish)", lambda: hip_ops.conv3x3_dense_wgrad(g2, y1, w2, s2), 2 * M * Cm * f + 2 * ws2, 2 * M * Cm * 9 * Cm),
        ("conv2: dgrad through the forward library (rotated image)", lambda: hip_ops.conv2d_nhwc(g2, rot, pad=1, out=out1),
         (2 * M * Cm + 9 * Cm * Cm) * f, 2 * M * Cm * 9 * Cm),
        ("conv1: pw_wgrad (partial + finish)", lambda: pw(x, [(0, Co)], w1, s1, None, g1, want_dx=False), M * (Co + Cm) * f + 2 * ws1, 2 * M * Co * Cm),
        ("conv1: pw_dgrad (accumulate)", lambda: pw(x, [(0, Co)], w1, s1, None, g1, dx=dx, accumulate=True, want_dw=False, want_dscale=False,
                                                   want_dshift=False), M * (2 * Co + Cm) * f, 2 * M * Co * Cm),
        ("yardstick: forward conv1 (1x1)", lambda: hip_ops.conv2d_nhwc(x, w1, scale=s1, shift=b1, act=_ffi.ACT_PRELU, slope=0.25, out=out1),
         (M * (Co + Cm) + Co * Cm) * f, 2 * M * Co * Cm),
        ("yardstick: forward conv2 (3x3)", lambda: hip_ops.conv2d_nhwc(y1, w2, pad=1, scale=s2, shift=b2, act=_ffi.ACT_PRELU, slope=0.25, out=out1),
         (2 * M * Cm + 9 * Cm * Cm) * f, 2 * M * Cm * 9 * Cm),
        ("yardstick: forward conv3 (1x1 + residual)", lambda: hip_ops.conv2d_nhwc(y2, w3, scale=s3, shift=b3, residual=x, act=_ffi.ACT_PRELU, slope=0.25,
                                                                                 out=out3), (M * (2 * Co + Cm) + Co * Cm) * f, 2 * M * Co * Cm),
    ]
    for name, fn, nbytes, flops in groups:
        us = timed(fn, a.reps)
        bound = max(nbytes / HBM, flops / MFMA) * 1e6
        print(json.dumps(dict(launch=name, shape=a.shape, pixels=M, us_per_pass=round(us, 1), bytes=nbytes, flops=flops,
                              us_bound=round(bound, 1), percent_of_bound=round(100 * bound / us, 1))), flush=True)
    if a.refresh:
        print(json.dumps(refresh_time(dev)), flush=True)


if __name__ == "__main__":
    main()
