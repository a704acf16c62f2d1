"""The launches of the backward of ResNet-50's stem on the tensors a seeded resnet50 saves at the given
image size, on their own:

    python scripts/resnet_stem_grads_bench.py --shape 1x800x1333 --reps 10 >> profiles/resnet_stem_grads_mi355x.jsonl
    python scripts/resnet_stem_grads_bench.py --shape 8x800x1333 --reps 10 >> profiles/resnet_stem_grads_mi355x.jsonl

Per new launch group, per forward launch of the same layer (the yardstick: the per-launch conv1 and tsod_maxpool3x3s2_f32) and
for one whole backward pass of layer1.0 as the earliest trained block (the existing kernels of sections 4.21 and 4.22, no block
dx) it prints one JSON line: the HIP-event time per pass (mean of `reps` passes back to back, after two warm-up passes, no
profiler attached), the bytes it must move, its FLOPs and the paper bound max(bytes / 6.3 TB/s, FLOPs / 157.3 TFLOP/s).  The
weight gradient's FLOPs are the ones it runs: 224 padded columns per output channel and pixel (147 are real)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import _ffi, hip_ops  # noqa: E402
from two_stage_object_detection_amd.models import resnet_grads  # noqa: E402
from two_stage_object_detection_amd.models.resnet import resnet50  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x800x1333", help="batch x image height x image width")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    N, H, W = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = resnet50(include_top=False).to(dev).eval().train_full()
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(N, 3, H, W, device=dev, generator=gen)
    sv = m.forward_nhwc(x).grad_fn.saved                       # the tensors the node would read; the model's own plan is dropped
    stem, b = sv["stem"], sv["blocks"][0]
    m.drop_plan()
    del sv
    x4, y, w, scale, slope = stem["x4"], stem["y"], stem["w"], stem["scale"], stem["slope"]
    pooled = b["x"]
    _, OH, OW, _ = y.shape
    M, MP = N * OH * OW, pooled.shape[0] * pooled.shape[1] * pooled.shape[2]
    dp = torch.randn(pooled.shape, device=dev, generator=gen)
    g = torch.empty_like(y)
    shift = torch.zeros(64, device=dev)
    out_y, L = torch.empty_like(y), _ffi.lib()
    ws = L.tsod_conv7x7s2_wgrad_workspace_bytes(N, H, W, 64)
    # layer1.0 alone under the autograd node, as the earliest trained block
    names = [f"layer1.0.{k}" for k, _ in m.layer1[0].named_parameters()]
    params = [p for _, p in m.layer1[0].named_parameters()]
    node = resnet_grads._ResNetGrads.apply(dict(out=b["y3"].clone(), nchw=False, names=names, blocks=[b]), *params)
    gy = torch.randn(b["y3"].shape, device=dev, generator=gen)
    f = 4
    groups = [
        ("prelu_grad_pool on the stem's y (launch + finish)", lambda: hip_ops.prelu_grad_pool(y, dp, slope, g=g),
         (2 * M + MP) * 64 * f, 4 * M * 64),
        ("conv1: conv7x7s2_wgrad (partial + finish)", lambda: hip_ops.conv7x7s2_wgrad(g, x4, w, scale),
         (M * 64 + N * H * W * 4) * f + 2 * ws, 2 * M * 64 * 224),
        ("yardstick: forward conv1 (7x7, stride 2, per-launch)",
         lambda: hip_ops.conv2d_nhwc(x4, w, stride=2, pad=3, kw_logical=7, scale=scale, shift=shift, act=_ffi.ACT_PRELU, slope=slope,
                                     out=out_y), (M * 64 + N * H * W * 4 + 64 * 224) * f, 2 * M * 64 * 224),
        ("yardstick: forward tsod_maxpool3x3s2_f32", lambda: hip_ops.maxpool3x3s2_nhwc(y), (M + MP) * 64 * f, 0),
        ("layer1.0: one whole backward pass as the earliest block (existing kernels, no block dx)",
         lambda: node.backward(gy, retain_graph=True), 0, 0),
    ]
    for name, fn, nbytes, flops in groups:
        us = timed(fn, a.reps)
        bound = max(nbytes / HBM, flops / MFMA) * 1e6
        print(json.dumps(dict(launch=name, shape=a.shape, pixels_conv1=M, pixels_pooled=MP, us_per_pass=round(us, 1), bytes=nbytes,
                              flops=flops, us_bound=round(bound, 1), percent_of_bound=round(100 * bound / us, 1) if bound else None)),
              flush=True)


if __name__ == "__main__":
    main()
