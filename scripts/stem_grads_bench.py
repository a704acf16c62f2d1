"""The launches of the HarDNet-39 stem's backward on tensors of the stem's shapes, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o stem -- python scripts/stem_grads_bench.py --shape 1x600x600 --reps 10

Runs, `reps` times: the forward launch of base.0 (3x3 stride 2, 4 -> 24 channels; the yardstick of the new kernel), then the
stem's backward in the order of the autograd node - base.2's depthwise backward with the fused ReLU6 mask, base.1's wgrad
(+ finish) and dgrad, base.0's tsod_conv3x3_wgrad_f32 (partial + finish).  Prints, per launch, the bytes it must move and its
FLOPs, so that the trace's times can be set against 6.3 TB/s and the f32 MFMA rate (157.3 TFLOP/s)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import _ffi, hip_ops  # noqa: E402

HBM, MFMA = 6.3e12, 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x600x600", help="batch x image height x image width")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    N, H, W = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    c0, c1 = 24, 48                                            # HarDNet-39's first_ch
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    OH2, OW2 = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    M, M2 = N * OH * OW, N * OH2 * OW2
    g = torch.Generator(device=dev).manual_seed(0)
    x4 = torch.rand(N, H, W, 4, device=dev, generator=g)
    w0 = torch.randn(c0, 3, 3, 4, device=dev, generator=g) / 5
    w0[..., 3] = 0
    sc0, sh0 = torch.rand(c0, device=dev, generator=g) + 0.5, torch.rand(c0, device=dev, generator=g)
    y0 = torch.empty(N, OH, OW, c0, device=dev)
    w1 = torch.randn(c1, c0, device=dev, generator=g) / c0 ** 0.5
    sc1 = torch.rand(c1, device=dev, generator=g) + 0.5
    y1 = torch.rand(N, OH, OW, c1, device=dev, generator=g) * 7 - 0.5
    w33 = torch.randn(3, 3, c1, device=dev, generator=g) / 3
    sc2, sh2 = torch.rand(c1, device=dev, generator=g) + 0.5, torch.randn(c1, device=dev, generator=g) / 3
    d_out = torch.randn(N, OH2, OW2, c1, device=dev, generator=g)
    d0 = torch.zeros(N, OH, OW, c0, device=dev)
    L = _ffi.lib()
    ws0 = L.tsod_conv3x3_wgrad_workspace_bytes(N, H, W, c0, 2)
    ws1 = L.tsod_pw_wgrad_workspace_bytes(M, c1, c0)
    f4 = 4
    rows = [
        dict(launch="base.0: forward conv3x3 s2", bytes=(N * H * W * 4 + M * c0) * f4, flops=2 * M * c0 * 27),
        dict(launch="base.2: dwconv3x3_grad_act (reduce + combine + gather)", bytes=(3 * M * c1 + M2 * c1) * f4, flops=2 * M2 * c1 * 9 * 3),
        dict(launch="base.1: pw_wgrad (partial + finish)", bytes=M * (c1 + c0) * f4 + 2 * ws1, flops=2 * M * c1 * c0),
        dict(launch="base.1: pw_dgrad", bytes=M * (c1 + 2 * c0) * f4, flops=2 * M * c1 * c0),
        dict(launch="base.0: conv3x3_wgrad (partial + finish)", bytes=(N * H * W * 4 + 2 * M * c0) * f4 + 2 * ws0, flops=2 * M * c0 * 27,
             slices=ws0 // (32 * 33 * 4), workspace_bytes=ws0),
    ]
    for _ in range(a.reps):
        hip_ops.conv2d_nhwc(x4, w0, stride=2, pad=1, scale=sc0, shift=sh0, act=_ffi.ACT_RELU6, out=y0)
        g1 = hip_ops.dwconv3x3_grad(y1, w33, sc2, sh2, 2, False, d_out, act_dx=True)[0]
        hip_ops.conv1x1_bn_relu6_grad(y0, [(0, c0)], w1, sc1, None, g1, dx=d0, accumulate=True)
        hip_ops.conv3x3_bn_relu6_grad(x4, w0, sc0, y0, d0, stride=2)
    torch.cuda.synchronize()
    for r in rows:
        r.update(shape=a.shape, pixels=M, us_at_6_3_TBps=round(r["bytes"] / HBM * 1e6, 2), us_at_f32_mfma=round(r["flops"] / MFMA * 1e6, 2))
        print(json.dumps(r))


if __name__ == "__main__":
    main()
