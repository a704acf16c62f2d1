"""The launches of a HarDBlock section's backward on tensors of HarDNet-39's last block, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o blocks -- python scripts/block_grads_bench.py --shape 1x600x600 --reps 10

Runs, `reps` times: the forward launches of the block's four CombConvLayers and its transition layer (1x1 GEMM + depthwise
3x3 each), then their backward in the order of the autograd node - transition wgrad + dgrad, then per layer (last first) the
depthwise backward with the fused ReLU6 mask, the 1x1's wgrad (+ finish) and dgrad.  Prints, per backward launch, the bytes it
must move and its FLOPs, so that the trace's times can be set against 6.3 TB/s and the f32 MFMA rate (157.3 TFLOP/s)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import _ffi, hip_ops  # noqa: E402
from two_stage_object_detection_amd.models.hardnet import HarDBlock, _pad4  # noqa: E402

HBM, MFMA = 6.3e12, 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x600x600", help="batch x image height x image width")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    N, IH, IW = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    H, W = (IH + 3) // 4, (IW + 3) // 4                        # the trunk's stride is 4
    M = N * H * W
    blk = HarDBlock(640, 160, 1.6, 4, dwconv=True)
    real, offs, P = blk.slice_table()
    g = torch.Generator(device=dev).manual_seed(0)
    buf = torch.rand(N, H, W, P, device=dev, generator=g)
    dbuf = torch.zeros_like(buf)
    layers = []
    for li in list(range(1, 5)) + [0]:                          # 0: the transition layer
        slices, cout = (blk.links[li - 1], real[li]) if li else (blk.output_slices(), 1024)
        cp, segs = _pad4(cout), [(offs[k], _pad4(real[k])) for k in slices]
        K = sum(ln for _, ln in segs)
        layers.append(dict(li=li, cout=cout, cp=cp, segs=segs, K=K, seg_real=[real[k] for k in slices],
                           w=torch.randn(cp, 1, 1, K, device=dev, generator=g) / K ** 0.5,
                           scale=torch.rand(cp, device=dev, generator=g) + 0.5, shift=torch.rand(cp, device=dev, generator=g),
                           y=torch.empty(N, H, W, cp, device=dev), w33=torch.randn(3, 3, cp, device=dev, generator=g) / 3,
                           sc2=torch.rand(cp, device=dev, generator=g) + 0.5, sh2=torch.randn(cp, device=dev, generator=g) / 3))
    g_tr = torch.randn(N, H, W, 1024, device=dev, generator=g)
    rows, f4 = [], 4
    for lay in layers:
        name = f"layer {lay['li']}" if lay["li"] else "transition"
        cp, K = lay["cp"], lay["K"]
        ws = _ffi.lib().tsod_pw_wgrad_workspace_bytes(M, cp, K)
        if lay["li"]:
            rows.append(dict(launch=f"{name}: dwconv3x3_grad_act (reduce + combine + gather)", bytes=4 * M * cp * f4, flops=2 * M * cp * 9 * 3))
        rows.append(dict(launch=f"{name}: pw_wgrad (partial + finish)", bytes=M * (cp + K) * f4 + 2 * ws, flops=2 * M * cp * K))
        rows.append(dict(launch=f"{name}: pw_dgrad", bytes=M * (cp + 2 * K) * f4, flops=2 * M * cp * K))
        rows.append(dict(launch=f"{name}: forward 1x1 GEMM", bytes=M * (cp + K) * f4, flops=2 * M * cp * K))
        if lay["li"]:
            rows.append(dict(launch=f"{name}: forward dwconv3x3", bytes=2 * M * cp * f4, flops=2 * M * cp * 9))
    for _ in range(a.reps):
        for lay in layers:                                        # forward
            hip_ops.conv2d_nhwc(buf, lay["w"], scale=lay["scale"], shift=lay["shift"], act=_ffi.ACT_RELU6, segs=lay["segs"], out=lay["y"])
            if lay["li"]:
                hip_ops.dwconv3x3_nhwc(lay["y"], lay["w33"], lay["sc2"], lay["sh2"], 1, False, out=buf, out_off=offs[lay["li"]])
        grad = g_tr
        for lay in [layers[-1]] + layers[-2::-1]:                 # backward: transition, then layers 4..1
            if lay["li"]:
                grad = hip_ops.dwconv3x3_grad(lay["y"], lay["w33"], lay["sc2"], lay["sh2"], 1, False, dbuf, dy_off=offs[lay["li"]],
                                              act_dx=True)[0]
            hip_ops.conv1x1_bn_relu6_grad(buf, lay["segs"], lay["w"], lay["scale"], None, grad, seg_real=lay["seg_real"],
                                          cout=lay["cout"], dx=dbuf, accumulate=True)
    torch.cuda.synchronize()
    for r in rows:
        r.update(shape=a.shape, pixels=M, us_at_6_3_TBps=round(r["bytes"] / HBM * 1e6, 2), us_at_f32_mfma=round(r["flops"] / MFMA * 1e6, 2))
        print(json.dumps(r))


if __name__ == "__main__":
    main()
