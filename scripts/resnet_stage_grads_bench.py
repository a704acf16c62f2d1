"""The launches of a ResNet projection Bottleneck's backward on tensors of ResNet-50's layer4.0 (x
[N,50,84,1024] -> [N,25,42,2048] at 800x1333: stride 2 on the 3x3 and on the 1x1 shortcut), on their own:

    python scripts/resnet_stage_grads_bench.py --shape 1x800x1333 --reps 10 >> profiles/resnet_stage_grads_mi355x.jsonl
    python scripts/resnet_stage_grads_bench.py --shape 8x800x1333 --reps 10 >> profiles/resnet_stage_grads_mi355x.jsonl

Per launch group of one backward pass (in the autograd node's order) and per forward launch of the same layer (the yardstick)
it prints one JSON line: the HIP-event time per pass (mean of `reps` passes of that group back to back, after two warm-up
passes), the bytes it must move, its FLOPs and the paper bound max(bytes / 6.3 TB/s, FLOPs / 157.3 TFLOP/s).  The stride-2 3x3's
input gradient runs 16 / 9 of the minimal MACs (the 2x2 phase pack); its line counts the MACs it runs and names the minimal
ones."""
import argparse
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x800x1333", help="batch x image height x image width")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=512, help="the block's mid channels (layer4: 512; the input has 2 width channels)")
    a = ap.parse_args()
    N, IH, IW = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    H, W = (IH + 15) // 16, (IW + 15) // 16                    # the block's input: layer3's stride is 16
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M1, M2, Cm, Ci, Co = N * H * W, N * OH * OW, a.width, 2 * a.width, 4 * a.width
    gen = torch.Generator(device=dev).manual_seed(0)

    def rnd(*s):
        return torch.randn(*s, device=dev, generator=gen)
    x, y1, y2, y3, d3 = rnd(N, H, W, Ci), rnd(N, H, W, Cm), rnd(N, OH, OW, Cm), rnd(N, OH, OW, Co), rnd(N, OH, OW, Co)
    w1, w2, w3, wd = (rnd(Cm, 1, 1, Ci) / Ci ** 0.5, rnd(Cm, 3, 3, Cm) / (9 * Cm) ** 0.5, rnd(Co, 1, 1, Cm) / Cm ** 0.5,
                      rnd(Co, 1, 1, Ci) / Ci ** 0.5)
    s1, s2, s3, sd = (torch.rand(c, device=dev, generator=gen) + 0.5 for c in (Cm, Cm, Co, Co))
    b1, b2, b3 = (rnd(c) for c in (Cm, Cm, Co))
    s2d = hip_ops.s2d_conv3x3_weight(w2, s2)
    stacked = torch.cat([w3.flatten(1) * s3.view(-1, 1), wd.flatten(1) * sd.view(-1, 1)], dim=1).contiguous()
    g3, g2 = torch.empty_like(y3), torch.empty_like(y2)
    d2, dx, xs, dxs = torch.empty_like(y2), torch.empty_like(x), hip_ops.pixel_subsample(x, 2), torch.empty(N, OH, OW, Ci, device=dev)
    p = torch.empty(N, OH + 1, OW + 1, 4 * Cm, device=dev)
    out1, out2, out3 = torch.empty_like(y1), torch.empty_like(y2), torch.empty_like(y3)
    L = _ffi.lib()
    ws1, ws3, wsd = (L.tsod_pw_wgrad_workspace_bytes(M1, Cm, Ci), L.tsod_pw_wgrad_workspace_bytes(M2, Co, Cm),
                     L.tsod_pw_wgrad_workspace_bytes(M2, Co, Ci))
    ws2 = L.tsod_conv3x3_strided_wgrad_workspace_bytes(N, H, W, Cm, Cm, 2)
    pw = hip_ops.conv1x1_bn_relu6_grad
    no_w = dict(want_dw=False, want_dscale=False, want_dshift=False)
    f = 4
    PM = N * (OH + 1) * (OW + 1)
    groups = [
        ("prelu_grad on y3 and y2 (2 launches + 2 finishes)", lambda: (hip_ops.prelu_grad(y3, d3, 0.25, g=g3), hip_ops.prelu_grad(y2, d2, 0.25, g=g2)),
         3 * M2 * (Co + Cm) * f, 4 * M2 * (Co + Cm)),
        ("conv3: pw_wgrad (partial + finish)", lambda: pw(y2, [(0, Cm)], w3, s3, None, g3, want_dx=False), M2 * (Co + Cm) * f + 2 * ws3, 2 * M2 * Co * Cm),
        ("conv3: pw_dgrad", lambda: pw(y2, [(0, Cm)], w3, s3, None, g3, dx=d2, **no_w), M2 * (Co + Cm) * f, 2 * M2 * Co * Cm),
        ("shortcut: pixel_subsample", lambda: hip_ops.pixel_subsample(x, 2), 2 * M2 * Ci * f, 0),
        ("shortcut: pw_wgrad (partial + finish)", lambda: pw(xs, [(0, Ci)], wd, sd, None, g3, want_dx=False), M2 * (Co + Ci) * f + 2 * wsd, 2 * M2 * Co * Ci),
        ("shortcut: pw_dgrad", lambda: pw(xs, [(0, Ci)], wd, sd, None, g3, dx=dxs, **no_w), M2 * (Co + Ci) * f, 2 * M2 * Co * Ci),
        ("shortcut: pixel_upsample_add", lambda: hip_ops.pixel_upsample_add(dx, dxs, 2), 3 * M2 * Ci * f, M2 * Ci),
        ("conv2: conv3x3_strided_wgrad (partial + finish)", lambda: hip_ops.conv3x3_strided_wgrad(g2, y1, w2, s2, stride=2),
         (M1 + M2) * Cm * f + 2 * ws2, 2 * M2 * Cm * 9 * Cm),
        (f"conv2: dgrad through the forward library (2x2 phase pack; the minimal FLOPs are {2 * M2 * Cm * 9 * Cm})",
         lambda: hip_ops.conv2d_nhwc(g2, s2d, pad=1, out=p), (M2 * Cm + PM * 4 * Cm + 16 * Cm * Cm) * f, 2 * PM * 4 * Cm * 4 * Cm),
        ("prelu_grad_d2s on y1 (launch + finish)", lambda: hip_ops.prelu_grad_d2s(y1, p, 0.25), 3 * M1 * Cm * f, 4 * M1 * Cm),
        ("conv1: pw_wgrad (partial + finish)", lambda: pw(x, [(0, Ci)], w1, s1, None, y1, want_dx=False), M1 * (Ci + Cm) * f + 2 * ws1, 2 * M1 * Ci * Cm),
        ("conv1: pw_dgrad (write)", lambda: pw(x, [(0, Ci)], w1, s1, None, y1, dx=dx, **no_w), M1 * (Ci + Cm) * f, 2 * M1 * Ci * Cm),
        ("yardstick: forward conv1 (1x1)", lambda: hip_ops.conv2d_nhwc(x, w1, scale=s1, shift=b1, act=_ffi.ACT_PRELU, slope=0.25, out=out1),
         (M1 * (Ci + Cm) + Ci * Cm) * f, 2 * M1 * Ci * Cm),
        ("yardstick: forward conv2 (3x3, stride 2)", lambda: hip_ops.conv2d_nhwc(y1, w2, stride=2, pad=1, scale=s2, shift=b2, act=_ffi.ACT_PRELU,
                                                                               slope=0.25, out=out2), ((M1 + M2) * Cm + 9 * Cm * Cm) * f, 2 * M2 * Cm * 9 * Cm),
        ("yardstick: forward conv3 + shortcut (one stacked GEMM)", lambda: hip_ops.conv2d_nhwc(y2, stacked, shift=b3, act=_ffi.ACT_PRELU, slope=0.25,
                                                                                              segs=[(0, Cm)], x2=x, stride2=2, out=out3),
         (M2 * (Cm + Ci + Co) + Co * (Cm + Ci)) * f, 2 * M2 * Co * (Cm + Ci)),
    ]
    for name, fn, nbytes, flops in groups:
        us = timed(fn, a.reps)
        bound = max(nbytes / HBM, flops / MFMA) * 1e6
        print(json.dumps(dict(launch=name, shape=a.shape, pixels_in=M1, pixels_out=M2, us_per_pass=round(us, 1), bytes=nbytes, flops=flops,
                              us_bound=round(bound, 1), percent_of_bound=round(100 * bound / us, 1))), flush=True)


if __name__ == "__main__":
    main()
