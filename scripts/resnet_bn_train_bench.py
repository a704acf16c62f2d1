"""What train-mode BatchNorm with ResNet's epilogue costs, as JSON lines:

    python scripts/resnet_bn_train_bench.py [--iters 20] [--warmup 3] [--reps 200]

(a) wall time per forward + backward of resnet50 at 1 x 3 x 600 x 600 in the modes "layer4" and "stem", folded BatchNorm under
    .eval() (the path of sections 4.22 / 4.23) against ``batch_stats=True`` under .train(): ``iters`` iterations after
    ``warmup``, one synchronize at the end;
(b) per kernel group of csrc/bn_train.hip, at (M, C) = (22 500, 256) (layer1's output at 600 x 600) and (361, 2048)
(layer4's), HIP-event time of ``reps`` back-to-back calls of the C entry points on preallocated tensors (no Python wrapper, no
allocation inside the window), beside a device copy (``Tensor.copy_``) of one tensor of the same shape:
  stats + apply          tsod_bn_stats_f32 + tsod_bn_apply_prelu_f32 with a residual tensor (4 passes over the tensor's bytes)
  fused grad             tsod_bn_prelu_train_grad_f32 with g_out (8 passes; 3 launches)
  the pair it replaces   tsod_prelu_grad_f32 + tsod_bn_train_grad_f32 on the same inputs (8 passes; 5 launches), in the same run,
                         alternating with the fused grad, three rounds each (the spread is printed)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import hip_ops  # noqa: E402
from two_stage_object_detection_amd._ffi import check, lib, ptr  # noqa: E402

SLOPE = 0.25


def step_time(m, x, gy, iters, warmup):
    def step():
        for p in m.trainable_parameters():
            p.grad = None
        m(x).backward(gy)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def module_steps(dev, iters, warmup):
    from two_stage_object_detection_amd.models.resnet import resnet50
    x = torch.rand(1, 3, 600, 600, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    for mode in ("layer4", "stem"):
        ms = {}
        for batch_stats in (False, True):
            torch.manual_seed(0)
            m = resnet50(include_top=False).requires_grad_(False).to(dev)
            m.train_from(mode, batch_stats=batch_stats)
            m.train(batch_stats)
            for p in m.trainable_parameters():
                p.requires_grad_(True)
            gy = torch.randn_like(m(x).detach())
            ms[batch_stats] = step_time(m, x, gy, iters, warmup)
            print(json.dumps(dict(workload=f"resnet50 train_from({mode!r}) forward+backward 1x3x600x600, {iters} iterations after "
                                           f"{warmup}", batch_stats=batch_stats, ms_per_iter=round(ms[batch_stats], 3))))
            del m
        print(json.dumps(dict(mode=mode, ratio_batch_stats_over_folded=round(ms[True] / ms[False], 3))))


def event_us(fn, reps):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def kernel_groups(dev, M, C, reps):
    L, st = lib(), hip_ops.stream_ptr()
    gen = torch.Generator(device=dev).manual_seed(M + C)
    z, r, dy = (torch.randn(M, C, device=dev, generator=gen) for _ in range(3))
    gamma, beta = torch.rand(C, device=dev, generator=gen) + 0.5, torch.randn(C, device=dev, generator=gen)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y, dz, g, dst = (torch.empty_like(z) for _ in range(4))
    mean, invstd, dgamma, dbeta = (torch.empty(C, device=dev) for _ in range(4))
    scale, shift = torch.empty(2, C, device=dev), torch.empty(2, C, device=dev)
    num = torch.empty(1, device=dev)
    ws_bytes = max(L.tsod_bn_prelu_train_grad_workspace_bytes(M, C), L.tsod_bn_train_workspace_bytes(M, C),
                   L.tsod_prelu_grad_workspace_bytes(M, C))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def forward():
        check(L.tsod_bn_stats_f32(ptr(z), M, C, C, C, 0, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(rm), ptr(rv), None, ptr(mean), ptr(invstd),
                                  ptr(scale), ptr(shift), ptr(ws), ws_bytes, st), "bn_stats")
        check(L.tsod_bn_apply_prelu_f32(ptr(z), M, C, C, C, 0, ptr(scale), ptr(shift), ptr(r), C, 0, None, 0, 0, None, None, SLOPE,
                                        ptr(y), C, 0, None, st), "bn_apply_prelu")

    def fused():
        check(L.tsod_bn_prelu_train_grad_f32(ptr(y), C, 0, ptr(dy), C, 0, ptr(z), C, 0, M, C, C, ptr(mean), ptr(invstd), ptr(gamma),
                                             SLOPE, ptr(dz), C, 0, ptr(dgamma), ptr(dbeta), ptr(num), ptr(g), C, 0, ptr(ws), ws_bytes,
                                             st), "bn_prelu_train_grad")

    def pair():
        check(L.tsod_prelu_grad_f32(ptr(y), M, C, C, ptr(dy), C, 0, SLOPE, ptr(g), C, ptr(num), ptr(ws), ws_bytes, st), "prelu_grad")
        check(L.tsod_bn_train_grad_f32(ptr(g), C, 0, ptr(z), C, 0, M, C, C, ptr(mean), ptr(invstd), ptr(gamma), ptr(dz), C, 0,
                                       ptr(dgamma), ptr(dbeta), ptr(ws), ws_bytes, st), "bn_train_grad")
    forward()
    fused()
    kept = [t.clone() for t in (dz, dgamma, dbeta, g)]
    pair()
    same = all(torch.equal(a, b) for a, b in zip(kept, (dz, dgamma, dbeta, g)))       # (the slope's sum is f64 in one, f32 in the other)
    copy_us = event_us(lambda: dst.copy_(z), reps)
    fwd_us = event_us(forward, reps)
    rounds = [(event_us(fused, reps), event_us(pair, reps)) for _ in range(3)]
    f_us, p_us = min(a for a, _ in rounds), min(b for _, b in rounds)
    base = dict(rows=M, C_pad=C, tensor_bytes=z.numel() * 4, copy_of_tensor_us=round(copy_us, 2))
    print(json.dumps(dict(kernels="bn_stats (partial + finish) + bn_apply_prelu (residual)", launches=3, passes=4, us=round(fwd_us, 2), **base)))
    print(json.dumps(dict(kernels="bn_prelu_train_grad with g_out (partial + finish + dz)", launches=3, passes=8, us=round(f_us, 2),
                          us_rounds=[round(a, 2) for a, _ in rounds], **base)))
    print(json.dumps(dict(kernels="prelu_grad + bn_train_grad (the pair)", launches=5, passes=8, us=round(p_us, 2),
                          us_rounds=[round(b, 2) for _, b in rounds], dz_dgamma_dbeta_g_bits_equal_fused=same, **base)))
    print(json.dumps(dict(rows=M, C_pad=C, fused_over_pair=round(f_us / p_us, 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    module_steps(dev, a.iters, a.warmup)
    for M, C in ((22500, 256), (361, 2048)):
        kernel_groups(dev, M, C, a.reps)


if __name__ == "__main__":
    main()
