"""What train-mode BatchNorm costs, as JSON lines:

    python scripts/bn_train_bench.py [--shape 1x600x600] [--iters 20] [--warmup 3]

(a) wall time per forward + backward of HarDNet-39 with every HarDBlock trainable (``train_blocks(n_blocks)``), folded BatchNorm
    under .eval() against ``batch_stats=True`` under .train(): ``iters`` iterations after ``warmup``, one synchronize at the end
    (the timer of profiles/hardnet_train_refactor_mi355x.jsonl);
(b) per kernel group of csrc/bn_train.hip, HIP-event time on tensors of the first and the last HarDBlock's widest layer against
    a device copy (``Tensor.copy_``) of the bytes the group has to move."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import hip_ops  # noqa: E402
from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction  # noqa: E402


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


def event_us(fn, reps=20):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    N, H, W = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.rand(N, 3, H, W, device=dev)
    ms = {}
    for batch_stats in (False, True):
        torch.manual_seed(0)
        m = HarDNetFeatureExtraction(depth_wise=True, arch=39).requires_grad_(False).to(dev)
        m.train_blocks(m.n_blocks, batch_stats=batch_stats)
        m.train(batch_stats)
        for p in m.trainable_parameters():
            p.requires_grad_(True)
        gy = torch.randn_like(m(x).detach())
        ms[batch_stats] = step_time(m, x, gy, a.iters, a.warmup)
        print(json.dumps(dict(workload=f"hardnet39 train_blocks({m.n_blocks}) forward+backward {N}x3x{H}x{W}, {a.iters} iterations "
                                       f"after {a.warmup}", batch_stats=batch_stats, ms_per_iter=round(ms[batch_stats], 3))))
        del m
    print(json.dumps(dict(ratio_batch_stats_over_folded=round(ms[True] / ms[False], 3))))
    h, w = (H + 3) // 4, (W + 3) // 4
    for C in (28, 160):                                       # a layer of the first HarDBlock, the widest of the last one
        M, cp = N * h * w, (C + 3) // 4 * 4
        z, g = torch.randn(N, h, w, cp, device=dev), torch.randn(N, h, w, cp, device=dev)
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        y, mean, invstd = hip_ops.batch_norm_train(z, gamma, beta, 1e-5, 0.1, rm, rv)
        dz, dst = torch.empty_like(z), torch.empty_like(z)
        one = z.numel() * 4
        copy_us = event_us(lambda: dst.copy_(z))
        fwd = event_us(lambda: hip_ops.batch_norm_train(z, gamma, beta, 1e-5, 0.1, rm, rv, out=y))
        bwd = event_us(lambda: hip_ops.batch_norm_train_grad(g, z, mean, invstd, gamma, dz=dz))
        print(json.dumps(dict(kernels="bn_stats (partial + finish) + bn_apply", rows=M, C_pad=cp, bytes=3 * one, us=round(fwd, 2),
                              copy_of_2x_tensor_bytes_us=round(copy_us, 2), us_per_copy_of_same_bytes=round(fwd / (1.5 * copy_us), 2))))
        print(json.dumps(dict(kernels="bn_train_grad (partial + finish + dz)", rows=M, C_pad=cp, bytes=5 * one, us=round(bwd, 2),
                              copy_of_2x_tensor_bytes_us=round(copy_us, 2), us_per_copy_of_same_bytes=round(bwd / (2.5 * copy_us), 2))))


if __name__ == "__main__":
    main()
