"""The launches of the HarDNet tail's backward on tensors of the tail's own shapes, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o tail -- python scripts/tail_grads_bench.py --shape 1x600x600 --reps 25

Runs, `reps` times each: the pair conv's backward, the second depthwise conv's backward (dx wanted), the first one's (ReLU,
no dx), and - the yardstick - the two forward depthwise launches on the same tensors.  Prints the bytes every launch must
move (x + dy read, dx written, partials) so that the trace's times can be set against 6.3 TB/s."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd import _ffi, hip_ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1x600x600", help="batch x image height x image width")
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    N, IH, IW = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    C, G = 1024, 512
    H, W = (IH + 3) // 4, (IW + 3) // 4                        # the trunk's stride is 4, the tail takes it to 16
    H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    H2, W2 = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
    g = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.rand(N, H, W, C, device=dev, generator=g)
    w1, w2 = (torch.randn(3, 3, C, device=dev, generator=g) / 3 for _ in range(2))
    b1, b2 = (torch.randn(C, device=dev, generator=g) / 3 for _ in range(2))
    wg = torch.randn(G, 2, device=dev, generator=g)
    gy = torch.randn(N, H2, W2, G, device=dev, generator=g)
    act = hip_ops.dwconv3x3_nhwc(x0, w1, None, b1, 2, True)
    b = hip_ops.dwconv3x3_nhwc(act, w2, None, b2, 2, False)
    L = _ffi.lib()
    f4 = 4
    ws1 = L.tsod_dwconv3x3_grad_workspace_bytes(N, H, W, C, 2, 0)      # (partials only: no g is written without dx)
    ws2 = L.tsod_dwconv3x3_grad_workspace_bytes(N, H1, W1, C, 2, 0)
    wsp = L.tsod_gconv1x1_pair_grad_workspace_bytes(N * H2 * W2, G)
    rows = [
        dict(launch="gconv1x1_pair_grad", bytes=(b.numel() + gy.numel() + b.numel()) * f4 + 2 * wsp),
        dict(launch="dwconv3x3_grad dw2 (dx)", bytes=(act.numel() + 2 * b.numel() + act.numel()) * f4 + 2 * ws2),
        dict(launch="dwconv3x3_grad dw1 (relu, no dx)", bytes=(x0.numel() + act.numel()) * f4 + 2 * ws1),
        dict(launch="dwconv3x3 forward dw1", bytes=(x0.numel() + act.numel()) * f4),
        dict(launch="dwconv3x3 forward dw2", bytes=(act.numel() + b.numel()) * f4),
    ]
    for _ in range(a.reps):
        d_b, _, _ = hip_ops.gconv1x1_pair_grad(b, wg, gy)
        d_a, _, _, _ = hip_ops.dwconv3x3_grad(act, w2, None, b2, 2, False, d_b)
        hip_ops.dwconv3x3_grad(x0, w1, None, b1, 2, True, d_a, want_dx=False)
        hip_ops.dwconv3x3_nhwc(x0, w1, None, b1, 2, True, out=act)
        hip_ops.dwconv3x3_nhwc(act, w2, None, b2, 2, False, out=b)
    torch.cuda.synchronize()
    for r in rows:
        r.update(shape=a.shape, tail_input=[N, H, W, C], us_at_6_3_TBps=round(r["bytes"] / 6.3e6, 2))
        print(json.dumps(r))


if __name__ == "__main__":
    main()
