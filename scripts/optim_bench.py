"""Time one optimizer step: the one-launch AdamW against torch.optim.AdamW on the same parameters.
    python scripts/optim_bench.py [--iters N] [--repeats R]

Cases: the trainer's eight head parameters (what head_grads=True trains) and all its 236 parameters (HarDNet-39).
Per case, three optimizers, measured alternately in every repeat (same box, same run):
  ours           two_stage_object_detection_amd.optim.AdamW   step(zero_grad=True)
  torch_default  torch.optim.AdamW (what the reference runs)  step() + zero_grad(set_to_none=False)
  torch_fused    torch.optim.AdamW(fused=True), as information step() + zero_grad(set_to_none=False)
  wall_us   back-to-back steps between two events, per step (host cost included); median, min and max over the repeats
  device_us the sum of kernel durations per step from a torch.profiler kernel trace (a run of its own), and the kernel
            launches per step counted in the same trace
  gbps      algorithmic bytes over device_us: 32 bytes per element with the gradient clear (read p, g, m, v; write p, m, v,
            g), 28 without it in one pass - the generic optimizers clear in a pass of their own, which is part of their step
The gradients start as random tensors and are zero after the first step (every variant clears them): an optimizer's
time does not depend on the gradient's values.  One JSON line per (case, optimizer).

Clipping by global norm (--what clip, or all): the same two parameter sets and the same alternating repeats, three ways
to clip at max_norm = 1 in front of the one-launch step:
  torch_clip+ours  torch.nn.utils.clip_grad_norm_(params, 1.0), then optim.AdamW step(zero_grad=True): what a user does
                   without the fused path - the baseline
  ours_fused_clip  optim.AdamW step(zero_grad=True, max_grad_norm=1.0): norm partials, norm finish, step
  ours_clip+ours   optim.clip_grad_norm_(params, 1.0), then step(zero_grad=True): norm partials, norm finish, scale, step
  gbps here counts 36 bytes per element for the fused path (the norm reads g once more) and 44 for the two composed ones
  (norm read, scale read and write, then the step's 32)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from two_stage_object_detection_amd.nets.frcnn_training import HEAD_PARAMS, FasterRCNNTrainer  # noqa: E402
from two_stage_object_detection_amd.optim import AdamW, clip_grad_norm_  # noqa: E402

HYPER = dict(lr=1e-4, weight_decay=1e-4)           # train/train.py's


def trace(fn, iters):
    """(kernel time per call of fn() in us, kernel launches per call, per-kernel times) from a profiler trace."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    total, count, names = 0.0, 0, {}
    for e in prof.events():
        dt = getattr(e, "device_type", None)
        if dt is None or "CUDA" not in str(dt) or e.device_time_total <= 0:
            continue
        if "Memcpy" in e.name or "Memset" in e.name:
            continue
        total += e.device_time_total
        count += 1
        names[e.name] = names.get(e.name, 0.0) + e.device_time_total
    return total / iters, count / iters, {k: v / iters for k, v in names.items()}


def wall_once(fn, iters):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def measure(case, src, steppers, bytes_per_element, args):
    """Warm up, time the steppers alternately in every repeat, trace each in a run of its own, print one line each."""
    elements = sum(p.numel() for p in src)
    for fn in steppers.values():                                                   # warm-up: state, code objects, tables
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    walls = {name: [] for name in steppers}
    for _ in range(args.repeats):                                                  # alternate them in every repeat
        for name, fn in steppers.items():
            walls[name].append(wall_once(fn, args.iters))
    for name, fn in steppers.items():
        dev_us, launches, per = trace(fn, min(args.iters, 50))
        w = sorted(walls[name])
        print(json.dumps(dict(case=case, optimizer=name, tensors=len(src), elements=elements,
                              wall_us=round(w[len(w) // 2], 2), wall_us_min=round(w[0], 2), wall_us_max=round(w[-1], 2),
                              device_us=round(dev_us, 2), launches_per_step=round(launches, 2),
                              gbps=round(elements * bytes_per_element[name] / dev_us / 1e3, 1) if dev_us > 0 else None,
                              iters=args.iters, repeats=args.repeats,
                              kernels={k[:60]: round(v, 2) for k, v in per.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--what", choices=("step", "clip", "all"), default="all")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tr = FasterRCNNTrainer(mode="train", num_classes=80).to(dev).eval()
    named = dict(tr.named_parameters())
    cases = {"head8": [named[k] for k in HEAD_PARAMS], "trainer236": list(named.values())}
    gen = torch.Generator(device=dev).manual_seed(0)
    for case, src in cases.items():
        if args.what == "clip":
            break
        steppers = {}
        for name, make in (("ours", lambda ps: AdamW(ps, **HYPER)),
                           ("torch_default", lambda ps: torch.optim.AdamW(ps, **HYPER)),
                           ("torch_fused", lambda ps: torch.optim.AdamW(ps, fused=True, **HYPER))):
            ps = [p.detach().clone().requires_grad_(True) for p in src]            # every optimizer its own copy
            for p in ps:
                p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
            opt = make(ps)
            if name == "ours":
                steppers[name] = lambda opt=opt: opt.step(zero_grad=True)
            else:
                steppers[name] = lambda opt=opt: (opt.step(), opt.zero_grad(set_to_none=False))
        measure(case, src, steppers, dict.fromkeys(steppers, 32), args)
    for case, src in cases.items():
        if args.what == "step":
            break
        steppers = {}
        for name in ("torch_clip+ours", "ours_fused_clip", "ours_clip+ours"):
            ps = [p.detach().clone().requires_grad_(True) for p in src]
            for p in ps:
                p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
            opt = AdamW(ps, **HYPER)
            if name == "torch_clip+ours":
                steppers[name] = lambda opt=opt, ps=ps: (torch.nn.utils.clip_grad_norm_(ps, 1.0), opt.step(zero_grad=True))
            elif name == "ours_fused_clip":
                steppers[name] = lambda opt=opt: opt.step(zero_grad=True, max_grad_norm=1.0)
            else:
                steppers[name] = lambda opt=opt, ps=ps: (clip_grad_norm_(ps, 1.0), opt.step(zero_grad=True))
        measure(case, src, steppers, {"torch_clip+ours": 44, "ours_fused_clip": 36, "ours_clip+ours": 44}, args)


if __name__ == "__main__":
    main()
