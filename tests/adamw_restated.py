"""Shared by tests/test_optim.py and tests/test_optim_gpu.py: the AdamW update of DESIGN.md section 4.16 restated in
float64 torch, seeded inputs, and runners for torch.optim.AdamW on CPU and for the library's host twin.

Gradients are redrawn every step with magnitudes 10^U(-6, 1), random signs, about 5 % exact zeros, and every seventh element
zero in EVERY step, so exp_avg_sq stays 0 there and the denominator is eps alone."""
import numpy as np
import torch

SIZES = (1, 18, 81, 1023, 4097, 33333, 100003)
STEPS = 40
HYPER = (dict(lr=1e-4, weight_decay=1e-4), dict(lr=1e-2, weight_decay=0.1))     # train/train.py's, and a harder pair
BETAS, EPS = (0.9, 0.999), 1e-8


def draw_params(sizes=SIZES, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in sizes]


def draw_grads(sizes=SIZES, steps=STEPS, seed=1):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        row = []
        for n in sizes:
            mag = 10.0 ** (torch.rand(n, generator=g) * 7 - 6)
            sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
            x = (mag * sign).float()
            x[torch.rand(n, generator=g) < 0.05] = 0
            x[3::7] = 0
            row.append(x)
        out.append(row)
    return out


def restated_step(p, g, m, v, t, lr, weight_decay, betas=BETAS, eps=EPS):
    """One update in float64 (tensors in place): the order of include/tsod.h, every scalar in double."""
    b1, b2 = betas
    p.mul_(1 - lr * weight_decay)
    m.add_((g - m) * (1 - b1))
    v.mul_(b2).add_((1 - b2) * g * g)
    denom = v.sqrt() / (1 - b2 ** t) ** 0.5 + eps
    p.add_(-(lr / (1 - b1 ** t)) * m / denom)


def run_restated(params, grads, lrs=None, state=None, first_step=1, **hp):
    """-> (p, exp_avg, exp_avg_sq) lists in float64 after len(grads) steps; ``lrs``: one learning rate per step."""
    p = [x.double().clone() for x in params]
    m, v = state if state is not None else ([torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p])
    m, v = [x.double().clone() for x in m], [x.double().clone() for x in v]
    for s, row in enumerate(grads):
        h = dict(hp)
        if lrs is not None:
            h["lr"] = lrs[s]
        for i, g in enumerate(row):
            restated_step(p[i], g.double(), m[i], v[i], first_step + s, **h)
    return p, m, v


def state_lists(opt, params):
    return ([opt.state[p]["exp_avg"].detach().cpu() for p in params], [opt.state[p]["exp_avg_sq"].detach().cpu() for p in params])


def run_optimizer(make_opt, params, grads, device="cpu", scheduler=None, step_kw=None):
    """``make_opt(list of leaf parameters)`` stepped over ``grads`` -> (p, exp_avg, exp_avg_sq) lists on the CPU, the
    optimizer, its parameters, the learning rate each step ran at, and the scheduler."""
    P = [x.clone().to(device).requires_grad_(True) for x in params]
    opt = make_opt(P)
    sched = scheduler(opt) if scheduler else None
    lrs = []
    for row in grads:
        for p, g in zip(P, row):
            p.grad = g.clone().to(device)
        lrs.append(opt.param_groups[0]["lr"])
        opt.step(**(step_kw or {}))
        if sched is not None:
            sched.step()
    m, v = state_lists(opt, P)
    return ([p.detach().cpu() for p in P], m, v), opt, P, lrs, sched


def run_twin(params, grads, first_step=1, **hp):
    """The library's host twin over the same steps -> (p, exp_avg, exp_avg_sq) lists of float32 tensors."""
    from two_stage_object_detection_amd import hip_ops
    p = [x.numpy().copy() for x in params]
    m, v = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p]
    for s, row in enumerate(grads):
        h = hip_ops.adamw_group(hp["lr"], BETAS[0], BETAS[1], EPS, hp["weight_decay"], first_step + s)
        for i, g in enumerate(row):
            hip_ops.adamw_step_host(p[i], g.numpy().copy(), m[i], v[i], h)
    return tuple([torch.from_numpy(x) for x in xs] for xs in (p, m, v))


def max_err(got, want):
    """max |got - want| over a list of tensors, in float64."""
    return max(float((a.double() - b.double()).abs().max()) for a, b in zip(got, want) if a.numel())


def assert_within_twice_reference(got, ref, exact, what):
    """The rule of DESIGN 4.16: per quantity, max |got - exact| <= 2 * max |torch's own f32 result - exact|."""
    for name, g, r, e in zip(("p", "exp_avg", "exp_avg_sq"), got, ref, exact):
        e_got, e_ref = max_err(g, e), max_err(r, e)
        print(f"{what} {name}: e_got {e_got:.3e}  e_ref {e_ref:.3e}")
        assert e_ref > 0, (what, name)
        assert e_got <= 2 * e_ref, (what, name, e_got, e_ref)


def bit_equal(a, b):
    return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))
