"""The one-launch AdamW on the GPU: the kernel against its host twin (bit for bit) and against
torch.optim.AdamW (no further from the float64 restatement than twice torch's own float32 result, the bar measured in the
test), skipped parameters and groups, the fused gradient clear, state interchange with torch in both directions,
checkpoint / resume, the reference's scheduler, version counters and the trainer's repacked weights, run-to-run identity."""
import copy
import os

import numpy as np
import pytest
import torch

import adamw_restated as R

pytestmark = pytest.mark.gpu


def ours(hp=None, **kw):
    from two_stage_object_detection_amd.optim import AdamW
    return lambda params: AdamW(params, betas=R.BETAS, eps=R.EPS, **(hp or {}), **kw)


def torch_adamw(hp):
    return lambda params: torch.optim.AdamW(params, betas=R.BETAS, eps=R.EPS, **hp)


def offset_view(x, dev):
    """A leaf parameter that starts one element (4 bytes) into its storage: the kernel's 4-byte path."""
    base = torch.zeros(x.numel() + 1, device=dev)
    base[1:] = x.to(dev)
    p = base[1:].detach().requires_grad_(True)
    assert p.data_ptr() % 16 == 4 and p.is_contiguous()
    return p


# ----------------------------------------------------------------------------------------------- 4. kernel == host twin
@pytest.mark.parametrize("hp", R.HYPER, ids=["train_py", "lr1e-2_wd0.1"])
def test_kernel_equals_host_twin_after_every_step(dev, hp):
    """The inputs of the CPU test plus a parameter viewed from one element into its storage and one of 49 chunks + a tail
    (100 003 elements): p, exp_avg and exp_avg_sq bit-identical to the host twin after each of 40 steps."""
    from two_stage_object_detection_amd import hip_ops
    sizes = R.SIZES + (5001,)
    params, grads = R.draw_params(sizes), R.draw_grads(sizes)
    P = [x.clone().to(dev).requires_grad_(True) for x in params[:-1]] + [offset_view(params[-1], dev)]
    opt = ours(hp)(P)
    tp = [x.numpy().copy() for x in params]
    tm, tv = [np.zeros_like(x) for x in tp], [np.zeros_like(x) for x in tp]
    worst = 0
    for t, row in enumerate(grads, 1):
        for p, g in zip(P, row):
            p.grad = g.to(dev)
        opt.step()
        h = hip_ops.adamw_group(hp["lr"], R.BETAS[0], R.BETAS[1], R.EPS, hp["weight_decay"], t)
        for i, g in enumerate(row):
            hip_ops.adamw_step_host(tp[i], g.numpy().copy(), tm[i], tv[i], h)
        for name, got, want in (("p", P, tp), ("exp_avg", [opt.state[p]["exp_avg"] for p in P], tm),
                                ("exp_avg_sq", [opt.state[p]["exp_avg_sq"] for p in P], tv)):
            for i, (a, b) in enumerate(zip(got, want)):
                differ = int((a.detach().cpu() != torch.from_numpy(b)).sum())
                worst = max(worst, differ)
                if differ:
                    print(f"step {t} {name}[{i}] (numel {b.size}): {differ} elements differ from the host twin")
                assert differ == 0, (t, name, i, differ)
    print(f"kernel vs host twin lr={hp['lr']}: {worst} differing elements over 40 steps")
    assert float(opt.state[P[0]]["step"]) == 40 and opt.state[P[0]]["step"].device.type == "cpu"


# ---------------------------------------------------------------------------------- 5. kernel against torch.optim.AdamW
@pytest.mark.parametrize("hp", R.HYPER, ids=["train_py", "lr1e-2_wd0.1"])
def test_kernel_against_torch_and_restatement(dev, hp):
    params, grads = R.draw_params(), R.draw_grads()
    exact = R.run_restated(params, grads, **hp)
    ref = R.run_optimizer(torch_adamw(hp), params, grads)[0]                     # torch.optim.AdamW, CPU float32
    got = R.run_optimizer(ours(hp), params, grads, device=dev)[0]
    R.assert_within_twice_reference(got, ref, exact, f"kernel lr={hp['lr']}")


# --------------------------------------------------------------------------------------------------- 6. skips and groups
def test_skipped_parameters_and_two_groups(dev):
    from two_stage_object_detection_amd.optim import AdamW
    sizes = (18, 4097, 33333, 700)
    params, grads = R.draw_params(sizes), R.draw_grads(sizes, steps=5)
    P = [x.clone().to(dev).requires_grad_(True) for x in params]
    hp = [dict(lr=1e-3, weight_decay=1e-2), dict(lr=3e-2, weight_decay=0.2)]
    opt = AdamW([dict(params=P[:2], **hp[0]), dict(params=P[2:], **hp[1])], betas=R.BETAS, eps=R.EPS)
    for row in grads:
        for p, g in zip(P[:3], row):
            p.grad = g.to(dev)
        opt.step()
    assert P[3].grad is None and torch.equal(P[3].detach().cpu(), params[3]) and P[3] not in opt.state
    assert len(opt.state) == 3
    for sl, h in ((slice(0, 2), hp[0]), (slice(2, 3), hp[1])):
        sub = [row[sl] for row in grads]
        exact = R.run_restated(params[sl], sub, **h)
        ref = R.run_optimizer(torch_adamw(h), params[sl], sub)[0]
        got = ([p.detach().cpu() for p in P[sl]],) + R.state_lists(opt, P[sl])
        R.assert_within_twice_reference(got, ref, exact, f"group lr={h['lr']}")
    # a parameter that gets its first gradient later starts at step 1 beside others at step 6: still one launch, own scalars
    P[3].grad = grads[0][3].to(dev)
    for p, g in zip(P[:3], grads[0]):
        p.grad = g.to(dev)
    opt.step()
    assert float(opt.state[P[3]]["step"]) == 1 and float(opt.state[P[2]]["step"]) == 6
    late = R.run_optimizer(ours(hp[1]), [params[3]], [[grads[0][3]]], device=dev)[0]
    assert torch.equal(P[3].detach().cpu(), late[0][0])


def test_rejected_inputs(dev):
    from two_stage_object_detection_amd._ffi import TsodError
    from two_stage_object_detection_amd.optim import AdamW
    with pytest.raises(TsodError, match="float32"):
        AdamW([torch.zeros(4, device=dev, dtype=torch.float16, requires_grad=True)])
    with pytest.raises(TsodError, match="contiguous"):
        AdamW([torch.zeros(6, 4, device=dev).t().requires_grad_(True)])
    p = torch.zeros(4, 6, device=dev, requires_grad=True)
    opt = AdamW([p])
    for bad, msg in ((torch.zeros(6, 4, device=dev).t(), "contiguous"), (torch.zeros(4, 6, device=dev).to_sparse(), "sparse")):
        p.grad = bad
        with pytest.raises(TsodError, match=msg):
            opt.step()
        assert p not in opt.state
    p.grad = torch.ones(4, 6, device=dev)
    opt.step()
    assert float(opt.state[p]["step"]) == 1 and float(p.detach().abs().min()) > 0
    p.grad = torch.zeros(6, 4, device=dev).t()                    # caught on a later step too: the layout is checked again
    with pytest.raises(TsodError, match="contiguous"):
        opt.step()
    assert float(opt.state[p]["step"]) == 1
    p.grad = None
    loss = opt.step(closure=lambda: (p.sum().backward(), torch.is_grad_enabled())[1])
    assert loss is True and float(opt.state[p]["step"]) == 2


def trainer_on(dev):
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    return FasterRCNNTrainer(mode="train", num_classes=80).to(dev).eval()


def test_one_launch_for_the_trainers_236_parameters(dev, monkeypatch):
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.optim import AdamW
    tr = trainer_on(dev)
    named = list(tr.named_parameters())
    assert len(named) == 236
    heads = [p for n, p in named if n.startswith(("rpn.", "head."))]
    rest = [p for n, p in named if not n.startswith(("rpn.", "head."))]
    opt = AdamW([dict(params=rest, lr=1e-4), dict(params=heads, lr=1e-3, weight_decay=0.0)])
    gen = torch.Generator(device=dev).manual_seed(3)
    before = [p.detach().clone() for _, p in named]
    for _, p in named:
        p.grad = torch.randn(p.shape, device=dev, generator=gen)
    calls = []
    real = hip_ops.adamw_step
    monkeypatch.setattr(hip_ops, "adamw_step", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    opt.step()
    assert calls == [236]
    opt.step(zero_grad=True)
    assert calls == [236, 236]
    assert all(not torch.equal(p.detach(), b) for (_, p), b in zip(named, before))
    assert all(float(p.grad.abs().max()) == 0 for _, p in named)


# ------------------------------------------------------------------------------------------- 7. the fused gradient clear
def test_step_zero_grad_keeps_gradients_allocated_and_matches_set_to_none(dev):
    sizes = (18, 81, 4097, 33333)
    params, grads = R.draw_params(sizes), R.draw_grads(sizes, steps=8)
    A = [x.clone().to(dev).requires_grad_(True) for x in params]
    B = [x.clone().to(dev).requires_grad_(True) for x in params]
    oa, ob = ours(R.HYPER[1])(A), ours(R.HYPER[1])(B)
    ptrs = None
    for cycle in range(2):                                        # two accumulation cycles of four micro-batches each
        for row in grads[4 * cycle:4 * cycle + 4]:
            for plist in (A, B):
                for p, g in zip(plist, row):
                    g = g.to(dev)
                    if p.grad is None:
                        p.grad = g.clone()
                    else:
                        p.grad += g
        oa.step(zero_grad=True)
        assert all(p.grad is not None and int((p.grad != 0).sum()) == 0 for p in A)
        if ptrs is None:
            ptrs = [p.grad.data_ptr() for p in A]
        assert ptrs == [p.grad.data_ptr() for p in A]
        ob.step()
        ob.zero_grad(set_to_none=True)                            # reallocates next cycle: the table is rebuilt
        assert all(p.grad is None for p in B)
    assert R.bit_equal([p.detach() for p in A], [p.detach() for p in B])
    for k in range(2):
        assert R.bit_equal(R.state_lists(oa, A)[k], R.state_lists(ob, B)[k])


# ------------------------------------------------------------------------------------------- 8. interchange with torch
def continue_with(make_opt, dev, params, state, grads):
    """A new optimizer on clones of ``params`` loaded with ``state``, stepped over ``grads`` -> (p, exp_avg, exp_avg_sq)."""
    P = [x.clone().to(dev).requires_grad_(True) for x in params]
    opt = make_opt(P)
    opt.load_state_dict(copy.deepcopy(state))      # (torch.load gives every reader its own tensors; a live dict does not)
    for row in grads:
        for p, g in zip(P, row):
            p.grad = g.to(dev)
        opt.step()
    return ([p.detach().cpu() for p in P],) + R.state_lists(opt, P)


@pytest.mark.parametrize("first", ["ours", "torch"])
def test_state_interchange_with_torch(dev, first):
    """3 steps with one optimizer, its state_dict loaded into the other, 3 more steps there: the trajectory continues.  The
    bar: twice the distance of torch.optim.AdamW's own 6 steps (same device) from the float64 restatement."""
    hp = R.HYPER[1]
    params, grads = R.draw_params(), R.draw_grads(steps=6)
    exact = R.run_restated(params, grads, **hp)
    ref = R.run_optimizer(torch_adamw(hp), params, grads, device=dev)[0]
    makers = dict(ours=ours(hp), torch=torch_adamw(hp))
    second = "torch" if first == "ours" else "ours"
    head, opt, P, _, _ = R.run_optimizer(makers[first], params, grads[:3], device=dev)
    sd = opt.state_dict()
    assert all(st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 3
               for st in sd["state"].values())
    crossed = continue_with(makers[second], dev, head[0], sd, grads[3:])
    stayed = continue_with(makers[first], dev, head[0], sd, grads[3:])
    R.assert_within_twice_reference(crossed, ref, exact, f"{first} -> {second}")
    R.assert_within_twice_reference(stayed, ref, exact, f"{first} -> {first}")


def test_checkpoint_resume_is_bit_identical(dev, tmp_path):
    """train.py's three-key checkpoint through torch.save / torch.load(weights_only=True): the resumed run's next step is the
    uninterrupted run's, bit for bit, at the scheduler's learning rate."""
    from torch.optim.lr_scheduler import CosineAnnealingLR
    hp = dict(lr=1e-2, weight_decay=1e-4)
    sizes = (18, 4097, 33333)
    params, grads = R.draw_params(sizes), R.draw_grads(sizes, steps=4)
    cosine = lambda o: CosineAnnealingLR(o, T_max=5)
    whole, *_ = R.run_optimizer(ours(hp), params, grads, device=dev, scheduler=cosine)
    head, opt, P, lrs, sched = R.run_optimizer(ours(hp), params, grads[:3], device=dev, scheduler=cosine)
    path = os.path.join(tmp_path, "ckpt.pth")
    torch.save({"model_state_dict": {str(i): p.detach() for i, p in enumerate(P)}, "optimizer_state_dict": opt.state_dict(),
                "scheduler_state_dict": sched.state_dict()}, path)
    ck = torch.load(path, weights_only=True)
    Q = [ck["model_state_dict"][str(i)].clone().to(dev).requires_grad_(True) for i in range(len(sizes))]
    opt2 = ours(hp)(Q)
    sched2 = cosine(opt2)
    opt2.load_state_dict(ck["optimizer_state_dict"])
    sched2.load_state_dict(ck["scheduler_state_dict"])
    assert opt2.param_groups[0]["lr"] == sched.get_last_lr()[0] != hp["lr"]
    for p, g in zip(Q, grads[3]):
        p.grad = g.to(dev)
    opt2.step()
    assert R.bit_equal([p.detach() for p in Q], whole[0])
    m, v = R.state_lists(opt2, Q)
    assert R.bit_equal(m, whole[1]) and R.bit_equal(v, whole[2])


# ------------------------------------------------------------------------------------------------------- 9. the scheduler
def test_cosine_annealing_drives_every_step(dev):
    """CosineAnnealingLR(T_max=5) over 12 epochs of one step: each step runs at that epoch's get_last_lr(), down to 0 at epoch 5
    and up again after it.  Against the restatement fed the same learning rates; bar: torch.optim.AdamW under the same
    scheduler on the CPU."""
    from torch.optim.lr_scheduler import CosineAnnealingLR
    hp = dict(lr=1e-2, weight_decay=1e-4)
    params, grads = R.draw_params(), R.draw_grads(steps=12)
    cosine = lambda o: CosineAnnealingLR(o, T_max=5)
    ref, _, _, ref_lrs, _ = R.run_optimizer(torch_adamw(hp), params, grads, scheduler=cosine)
    P = [x.clone().to(dev).requires_grad_(True) for x in params]
    opt = ours(hp)(P)
    sched = cosine(opt)
    lrs = []
    for row in grads:
        for p, g in zip(P, row):
            p.grad = g.to(dev)
        lrs.append(sched.get_last_lr()[0])
        opt.step()
        sched.step()
    assert lrs == ref_lrs and lrs[0] == 1e-2 and abs(lrs[5]) < 1e-12 and lrs[4] < lrs[3] and lrs[6] > lrs[5] and lrs[9] > lrs[7]
    exact = R.run_restated(params, grads, lrs=lrs, **hp)
    got = ([p.detach().cpu() for p in P],) + R.state_lists(opt, P)
    R.assert_within_twice_reference(got, ref, exact, "cosine")
    wrong = R.run_restated(params, grads, **hp)                                   # a constant learning rate is far outside the bar
    assert R.max_err(got[0], wrong[0]) > 100 * R.max_err(ref[0], exact[0])


# --------------------------------------------------------------------------------- 10. version counters and the trainer
def test_version_counters_advance(dev):
    params, grads = R.draw_params((18, 4097)), R.draw_grads((18, 4097), steps=3)
    P = [x.clone().to(dev).requires_grad_(True) for x in params]
    opt = ours(R.HYPER[0])(P)
    for row in grads:
        for p, g in zip(P, row):
            p.grad = g.to(dev)
        before = [p._version for p in P]
        opt.step()
        assert all(p._version >= b + 1 for p, b in zip(P, before))


def test_trainer_runs_the_stepped_weights(dev, golden_dir):
    """forward, (losses[-1] / 32).backward(), AdamW(model.parameters(), lr=1e-2).step() on a head_grads trainer with a frozen
    backbone: the next forward equals, bit for bit, that of a fresh trainer loaded with the stepped state_dict - the packed
    weights were rebuilt because step() advanced the version counters (remove that call and the losses stay the old ones)."""
    from test_trainer_grads import grad_trainer, image, t
    from two_stage_object_detection_amd.optim import AdamW
    z = np.load(os.path.join(golden_dir, "trainer_ref.npz"))
    x, bbox, label = image(z)[None].to(dev), t(z, "bbox").to(dev), t(z, "label").to(dev)
    tr = grad_trainer(dev)
    backbone_before = {k: p.detach().clone() for k, p in tr.feat_extra.named_parameters()}
    opt = AdamW(tr.parameters(), lr=1e-2)
    losses = tr(x, [bbox], [label])[0]
    (losses[-1] / 32).backward()
    opt.step()
    with torch.no_grad():
        after = tr(x, [bbox], [label])
    fresh = grad_trainer(dev)
    fresh.load_state_dict({k: v.cpu() for k, v in tr.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(x, [bbox], [label])
    old = torch.stack([l.detach() for l in losses])
    got_l, want_l = torch.stack(after[0]), torch.stack(want[0])
    print("losses before the step", old.tolist(), "after", got_l.tolist(), "fresh trainer", want_l.tolist())
    assert not torch.equal(got_l, old)
    assert torch.equal(got_l, want_l)
    for k in (1, 2, 3):                                            # anchors_pred, classes_pred, classes_score_pred
        assert torch.equal(after[k], want[k]), k
    named = dict(tr.named_parameters())
    stepped = [p for p in named.values() if p in opt.state]
    assert len(stepped) == 8 and all(p.requires_grad for p in stepped)
    for k, p in tr.feat_extra.named_parameters():
        assert p not in opt.state and torch.equal(p.detach(), backbone_before[k]), k


# ---------------------------------------------------------------------------------------------------- 11. run to run
def test_two_runs_give_the_same_bits(dev):
    params, grads = R.draw_params(), R.draw_grads(steps=10)
    a = R.run_optimizer(ours(R.HYPER[1]), params, grads, device=dev, step_kw=dict(zero_grad=True))[0]
    b = R.run_optimizer(ours(R.HYPER[1]), params, grads, device=dev, step_kw=dict(zero_grad=True))[0]
    for x, y in zip(a, b):
        assert R.bit_equal(x, y)
