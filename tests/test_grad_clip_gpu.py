"""Gradient clipping by global norm on the GPU: the norm kernels against their host twin (bit for
bit: aligned, 4-byte-aligned, more than 256 chunks, inf and NaN), the clipped one-launch step against multiply-then-step,
the non-finite norm, optim.clip_grad_norm_, the launch structure, run-to-run identity and the scheduler."""
import numpy as np
import pytest
import torch

import adamw_restated as R
import grad_clip_restated as C

pytestmark = pytest.mark.gpu

HP = [dict(lr=1e-3, weight_decay=1e-2), dict(lr=3e-2, weight_decay=0.2)]
CLIPS, KEEPS = 1.0, 1e30                   # the drawn gradients' norm is about 50: the first clips, the second does not


def offset_copy(x, dev):
    """A copy of ``x`` that starts one element (4 bytes) into its storage: the kernels' 4-byte path."""
    base = torch.zeros(x.numel() + 1, device=dev)
    base[1:] = x.to(dev)
    v = base[1:1 + x.numel()]
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def work_list(tensors, dev):
    """Device table and chunks over ``tensors`` as gradients (only `grad` and `n` of a record are read by the norm)."""
    from two_stage_object_detection_amd import hip_ops
    numels = [t.numel() for t in tensors]
    table = hip_ops.adamw_table([(t.data_ptr(),) * 4 for t in tensors], numels, [0] * len(tensors), 1)
    chunks = hip_ops.adamw_chunks(numels)
    return torch.from_numpy(table).to(dev), torch.from_numpy(chunks).to(dev)


def kernel_record(tensors, max_norm, dev):
    """tsod_grad_norm_f32 over device tensors -> the device record."""
    from two_stage_object_detection_amd import hip_ops
    table, chunks = work_list(tensors, dev)
    workspace = torch.full((max(chunks.shape[0], 1),), float("nan"), dtype=torch.float64, device=dev)
    record = hip_ops.grad_norm_record(dev)
    hip_ops.grad_norm(table, chunks, max_norm, record, workspace)
    return record


def read(record):
    """(sum_sq, norm, coef) of a device record as numpy scalars."""
    host = record.cpu().numpy()
    f = host.view(np.float32)
    return np.float64(host[0]), np.float32(f[2]), np.float32(f[3])


def twin(grads, max_norm):
    from two_stage_object_detection_amd import hip_ops
    return hip_ops.grad_norm_host([np.ascontiguousarray(g.numpy()) for g in grads], max_norm)


# ------------------------------------------------------------------------------------------------- 1. kernel == host twin
SIZE_SETS = [C.SIZES] + [(n,) for n in C.SIZES] + [(2048 * 300,)]


@pytest.mark.parametrize("sizes", SIZE_SETS, ids=["all"] + [str(n) for n in C.SIZES] + ["300_chunks"])
def test_norm_kernel_equals_host_twin(dev, sizes):
    """Aligned tensors and the same values from base[1:1 + n] (4-byte loads): both equal the host twin bit for bit.  2048 x 300
    elements: the finish workgroup takes a second round past 256 partials."""
    grads = C.draw_grads(sizes)
    want = twin(grads, CLIPS)
    aligned = [g.to(dev) for g in grads]
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    got = read(kernel_record(aligned, CLIPS, dev))
    shifted = read(kernel_record([offset_copy(g, dev) for g in grads], CLIPS, dev))
    mixed = read(kernel_record([offset_copy(g, dev) if i % 2 else g.to(dev) for i, g in enumerate(grads)], CLIPS, dev))
    print(f"sizes {sizes}: kernel {got}, 4-byte path {shifted}, host twin {want}")
    assert C.same_record(got, want), (got, want)
    assert C.same_record(shifted, want), (shifted, want)
    assert C.same_record(mixed, want), (mixed, want)
    assert C.ulp_distance_f32(got[1], C.exact_norm(grads)) <= 1.0


@pytest.mark.parametrize("special", ["zeros", "below", "inf", "nan", "max_norm_0"])
def test_norm_kernel_special_values(dev, special):
    grads, max_norm = C.draw_grads(), CLIPS
    if special == "zeros":
        grads = [torch.zeros_like(g) for g in grads]
    elif special == "below":
        max_norm = KEEPS
    elif special == "inf":
        grads[4][2047] = float("-inf")
    elif special == "nan":
        grads[6][4099] = float("nan")
    else:
        max_norm = 0.0
    want = twin(grads, max_norm)
    got = read(kernel_record([g.to(dev) for g in grads], max_norm, dev))
    print(f"{special}: kernel {got}, host twin {want}")
    assert C.same_record(got, want), (got, want)
    if special in ("zeros", "below"):
        assert got[2] == 1.0
    if special == "inf":
        assert np.isinf(got[1]) and got[2] == 0.0
    if special == "nan":
        assert np.isnan(got[1]) and np.isnan(got[2])


def test_empty_work_list_writes_zero_zero_one(dev):
    """Through the C entry point: an empty torch tensor has no pointer to pass."""
    from two_stage_object_detection_amd import _ffi, hip_ops
    g = torch.ones(4, device=dev)
    table, chunks = work_list([g], dev)
    workspace = torch.zeros(1, dtype=torch.float64, device=dev)
    for n_tensors, n_chunks in ((1, 0), (0, 1), (0, 0)):
        record = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
        rc = _ffi.lib().tsod_grad_norm_f32(table.data_ptr(), n_tensors, chunks.data_ptr(), n_chunks, 0.0, record.data_ptr(),
                                           workspace.data_ptr(), 8, _ffi.stream_ptr())
        assert rc == 0 and read(record) == (0.0, 0.0, 1.0), (n_tensors, n_chunks)
    record = hip_ops.grad_norm_record(dev)
    hip_ops.grad_norm(table, chunks, 4.0, record, workspace)
    assert read(record) == (4.0, 2.0, 1.0)


def test_parameter_without_gradient_is_skipped(dev):
    from two_stage_object_detection_amd.optim import AdamW
    sizes = (18, 2049, 4100)
    grads = C.draw_grads(sizes)
    P = [torch.zeros(n, device=dev, requires_grad=True) for n in sizes]
    P[0].grad, P[2].grad = grads[0].to(dev), grads[2].to(dev)
    opt = AdamW(P, **HP[0])
    opt.step(max_grad_norm=CLIPS)
    want = twin([grads[0], grads[2]], CLIPS)
    assert C.same_bits(np.float32(opt.grad_norm.item()), want[1])
    assert P[1].grad is None and P[1] not in opt.state and float(P[1].detach().abs().max()) == 0


# ---------------------------------------------------------------------------------------------- 2. fused against composed
def two_groups(dev, params):
    from two_stage_object_detection_amd.optim import AdamW
    P = [x.clone().to(dev).requires_grad_(True) for x in params[:-1]] + [offset_copy(params[-1], dev).detach().requires_grad_(True)]
    opt = AdamW([dict(params=P[:2], **HP[0]), dict(params=P[2:], **HP[1])], betas=R.BETAS, eps=R.EPS)
    return P, opt


FUSED_SIZES = (18, 2047, 4100, 5001)


@pytest.mark.parametrize("zero_grad", [False, True], ids=["keep_grads", "zero_grad"])
@pytest.mark.parametrize("max_norm", [CLIPS, KEEPS], ids=["clips", "does_not_clip"])
def test_clipped_step_equals_multiply_then_step(dev, max_norm, zero_grad):
    """step(max_grad_norm=m, zero_grad=z) against: the coefficient read from a record, torch._foreach_mul_(grads, coef),
    step(zero_grad=z) - parameters, exp_avg and exp_avg_sq bit for bit after each of 5 steps, two groups, one parameter on
    the 4-byte path.  With a non-clipping m also against step() without the keyword."""
    params = R.draw_params(FUSED_SIZES)
    A, oa = two_groups(dev, params)
    B, ob = two_groups(dev, params)
    Q, oq = two_groups(dev, params)
    ptrs = None
    for t in range(5):
        row = C.draw_grads(FUSED_SIZES, seed=10 + t)
        for plist in (A, B, Q):
            for p, g in zip(plist, row):
                if p.grad is None:
                    p.grad = g.to(dev) if p.data_ptr() % 16 == 0 else offset_copy(g, dev)
                else:
                    p.grad.copy_(g)
        if ptrs is None:
            ptrs = [p.grad.data_ptr() for p in A]
        record = kernel_record([p.grad for p in B], max_norm, dev)
        coef = record.view(torch.float32)[3]
        want_norm, want_coef = read(record)[1:]
        clipped = [p.grad * coef for p in B]
        oa.step(max_grad_norm=max_norm, zero_grad=zero_grad)
        torch._foreach_mul_([p.grad for p in B], coef)
        ob.step(zero_grad=zero_grad)
        assert C.same_bits(np.float32(oa.grad_norm.item()), want_norm)
        assert (want_coef < 1.0) == (max_norm == CLIPS)
        for name, got, want in (("p", A, B), ("exp_avg", R.state_lists(oa, A)[0], R.state_lists(ob, B)[0]),
                                ("exp_avg_sq", R.state_lists(oa, A)[1], R.state_lists(ob, B)[1])):
            for i, (a, b) in enumerate(zip(got, want)):
                assert torch.equal(a.detach().cpu(), b.detach().cpu()), (t, name, i)
        assert ptrs == [p.grad.data_ptr() for p in A]                     # the same storage either way
        if zero_grad:
            assert all(int((p.grad != 0).sum()) == 0 for p in A)
        else:
            assert all(torch.equal(p.grad, c) for p, c in zip(A, clipped))   # g * coef, as after torch's clip
        if max_norm == KEEPS:
            oq.step(zero_grad=zero_grad)
            assert R.bit_equal([p.detach() for p in A], [p.detach() for p in Q])
            for k in range(2):
                assert R.bit_equal(R.state_lists(oa, A)[k], R.state_lists(oq, Q)[k])
    assert all(float(oa.state[p]["step"]) == 5 for p in A)


def test_rejected_max_grad_norm(dev):
    from two_stage_object_detection_amd.optim import AdamW
    p = torch.ones(8, device=dev, requires_grad=True)
    p.grad = torch.ones(8, device=dev)
    opt = AdamW([p])
    for bad in (-1.0, float("inf"), float("nan"), "1", torch.tensor(1.0)):
        with pytest.raises(ValueError):
            opt.step(max_grad_norm=bad)
    with pytest.raises(ValueError):
        opt.step(error_if_nonfinite=True)
    assert p not in opt.state and float(p.detach().min()) == 1 and opt.grad_norm is None
    assert set(opt.param_groups[0]) == set(torch.optim.AdamW([torch.zeros(1, requires_grad=True)]).param_groups[0])
    assert set(opt.state_dict()) == {"state", "param_groups"}
    q = torch.ones(8, device=dev, requires_grad=True)                     # no gradient anywhere: no norm
    none = AdamW([q])
    none.step(max_grad_norm=1.0)
    assert none.grad_norm is None


# ------------------------------------------------------------------------------------------------- 3. the non-finite norm
@pytest.mark.parametrize("first_step", [True, False], ids=["first_step", "later_step"])
def test_error_if_nonfinite_leaves_everything_unchanged(dev, first_step):
    sizes = (18, 2049, 700)
    params = R.draw_params(sizes)
    P, opt = two_groups(dev, params)
    if not first_step:
        for p, g in zip(P, C.draw_grads(sizes)):
            p.grad = g.to(dev)
        opt.step(max_grad_norm=CLIPS)
    bad = C.draw_grads(sizes, seed=9)
    bad[1][100] = float("inf")
    for p, g in zip(P, bad):
        p.grad = g.to(dev)
    before = [p.detach().clone() for p in P]
    state = [{k: v.clone() for k, v in opt.state[p].items()} for p in P if p in opt.state]
    with pytest.raises(RuntimeError, match="non-finite, so it cannot be clipped"):
        opt.step(max_grad_norm=CLIPS, error_if_nonfinite=True)
    assert all(torch.equal(p.detach(), b) for p, b in zip(P, before))
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(P, bad))
    if first_step:
        assert len(opt.state) == 0
    else:
        for p, old in zip(P, state):
            assert float(opt.state[p]["step"]) == 1
            assert all(torch.equal(opt.state[p][k], old[k]) for k in old)
    assert torch.isinf(opt.grad_norm)
    # the default lets it through, as torch does: coef = 0, inf * 0 = NaN in the parameter that held the inf
    opt.step(max_grad_norm=CLIPS)
    assert not torch.isfinite(P[1].detach()).all()
    assert float(opt.state[P[1]]["step"]) == (1 if first_step else 2)


# ------------------------------------------------------------------------------------------------ 4. optim.clip_grad_norm_
def test_clip_grad_norm_function(dev):
    from two_stage_object_detection_amd import optim
    from two_stage_object_detection_amd._ffi import TsodError
    grads = C.draw_grads()
    P = [torch.zeros(g.numel(), device=dev, requires_grad=True) for g in grads] + [torch.zeros(3, device=dev, requires_grad=True)]
    for p, g in zip(P, grads):
        p.grad = g.to(dev)
    want = twin(grads, CLIPS)
    norm = optim.clip_grad_norm_(P, CLIPS)
    assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.device == P[0].device
    assert C.same_bits(np.float32(norm.item()), want[1]) and want[2] < 1
    assert C.ulp_distance_f32(np.float32(norm.item()), C.exact_norm(grads)) <= 1.0
    for p, g in zip(P, grads):
        assert torch.equal(p.grad.cpu(), g * torch.tensor(want[2])), p.shape
    assert P[-1].grad is None
    first = float(norm)
    again = optim.clip_grad_norm_(P, CLIPS)                               # now about 1: below max + 1e-6 or a hair above
    assert float(norm) == first and abs(float(again) - 1.0) < 1e-5       # the first result is the caller's own
    one = optim.clip_grad_norm_(P[0], KEEPS, norm_type=2)                 # a single tensor, nothing clipped
    assert C.same_bits(np.float32(one.item()), twin([P[0].grad.cpu()], KEEPS)[1])
    empty = optim.clip_grad_norm_([P[-1]], CLIPS)
    assert empty.dim() == 0 and float(empty) == 0.0
    for bad in (1, float("inf"), 1.5):
        with pytest.raises(ValueError):
            optim.clip_grad_norm_(P, CLIPS, norm_type=bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            optim.clip_grad_norm_(P, bad)
    cpu = torch.zeros(4, requires_grad=True)
    cpu.grad = torch.ones(4)
    with pytest.raises(TsodError, match="no CPU fallback"):
        optim.clip_grad_norm_([cpu], CLIPS)
    f64 = torch.zeros(4, device=dev, dtype=torch.float64, requires_grad=True)
    f64.grad = torch.ones(4, device=dev, dtype=torch.float64)
    with pytest.raises(TsodError, match="float32"):
        optim.clip_grad_norm_([P[0], f64], CLIPS)
    P[1].grad[0] = float("nan")
    kept = [p.grad.clone() for p in P[:-1]]
    with pytest.raises(RuntimeError, match="non-finite"):
        optim.clip_grad_norm_(P, CLIPS, error_if_nonfinite=True)
    assert all(torch.equal(p.grad, k) or i == 1 for i, (p, k) in enumerate(zip(P, kept)))
    assert torch.isnan(optim.clip_grad_norm_(P, CLIPS))


# ------------------------------------------------------------------------------------------------- 5. launch structure
def test_one_norm_call_and_one_clipped_step_call(dev, monkeypatch):
    from two_stage_object_detection_amd import hip_ops
    sizes = (18, 2049, 4100)
    P, opt = two_groups(dev, R.draw_params(sizes))
    for p, g in zip(P, C.draw_grads(sizes)):
        p.grad = g.to(dev)
    calls = []

    def spy(name):
        real = getattr(hip_ops, name)
        monkeypatch.setattr(hip_ops, name, lambda *a, **k: (calls.append(name), real(*a, **k))[1])
    for name in ("grad_norm", "adamw_step_clipped", "adamw_step", "grad_scale", "adamw_table", "adamw_chunks"):
        spy(name)
    opt.step(max_grad_norm=CLIPS)
    assert calls == ["adamw_table", "adamw_chunks", "grad_norm", "adamw_step_clipped"]
    del calls[:]
    opt.step(max_grad_norm=CLIPS, zero_grad=True)                         # the table is not uploaded again
    assert calls == ["grad_norm", "adamw_step_clipped"]
    del calls[:]
    opt.step()                                                            # a plain step is still its single call
    opt.step(zero_grad=True)
    assert calls == ["adamw_step", "adamw_step"]


# ----------------------------------------------------------------------------------------------------- 6. repeatability
def test_two_runs_give_the_same_bits(dev):
    from two_stage_object_detection_amd.optim import AdamW
    sizes = C.SIZES + (2048 * 20 + 7,)
    params = R.draw_params(sizes)
    rows = [C.draw_grads(sizes, seed=20 + t) for t in range(4)]
    runs = []
    for _ in range(2):
        norms = []
        P = [x.clone().to(dev).requires_grad_(True) for x in params]
        opt = AdamW(P, **HP[1])
        for row in rows:
            for p, g in zip(P, row):
                p.grad = g.to(dev)
            opt.step(max_grad_norm=CLIPS)
            norms.append(opt.grad_norm.clone())
        runs.append(([p.detach().cpu() for p in P], R.state_lists(opt, P), torch.stack(norms).cpu(), [p.grad.cpu() for p in P]))
    a, b = runs
    assert R.bit_equal(a[0], b[0]) and R.bit_equal(a[1][0], b[1][0]) and R.bit_equal(a[1][1], b[1][1])
    assert torch.equal(a[2], b[2]) and R.bit_equal(a[3], b[3])


# --------------------------------------------------------------------------------------------------------- 7. the scheduler
def test_cosine_annealing_drives_the_clipped_step(dev):
    from torch.optim.lr_scheduler import CosineAnnealingLR
    from two_stage_object_detection_amd.optim import AdamW
    sizes = (18, 2049)
    params = R.draw_params(sizes)
    hp = dict(lr=1e-2, weight_decay=1e-4)

    def run(clip_kw, pre=None):
        P = [x.clone().to(dev).requires_grad_(True) for x in params]
        opt = AdamW(P, betas=R.BETAS, eps=R.EPS, **hp)
        sched = CosineAnnealingLR(opt, T_max=5)
        lrs, norms = [], []
        for t in range(7):
            for p, g in zip(P, C.draw_grads(sizes, seed=30 + t)):
                p.grad = g.to(dev)
            if pre is not None:
                pre(P)
            lrs.append(sched.get_last_lr()[0])
            opt.step(**clip_kw)
            sched.step()
            norms.append(opt.grad_norm)
        return [p.detach().cpu() for p in P], lrs, norms

    from two_stage_object_detection_amd import optim
    got, lrs, norms = run(dict(max_grad_norm=CLIPS))
    want, want_lrs, _ = run({}, pre=lambda P: optim.clip_grad_norm_(P, CLIPS))
    assert lrs == want_lrs and lrs[0] == 1e-2 and abs(lrs[5]) < 1e-12 and lrs[6] > lrs[5]
    assert all(n is not None and n.dim() == 0 and n.is_cuda and float(n) > 1 for n in norms)
    assert R.bit_equal(got, want)
