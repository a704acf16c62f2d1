"""The reference's optimizer step on HIP: ``AdamW`` updates every parameter of every group in ONE
kernel launch (``hip_ops.adamw_step`` -> csrc/optim.hip), optionally clearing the gradients in the same pass.

It is a ``torch.optim.Optimizer``: param groups, ``state_dict()`` / ``load_state_dict()``, ``zero_grad()`` and every
``torch.optim.lr_scheduler`` work as with ``torch.optim.AdamW``, and the state (``step`` as an f32 CPU scalar, ``exp_avg``,
``exp_avg_sq``) is interchangeable with it in both directions.  HIP only: no CPU fallback.

Gradient clipping by global norm: ``AdamW.step(max_grad_norm=m)`` puts a two-launch deterministic norm in front of the
step and multiplies by the clip coefficient inside it (``hip_ops.grad_norm`` -> ``hip_ops.adamw_step_clipped``);
``clip_grad_norm_`` is the same norm followed by a scaling launch, for use in front of any optimizer.
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from . import hip_ops
from ._ffi import ADAMW_MAX_GROUPS, TsodError

# torch.optim.AdamW's group keys beyond the hyper-parameters, with the only values this optimizer implements
_FIXED = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
              decoupled_weight_decay=True)
# (foreach / fused only pick torch's implementation: any value of a loaded group is accepted and ignored)
_MUST_MATCH = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


def _check_group(group) -> None:
    for key in _MUST_MATCH:
        if group.get(key, _FIXED[key]) != _FIXED[key]:
            raise ValueError(f"AdamW (HIP): {key}={group[key]!r} is not implemented; only {key}={_FIXED[key]!r}")
    lr, (beta1, beta2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
    for name, v in (("lr", lr), ("beta1", beta1), ("beta2", beta2), ("eps", eps), ("weight_decay", wd)):
        if isinstance(v, torch.Tensor):
            raise ValueError(f"AdamW (HIP): {name} must be a Python number (a tensor is torch's capturable path)")
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
        raise ValueError(f"Invalid beta parameters: {(beta1, beta2)}")
    if not 0.0 <= wd:
        raise ValueError(f"Invalid weight_decay value: {wd}")


def _check_param(p) -> None:
    if not p.is_cuda:
        raise TsodError("AdamW (HIP): parameters must live on a CUDA/ROCm device; there is no CPU fallback "
                        f"(got a {p.device} parameter of shape {tuple(p.shape)})")
    if p.dtype != torch.float32:
        raise TsodError(f"AdamW (HIP): float32 parameters only, got {p.dtype}")
    if p.layout != torch.strided or not p.is_contiguous():
        raise TsodError(f"AdamW (HIP): parameters must be dense and contiguous (shape {tuple(p.shape)}, strides {p.stride()})")


def _check_grad(p, g) -> None:
    if g.is_sparse or g.layout != torch.strided:
        raise TsodError("AdamW (HIP): sparse gradients are not supported")
    if g.device != p.device:
        raise TsodError(f"AdamW (HIP): gradient on {g.device}, its parameter on {p.device}")
    if g.dtype != torch.float32 or g.shape != p.shape or not g.is_contiguous():
        raise TsodError(f"AdamW (HIP): the gradient must be a contiguous float32 tensor of the parameter's shape "
                        f"{tuple(p.shape)}, got {g.dtype} {tuple(g.shape)} strides {g.stride()}")


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (amsgrad=False, maximize=False) with the update of all tensors of all groups in one launch.

    ``step(zero_grad=True)`` also clears the gradients in that pass and keeps the ``.grad`` tensors allocated;
    ``step(max_grad_norm=m)`` clips by global norm in it (see ``step``; the keyword lives on ``step`` only, ``param_groups``
    and ``state_dict()`` keep torch's key set) and leaves the norm in ``grad_norm``.  Parameters
    without a gradient are skipped and get no state.  Not implemented: amsgrad, maximize, capturable (graph capture of the
    step), tensor learning rates, more than one device per optimizer, more than 32 distinct (group, step count) pairs in
    one step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **_FIXED)
        self._layout = None            # (signature, device table, device chunks) of the last launch
        self._clip_buffers = None      # (norm workspace, result record) for that layout, made by the first clipped step
        self.grad_norm = None          # step(max_grad_norm=): the norm before clipping, a 0-d device tensor
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            _check_group(group)
            for p in group["params"]:
                _check_param(p)
        except Exception:
            self.param_groups.pop()
            raise

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._clip_buffers = None
        for group in self.param_groups:
            _check_group(group)
        for st in self.state.values():             # a fused torch.optim.AdamW keeps `step` on the device: bring it home once
            if "step" in st and (st["step"].device.type != "cpu" or st["step"].dtype != torch.float32):
                st["step"] = st["step"].to("cpu", torch.float32)
        self._layout = None

    def __setstate__(self, state):
        super().__setstate__(state)
        self._layout = None
        self._clip_buffers = None
        self.__dict__.setdefault("grad_norm", None)

    @torch.no_grad()
    def step(self, closure=None, *, zero_grad=False, max_grad_norm=None, error_if_nonfinite=False):
        """One update of every parameter that has a gradient, in one launch.

        ``zero_grad``: clear the gradients in the same pass (the ``.grad`` tensors stay allocated).
        ``max_grad_norm``: clip by global norm first, as ``torch.nn.utils.clip_grad_norm_(all parameters, max_grad_norm)``
        in front of the step would: the 2-norm over every gradient of every group (two launches, fixed summation order,
        bit-identical from run to run), then the step multiplies each gradient by min(1, max / (norm + 1e-6)) as it reads
        it - three launches in all, no device-to-host copy, no synchronisation.  Without ``zero_grad`` the ``.grad``
        tensors hold the clipped gradients afterwards.  ``self.grad_norm`` is then the norm before clipping: a 0-d float32
        device tensor that views the optimizer's result record, which the next clipped step overwrites (clone it to keep
        it); ``None`` when no parameter had a gradient.  A finite number >= 0, else ``ValueError``.
        ``error_if_nonfinite``: read the norm back once (this synchronises) and raise ``RuntimeError`` when it is NaN or
        infinite, before anything is stepped: parameters, state, step counters and gradients stay as they were.  With the
        default a non-finite norm flows into the parameters, as with torch."""
        if max_grad_norm is not None:
            max_grad_norm = _check_max_norm(max_grad_norm, "max_grad_norm")
        elif error_if_nonfinite:
            raise ValueError("AdamW (HIP): error_if_nonfinite needs max_grad_norm")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params, steps, group_of, sig, fresh = [], [], [], [], []
        for gi, group in enumerate(self.param_groups):
            _check_group(group)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise TsodError("AdamW (HIP): sparse gradients are not supported")
                st = self.state.get(p)
                if not st:
                    _check_param(p)
                    _check_grad(p, g)
                    st = self.state[p]
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    fresh.append(p)
                params.append(p)
                steps.append(st["step"])
                group_of.append(gi)
                sig.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()))
        if not params:
            if max_grad_norm is not None:
                self.grad_norm = None
            return loss
        counts = [t + 1 for t in torch.stack(steps).tolist()]      # host tensors: no device traffic
        slot_of, slots = {}, []
        for gi, t in zip(group_of, counts):
            slots.append(slot_of.setdefault((gi, t), len(slot_of)))
        if len(slot_of) > ADAMW_MAX_GROUPS:
            raise TsodError(f"AdamW (HIP): {len(slot_of)} distinct (param group, step count) pairs in one step, at most "
                            f"{ADAMW_MAX_GROUPS} fit one launch")
        scalars = [hip_ops.adamw_group(self.param_groups[gi]["lr"], *self.param_groups[gi]["betas"],
                                       self.param_groups[gi]["eps"], self.param_groups[gi]["weight_decay"], t)
                   for gi, t in slot_of]
        sig = (sig, slots)
        if self._layout is None or self._layout[0] != sig:
            device = params[0].device
            for p in params:
                _check_param(p)
                _check_grad(p, p.grad)
                if p.device != device:
                    raise TsodError(f"AdamW (HIP): parameters on {device} and {p.device}; one device per optimizer")
                state = self.state[p]
                for k in ("exp_avg", "exp_avg_sq"):
                    m = state[k]
                    if m.device != device or m.dtype != torch.float32 or m.shape != p.shape or not m.is_contiguous():
                        raise TsodError(f"AdamW (HIP): state {k} must be a contiguous float32 tensor like its parameter")
            with torch.cuda.device(device):
                table, chunks = _upload([s[:4] for s in sig[0]], [s[4] for s in sig[0]], slots, len(slot_of), device)
            self._layout = (sig, table, chunks)
            self._clip_buffers = None
        _, table, chunks = self._layout
        if max_grad_norm is None:
            torch._foreach_add_(steps, 1)
            with torch.cuda.device(table.device):
                hip_ops.adamw_step(table, chunks, scalars, zero_grad)
        else:
            if self._clip_buffers is None:         # cached with the layout: the norm's partials and the result record
                self._clip_buffers = _clip_buffers(chunks)
            workspace, record = self._clip_buffers
            with torch.cuda.device(table.device):
                hip_ops.grad_norm(table, chunks, max_grad_norm, record, workspace)
                self.grad_norm = hip_ops.grad_norm_fields(record)[1]
                if error_if_nonfinite and not math.isfinite(float(self.grad_norm)):      # the one read-back
                    for p in fresh:
                        del self.state[p]
                    raise RuntimeError(_NONFINITE)
                torch._foreach_add_(steps, 1)
                hip_ops.adamw_step_clipped(table, chunks, scalars, zero_grad, record)
        # the kernel wrote through raw pointers: tell autograd (and every cache keyed on Tensor._version) by hand
        torch.autograd.graph.increment_version(params)
        return loss


def _upload(pointers, numels, slots, n_slots, device):
    """Table and work list -> one pinned buffer -> the device, asynchronously on the current stream.  A fresh pinned
    buffer every time (torch's host allocator hands a block out again only after the copy that reads it has run)."""
    table = hip_ops.adamw_table(pointers, numels, slots, n_slots)
    chunks = hip_ops.adamw_chunks(numels)
    words = table.size
    host = torch.empty(words + len(chunks), dtype=torch.int64, pin_memory=True)
    view = host.numpy()
    view[:words] = table.reshape(-1)
    view[words:] = chunks.reshape(-1).view(np.int64)
    dev = host.to(device, non_blocking=True)
    return dev[:words].view(-1, 6), dev[words:].view(torch.int32).view(-1, 2)


def _clip_buffers(chunks):
    """(workspace, result record) of ``hip_ops.grad_norm`` for this work list."""
    workspace = torch.empty(max(hip_ops.grad_norm_workspace_bytes(chunks.shape[0]) // 8, 1), dtype=torch.float64,
                            device=chunks.device)
    return workspace, hip_ops.grad_norm_record(chunks.device)


def _check_max_norm(value, name) -> float:
    if not isinstance(value, numbers.Real) or isinstance(value, bool):
        raise ValueError(f"{name} must be a Python number (a tensor would have to be read back), got {type(value).__name__}")
    v = float(value)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0, got {value!r}")
    return v


_NONFINITE = ("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped. To "
              "disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
_clip_layout = None            # (signature, device table, device chunks, workspace) of the last clip_grad_norm_ call


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """``torch.nn.utils.clip_grad_norm_`` on HIP, for use in front of any optimizer: the 2-norm over the gradients of
    ``parameters`` (a tensor or an iterable of tensors; those without a gradient are skipped) in the fixed order of
    ``AdamW.step(max_grad_norm=)`` - the same bits - then every gradient times min(1, max_norm / (norm + 1e-6)), in place:
    three launches, nothing copied to the host.  Returns the norm before clipping as a 0-d float32 device tensor
    (``tensor(0.)`` when there is no gradient, as torch does).  Gradients must be float32, dense, contiguous and on one
    CUDA/ROCm device (``TsodError``; no CPU fallback); ``norm_type`` other than 2 and a ``max_norm`` that is not a finite
    number >= 0 raise ``ValueError``.  ``error_if_nonfinite`` reads the norm back once and raises ``RuntimeError`` before
    any gradient is touched."""
    global _clip_layout
    if not isinstance(norm_type, numbers.Real) or float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_ (HIP): only norm_type=2 is implemented, got {norm_type!r}")
    max_norm = _check_max_norm(max_norm, "max_norm")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    device = grads[0].device
    for g in grads:
        if g.is_sparse or g.layout != torch.strided:
            raise TsodError("clip_grad_norm_ (HIP): sparse gradients are not supported")
        if not g.is_cuda:
            raise TsodError("clip_grad_norm_ (HIP): gradients must live on a CUDA/ROCm device; there is no CPU fallback "
                            f"(got a {g.device} gradient of shape {tuple(g.shape)})")
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise TsodError(f"clip_grad_norm_ (HIP): gradients must be contiguous float32 tensors, got {g.dtype} "
                            f"{tuple(g.shape)} strides {g.stride()}")
        if g.device != device:
            raise TsodError(f"clip_grad_norm_ (HIP): gradients on {device} and {g.device}; one device per call")
    sig = (device, [(g.data_ptr(), g.numel()) for g in grads])
    with torch.cuda.device(device):
        if _clip_layout is None or _clip_layout[0] != sig:
            # only `grad` and `n` of a record are read: the gradient's pointer stands in for the other three
            table, chunks = _upload([(ptr,) * 4 for ptr, _ in sig[1]], [n for _, n in sig[1]], [0] * len(grads), 1, device)
            _clip_layout = (sig, table, chunks, _clip_buffers(chunks)[0])
        _, table, chunks, workspace = _clip_layout
        record = hip_ops.grad_norm_record(device)          # the caller's: a later call does not overwrite it
        hip_ops.grad_norm(table, chunks, max_norm, record, workspace)
        norm = hip_ops.grad_norm_fields(record)[1]
        if error_if_nonfinite and not math.isfinite(float(norm)):
            raise RuntimeError(_NONFINITE)
        hip_ops.grad_scale(table, chunks, record)
    torch.autograd.graph.increment_version(grads)
    return norm
