"""The loss bookkeeping of the reference's training script on the device.

The reference appends ``total_loss.detach().cpu()`` every step (train/train.py:88: a device-to-host copy and a wait per
micro-batch) and smooths the list at the end with ``update_ema`` in a Python loop (train/train.py:147-160).  Here the log
lives on the device and the loop is one launch:

* ``update_ema``   the reference's function, for host or device scalars;
* ``ema_curve``    the whole loop of train.py:147-153 over a series, ``hip_ops.ema_scan``;
* ``TrainingLog``  a growable f32 device buffer that ``append`` fills with stream-ordered device copies.

Nothing here reads device memory on the host; lengths are host integers.
"""
from __future__ import annotations

import torch

from .. import hip_ops


def update_ema(current_value, ema_alpha, last_ema=None):
    """utils/utils.py:13-16 of the reference: the first value as it is, then ``alpha current + (1 - alpha) last``."""
    if last_ema is None:
        return current_value
    return ema_alpha * current_value + (1 - ema_alpha) * last_ema


class TrainingLog:
    """A device-resident list of f32 scalars: ``append`` costs one small device copy on the current stream and no host read,
    so a training loop can keep its loss curve without the reference's ``.cpu()`` per step."""

    def __init__(self, device, capacity=4096):
        if int(capacity) < 1:
            raise ValueError(f"TrainingLog: capacity must be at least 1, got {capacity}")
        self._buf = torch.empty(int(capacity), dtype=torch.float32, device=device)
        self._n = 0

    def __len__(self):
        return self._n

    @property
    def device(self):
        return self._buf.device

    @property
    def capacity(self):
        return self._buf.numel()

    @property
    def values(self) -> torch.Tensor:
        """The samples so far, an f32 [n] view of the buffer (valid until the next growth)."""
        return self._buf[:self._n]

    def append(self, loss) -> None:
        """``loss``: a 0-d (or one-element) device tensor, copied on the current stream, or a Python number."""
        if self._n == self._buf.numel():                 # grow by doubling; the old samples move with a device copy
            grown = torch.empty(2 * self._buf.numel(), dtype=torch.float32, device=self._buf.device)
            grown[:self._n].copy_(self._buf)
            self._buf = grown
        slot = self._buf[self._n:self._n + 1]
        if isinstance(loss, torch.Tensor):
            if loss.numel() != 1:
                raise ValueError(f"TrainingLog.append: a scalar, got a tensor of shape {tuple(loss.shape)}")
            slot.copy_(loss.detach().reshape(1), non_blocking=True)
        else:
            slot.fill_(float(loss))
        self._n += 1

    def ema(self, alpha=0.01) -> torch.Tensor:
        return ema_curve(self, alpha)


def as_series(values, device=None):
    """What every curve argument accepts -> a contiguous f32 [n] device tensor (None for an empty list): a ``TrainingLog``, a
    1-D device tensor, or a list of Python numbers (uploaded once, through pinned memory, without waiting) or of 0-d device
    tensors (stacked on the device)."""
    device = torch.device("cuda") if device is None else device           # (host data goes to the current device)
    if isinstance(values, TrainingLog):
        return values.values
    if isinstance(values, torch.Tensor):
        if values.dim() != 1:
            raise ValueError(f"a series is 1-D, got a tensor of shape {tuple(values.shape)}")
        if not values.is_cuda:
            return values.to(torch.float32).contiguous().pin_memory().to(device, non_blocking=True)
        return values.to(torch.float32).contiguous()
    values = list(values)
    if not values:
        return None
    if all(isinstance(v, torch.Tensor) and v.is_cuda for v in values):
        return torch.stack([v.detach().reshape(()) for v in values]).to(torch.float32)
    host = torch.tensor([float(v) for v in values], dtype=torch.float32)
    return host.pin_memory().to(device, non_blocking=True)


def ema_curve(values, alpha=0.01, device=None) -> torch.Tensor:
    """The loop of train/train.py:147-153 in one launch: ``out[0] = v[0]``, ``out[i] = update_ema(v[i], alpha, out[i-1])`` in
    f32, bit for bit -> f32 [n] on the device.  ``values``: see ``as_series``."""
    x = as_series(values, device)
    if x is None:
        return torch.empty(0, dtype=torch.float32, device="cuda" if device is None else device)
    return hip_ops.ema_scan(x, alpha)
