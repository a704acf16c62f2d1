#!/usr/bin/env python3
"""Generate tests/golden/ema_ref.npz by running the REFERENCE's own ``update_ema`` (utils/utils.py:13-16) through the loop of
its training script (train/train.py:147-153) on CPU.

Run in the build container only (needs the reference checkout; it is never shipped):

    python tests/golden/make_golden_ema.py

* The series: 1000 seeded f32 samples shaped like a training loss (a decaying level plus noise), held as the script holds
  them - a list of 0-d f32 CPU tensors, what ``total_loss.detach().cpu()`` appends (train/train.py:88).
* For alpha in (0.01, 0.3) the loop is the script's, verbatim: the first value as it is, then ``update_ema(train_loss[i],
  ema_alpha, ema_train_loss[i-1])``.

Stored (arrays only, no reference source): ``x`` f32 [1000], ``alphas`` f64 [2] and ``ema_0``, ``ema_1`` f32 [1000].
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TSOD_REFERENCE", "/root/reference")

spec = importlib.util.spec_from_file_location("reference_utils", os.path.join(REF, "utils", "utils.py"))
reference_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(reference_utils)
update_ema = reference_utils.update_ema

N, ALPHAS = 1000, (0.01, 0.3)


def main():
    gen = torch.Generator().manual_seed(20240428)
    steps = torch.arange(N, dtype=torch.float32)
    x = 2.5 * torch.exp(-steps / 300.0) + 0.4 + 0.3 * torch.randn(N, generator=gen)
    train_loss = [v.detach().cpu() for v in x]                       # 0-d f32 tensors, as train/train.py:88 appends them
    out = dict(x=x.numpy().astype(np.float32), alphas=np.array(ALPHAS, dtype=np.float64))
    for k, ema_alpha in enumerate(ALPHAS):
        ema_train_loss = []
        for i in range(len(train_loss)):
            if i == 0:
                ema_train_loss.append(train_loss[0])
            else:
                ema_train_loss.append(update_ema(train_loss[i], ema_alpha, ema_train_loss[i - 1]))
        assert all(v.dtype == torch.float32 for v in ema_train_loss)
        out[f"ema_{k}"] = torch.stack(ema_train_loss).numpy()
    path = os.path.join(HERE, "ema_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
