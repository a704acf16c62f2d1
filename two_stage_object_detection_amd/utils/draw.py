"""The reference's training figure on the GPU: ``utils/draw.py:plot_training_metrics`` - three stacked
panels, training loss with its EMA, evaluation loss with its EMA, the three mAP curves - rendered from device-resident series
into a u8 device image by ``hip_ops.plot_items`` / ``plot_limits`` / ``plot_series``, and ``save_png`` for that image and the
overlay's.  Nothing is read back: lengths are host integers, axis limits and y-tick labels are made on the device.

The figure is defined by this project's own rules (the pixel rules in include/tsod.h, the layout in ``figure_plan``), not by
matplotlib's rasteriser: a 5x7 bitmap font, unrotated labels, lines without anti-aliasing.  The font has no '@', so the mAP
legend reads ``mAP 0.5`` for the reference's ``mAP@0.5``.
"""
from __future__ import annotations

import struct
import zlib

import torch

from .. import hip_ops
from .utils import as_series

SUPTITLE = "Training and Evaluation Metrics"
TITLES = ("Training Loss", "Evaluation Loss", "Evaluation mAP")
YLABELS = ("Loss", "Loss", "mAP")
XLABEL = "Epoch"
# (argument, legend label, colour, alpha, width, marker, marker size) per panel, in the reference's drawing order
SERIES = (
    (("train_loss", "Train Loss", (0x1f, 0x77, 0xb4), 128, 1, None, 1),
     ("ema_train_loss", "EMA Train Loss", (0xff, 0x7f, 0x0e), 255, 1, None, 1)),
    (("eval_loss", "Eval Loss", (0x2c, 0xa0, 0x2c), 179, 1, "o", 5),
     ("ema_eval_loss", "EMA Eval Loss", (0xd6, 0x27, 0x28), 255, 1, "s", 5)),
    (("mAP50_list", "mAP 0.5", (0x94, 0x67, 0xbd), 204, 1, "o", 5),
     ("mAP50_95_list", "mAP 0.5:0.95", (0x8c, 0x56, 0x4b), 204, 1, "s", 5),
     ("mAP95_list", "mAP 0.95", (0xe3, 0x77, 0xc2), 204, 1, "^", 5)),
)
Y_TICKS = 5
GRID_ALPHA, SEPARATOR_ALPHA, LEGEND_ALPHA = 77, 128, 204             # 0.3, 0.5 and 0.8 of 255
GRAY = (128, 128, 128)
EVAL_EVERY = 10                                                      # the reference evaluates every 10th epoch
MIN_SIZE = (244, 200)                                                # (H, W): the smallest figure the layout fits into


def _unit(H, W):
    """The layout's length unit in pixels: 2 at the default size, 1 for small figures."""
    return 2 if H >= 1100 and W >= 900 else 1


def figure_plan(epoch_num, total_steps, lengths, size=(1500, 1200)):
    """HOST, integers only: the figure's layout -> ``dict(H, W, background, panels, legends)``.

    ``lengths``: the sample count of each of the seven series by argument name.  ``background`` and ``legends`` are item
    lists for ``hip_ops.plot_items`` (a "number" item names its ``panel`` instead of a limits tensor); a panel is ``dict(rect,
    x_range, fixed_limits, series)`` with the series' styles and abscissae for ``hip_ops.plot_series``.  Painting order:
    background items, each panel's series, legend items."""
    H, W = (int(v) for v in size)
    if H < MIN_SIZE[0] or W < MIN_SIZE[1]:
        raise ValueError(f"plot_training_metrics: size (H, W) = {(H, W)} is too small for the layout, the minimum is {MIN_SIZE}")
    epoch_num, total_steps = int(epoch_num), int(total_steps)
    if epoch_num < 1 or total_steps < 0:
        raise ValueError(f"plot_training_metrics: epoch_num >= 1 and step_num >= 0, got {epoch_num} and {total_steps}")
    t = _unit(H, W)
    sup = 2 * t if len(SUPTITLE) * 12 * t <= W else t
    header = 8 * sup + 6 * t
    band = (H - header) // 3
    left, right = 72 * t, 8 * t
    items = [dict(kind="rect", x=0, y=0, w=W, h=H, color=(255, 255, 255)),
             dict(kind="text", x=W // 2, y=3 * t, text=SUPTITLE, scale=sup, align="center")]
    legends, panels = [], []
    for p in range(3):
        top = header + p * band
        px0, py0, pw, ph = left, top + 12 * t, W - left - right, band - 34 * t
        n = max([lengths.get(s[0], 0) for s in SERIES[p]] + ([total_steps] if p == 0 else []))
        if p == 0:
            x_lo, x_hi, first, step = 0, max(n - 1, 0), 0, 1
            per_epoch = total_steps // epoch_num
            ticks = [(i * per_epoch, str(i)) for i in range(epoch_num + 1) if i * per_epoch < total_steps and (per_epoch or i == 0)]
        else:
            x_lo, x_hi, first, step = 0, EVAL_EVERY * max(n, 1), 1, EVAL_EVERY
            ticks = [(EVAL_EVERY * i + 1, str(EVAL_EVERY * i + 1)) for i in range(n)]
        column = lambda x: px0 + ((x - x_lo) * (pw - 1) // (x_hi - x_lo) if x_hi > x_lo else 0)
        items.append(dict(kind="text", x=px0 + pw // 2, y=top + 2 * t, text=TITLES[p], scale=t, align="center"))
        items.append(dict(kind="text", x=2 * t, y=top + 2 * t, text=YLABELS[p], scale=t))
        items.append(dict(kind="text", x=px0 + pw // 2, y=py0 + ph + 13 * t, text=XLABEL, scale=t, align="center"))
        for k in range(Y_TICKS + 1):                                 # horizontal grid lines and their device-made labels
            r = py0 + (ph - 1) - (2 * k * (ph - 1) + Y_TICKS) // (2 * Y_TICKS)
            items.append(dict(kind="rect", x=px0, y=r, w=pw, h=1, alpha=GRID_ALPHA))
            items.append(dict(kind="number", x=px0 - 3 * t, y=r - 3 * t, panel=p, tick=k, ticks=Y_TICKS, scale=t, align="right"))
        label_end = -1
        for i, (x, label) in enumerate(ticks):                       # vertical grid lines, epoch separators, x-tick labels
            c = column(x)
            items.append(dict(kind="rect", x=c, y=py0, w=1, h=ph, alpha=GRID_ALPHA))
            if p == 0 and i > 0:
                items.append(dict(kind="rect", x=c, y=py0, w=t, h=ph, color=GRAY, alpha=SEPARATOR_ALPHA, dash=(6 * t, 4 * t)))
            half = len(label) * 3 * t
            if c - half > label_end:                                 # a label that would run into the one before it is left out
                items.append(dict(kind="text", x=c, y=py0 + ph + 3 * t, text=label, scale=t, align="center"))
                label_end = c + half + 2 * t
        for x, y, w, h in ((px0 - 1, py0 - 1, pw + 2, 1), (px0 - 1, py0 + ph, pw + 2, 1), (px0 - 1, py0, 1, ph), (px0 + pw, py0, 1, ph)):
            items.append(dict(kind="rect", x=x, y=y, w=w, h=h))
        series = [dict(key=key, x_first=first, x_step=step, color=color, alpha=alpha, width=width, marker=marker,
                       marker_size=size_, label=label)
                  for key, label, color, alpha, width, marker, size_ in SERIES[p] if lengths.get(key, 0) > 0]
        panels.append(dict(rect=(px0, py0, pw, ph), x_range=(x_lo, x_hi), fixed_limits=(0.0, 1.0) if p == 2 else None, series=series))
        if series:                                                   # the legend: upper right corner, over the curves
            lw = (max(len(s["label"]) for s in series) * 6 + 20) * t
            lh = (len(series) * 9 + 3) * t
            lx, ly = px0 + pw - lw - 3 * t, py0 + 3 * t
            legends.append(dict(kind="rect", x=lx, y=ly, w=lw, h=lh, color=(255, 255, 255), alpha=LEGEND_ALPHA))
            for x, y, w, h in ((lx, ly, lw, 1), (lx, ly + lh - 1, lw, 1), (lx, ly, 1, lh), (lx + lw - 1, ly, 1, lh)):
                legends.append(dict(kind="rect", x=x, y=y, w=w, h=h, color=GRAY))
            for j, s in enumerate(series):
                y = ly + (2 + 9 * j) * t
                legends.append(dict(kind="rect", x=lx + 3 * t, y=y + 2 * t, w=12 * t, h=3 * t, color=s["color"], alpha=s["alpha"]))
                legends.append(dict(kind="text", x=lx + 18 * t, y=y, text=s["label"], scale=t))
    return dict(H=H, W=W, background=items, panels=panels, legends=legends)


def _total_steps(step_num):
    """``step_num``: the step count, or the reference's ``list(range(n))`` (train/train.py:162) - any other list is refused."""
    if isinstance(step_num, int):
        return step_num
    steps = list(step_num)
    if steps != list(range(len(steps))):
        raise ValueError("plot_training_metrics: step_num is an int or list(range(n)); the abscissa of sample i is i")
    return len(steps)


def plot_training_metrics(epoch_num, step_num, train_loss, ema_train_loss, eval_loss, ema_eval_loss, mAP50_list, mAP50_95_list,
                          mAP95_list, *, size=(1500, 1200), out=None, path=None, device=None):
    """The reference's ``plot_training_metrics`` figure as a u8 device image [H, W, 3] (``size`` = (H, W); the reference's
    figure is 12 x 15 inches, portrait).

    The positional arguments are the reference's.  Every series is a ``TrainingLog``, a 1-D f32 device tensor, or a list of
    Python numbers or 0-d device tensors (``utils.as_series``); empty evaluation lists leave their panels with frame, grid
    and text only.  ``step_num``: an int or ``list(range(n))``.  ``out``: a u8 [H, W, 3] device image painted in place (its
    size is the figure's); ``path``: also written there with ``save_png``.  No device-to-host copy and no host wait, except
    ``save_png``'s."""
    total = _total_steps(step_num)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 3 or out.shape[2] != 3:
            raise ValueError("plot_training_metrics: out is a u8 [H, W, 3] device image")
        size, device = (out.shape[0], out.shape[1]), out.device
    names = [key for panel in SERIES for key, *_ in panel]
    given = dict(zip(names, (train_loss, ema_train_loss, eval_loss, ema_eval_loss, mAP50_list, mAP50_95_list, mAP95_list)))
    if device is None:
        device = next((v.device for v in given.values() if hasattr(v, "device")), torch.device("cuda"))
    plan = figure_plan(epoch_num, total, {k: len(v) for k, v in given.items()}, size)
    data = {k: as_series(v, device) for k, v in given.items()}
    image = out if out is not None else torch.empty((plan["H"], plan["W"], 3), dtype=torch.uint8, device=device)
    limits = torch.arange(2, dtype=torch.float32, device=device).repeat(3, 1)          # (0, 1) per panel, made on the device
    for p, panel in enumerate(plan["panels"]):
        if panel["fixed_limits"] is None:
            hip_ops.plot_limits([data[s["key"]] for s in panel["series"]], out=limits[p])
    with_limits = lambda items: [dict(it, limits=limits[it["panel"]]) if it["kind"] == "number" else it for it in items]
    hip_ops.plot_items(image, with_limits(plan["background"]))
    for p, panel in enumerate(plan["panels"]):
        if panel["series"]:
            hip_ops.plot_series(image, panel["rect"], [dict(s, y=data[s["key"]]) for s in panel["series"]], panel["x_range"], limits[p])
    if plan["legends"]:
        hip_ops.plot_items(image, plan["legends"])
    if path is not None:
        save_png(image, path)
    return image


def _chunk(tag, payload):
    return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload) & 0xffffffff)


def save_png(image_u8, path):
    """Write a u8 [H, W, 3] image (device or host, rows may be pitched) as an 8-bit RGB PNG: one device-to-host copy, then the
    standard library only - filter type 0 on every row, one IDAT chunk."""
    if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3:
        raise ValueError("save_png: the image is a u8 [H, W, 3] tensor")
    H, W, _ = image_u8.shape
    if H < 1 or W < 1:
        raise ValueError(f"save_png: an image has at least one pixel, got {H} x {W}")
    rows = image_u8.contiguous().cpu().numpy().reshape(H, 3 * W)
    raw = b"".join(b"\0" + rows[r].tobytes() for r in range(H))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b""))
