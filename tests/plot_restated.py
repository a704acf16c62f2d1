"""NumPy restatement of the training-curve kernels from the text of include/tsod.h ("training
curves"): integer arithmetic where the header says integer (Python ints), np.float32 operations - one rounding each - where it
says f32.  Shared by the CPU and GPU tests; nothing here imports the package."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
MARKERS = {None: 0, "none": 0, "o": 1, "s": 2, "^": 3}


# --------------------------------------------------------------------------------------------------------------------- K1
def ema_constants(alpha):
    return F(alpha), F(1.0 - float(alpha))


def ema(x, alpha):
    """x f32 [n] or [rows, n] -> the same shape: out[0] = x[0], out[i] = fadd(fmul(a, x[i]), fmul(b, out[i-1]))."""
    a, b = ema_constants(alpha)
    x = np.asarray(x, dtype=F)
    rows = x.reshape(-1, x.shape[-1])
    out = np.empty_like(rows)
    with np.errstate(all="ignore"):
        for r in range(rows.shape[0]):
            p = a * rows[r]                                          # f32 products, one rounding each
            prev = F(0)
            for i in range(rows.shape[1]):
                prev = rows[r, i] if i == 0 else F(p[i] + F(b * prev))
                out[r, i] = prev
    return out.reshape(x.shape)


# --------------------------------------------------------------------------------------------------------------------- K2
def limits(series):
    vals = [np.asarray(s, dtype=F).ravel() for s in series]
    vals = np.concatenate(vals) if vals else np.zeros(0, dtype=F)
    vals = vals[np.isfinite(vals)]
    with np.errstate(all="ignore"):
        if vals.size == 0:
            lo, hi = F(0), F(1)
        else:
            m, M = vals.min(), vals.max()
            if M == m:
                lo, hi = F(m - F(0.5)), F(m + F(0.5))
            else:
                half = F(F(F(0.5) * M) - F(F(0.5) * m))
                pad = F(F(0.1) * half)
                lo, hi = F(m - pad), F(M + pad)
        clamp = lambda v: np.fmin(np.fmax(v, -FLT_MAX), FLT_MAX)
        return np.array([clamp(lo), clamp(hi)], dtype=F)


# --------------------------------------------------------------------------------------------------------------------- K3
def columns(n, x_first, x_step, x_lo, x_hi, px0, pw):
    """c_i for i = 0 .. n-1, in Python integers."""
    if x_hi == x_lo:
        return [px0] * n
    return [px0 + ((x_first + i * x_step - x_lo) * (pw - 1)) // (x_hi - x_lo) for i in range(n)]


def rows_of(y, lim, py0, ph):
    """r_i (int64 array; meaningless where y is not finite)."""
    y = np.asarray(y, dtype=F)
    lo, hi = F(lim[0]), F(lim[1])
    with np.errstate(all="ignore"):
        s = F(F(ph - 1) / F(hi - lo))
        t = (y - lo).astype(F) * s
        t = np.fmin(np.fmax(t.astype(F), F(0)), F(ph - 1))
        t = np.where(np.isfinite(y), t, F(0))
        return py0 + (ph - 1) - np.rint(t).astype(np.int64)


def segment_rows(c0, r0, c1, r1, c):
    """The (first, last) rows the segment paints in column c, c0 <= c <= c1."""
    if c0 == c1:
        return min(r0, r1), max(r0, r1)
    dx, dy = c1 - c0, r1 - r0
    B = lambda cc: r0 + ((2 * (cc - c0) - 1) * dy + dx) // (2 * dx)          # Python's // is floor division
    a = r0 if c == c0 else B(c)
    b = r1 if c == c1 else B(c + 1)
    return min(a, b), max(a, b)


def marker_pixels(marker, size):
    """The (u, v) offsets of a marker bitmap."""
    k = size // 2
    out = []
    for u in range(-k, k + 1):
        for v in range(-k, k + 1):
            if marker == 2 or (marker == 1 and u * u + v * v <= k * k + k) or (marker == 3 and 2 * abs(u) <= v + k):
                out.append((u, v))
    return out


def series_coverage(s, rect, x_range, lim):
    """The boolean [ph, pw] coverage of one series inside the rectangle."""
    px0, py0, pw, ph = rect
    y = np.asarray(s["y"], dtype=F)
    n = len(y)
    cov = np.zeros((ph, pw), dtype=bool)
    cs = columns(n, s.get("x_first", 0), s.get("x_step", 1), x_range[0], x_range[1], px0, pw)
    rs = rows_of(y, lim, py0, ph).tolist()
    fin = np.isfinite(y).tolist()
    w = s.get("width", 1)
    a = w // 2
    marker = MARKERS[s.get("marker")]
    offsets = marker_pixels(marker, s.get("marker_size", 1)) if marker else []

    def line(c, ra, rb):                                             # skeleton rows ra..rb of column c, dilated to w x w
        x0, x1 = max(c - a, px0), min(c - a + w - 1, px0 + pw - 1)
        y0, y1 = max(ra - a, py0), min(rb - a + w - 1, py0 + ph - 1)
        if x0 <= x1 and y0 <= y1:
            cov[y0 - py0:y1 - py0 + 1, x0 - px0:x1 - px0 + 1] = True

    for i in range(n):
        if not fin[i]:
            continue
        if w >= 1:
            line(cs[i], rs[i], rs[i])
        for u, v in offsets:
            x, yy = cs[i] + u, rs[i] + v
            if px0 <= x < px0 + pw and py0 <= yy < py0 + ph:
                cov[yy - py0, x - px0] = True
        if w >= 1 and i + 1 < n and fin[i + 1]:
            for c in range(cs[i], cs[i + 1] + 1):
                line(c, *segment_rows(cs[i], rs[i], cs[i + 1], rs[i + 1], c))
    return cov


def blend(img, mask, color, alpha):
    """img u8 [..., 3] blended in place where mask: out = (a c + (255 - a) src + 127) // 255."""
    a = int(alpha)
    for ch in range(3):
        plane = img[..., ch]
        src = plane[mask].astype(np.int64)
        plane[mask] = ((a * int(color[ch]) + (255 - a) * src + 127) // 255).astype(np.uint8)


def plot_series(img, rect, series, x_range, lim):
    """img u8 [H, W, 3] (a view is fine), painted in place -> the number of pixels covered by at least one series."""
    px0, py0, pw, ph = rect
    view = img[py0:py0 + ph, px0:px0 + pw]
    covered = np.zeros((ph, pw), dtype=bool)
    for s in series:
        if len(s["y"]) == 0 or s.get("alpha", 255) == 0:
            continue
        cov = series_coverage(s, rect, x_range, lim)
        blend(view, cov, s.get("color", (0, 0, 0)), s.get("alpha", 255))
        covered |= cov
    return int(covered.sum())


# --------------------------------------------------------------------------------------------------------------------- K4
def format_number(lim, tick, ticks):
    lo, hi = F(lim[0]), F(lim[1])
    with np.errstate(all="ignore"):
        d = F(hi - lo)
        t = F(F(tick) * d)
        q = F(t / F(ticks))
        v = F(lo + q)
        p = F(np.abs(v) * F(1000))
    if not (p < F(1e9)):
        return b"-.---"
    m = int(np.rint(p))
    return (b"-" if v < 0 and m > 0 else b"") + b"%d.%03d" % (m // 1000, m % 1000)


def plot_items(img, items, font, limits_of=None):
    """img u8 [H, W, 3] painted in place.  ``items``: the dicts of hip_ops.pack_plot_items; a number item's limits come from
    ``limits_of(item)`` (default: ``item["limits"]`` as a host pair)."""
    H, W, _ = img.shape
    align = {"left": 0, "right": 1, "center": 2}
    for it in items:
        color, alpha = it.get("color", (0, 0, 0)), it.get("alpha", 255)
        if alpha == 0:
            continue
        mask = np.zeros((H, W), dtype=bool)
        if it["kind"] == "rect":
            if it["w"] < 1 or it["h"] < 1:
                continue
            period, on = it.get("dash", (0, 0))
            for y in range(max(it["y"], 0), min(it["y"] + it["h"], H)):
                if period <= 0 or (y - it["y"]) % period < on:
                    mask[y, max(it["x"], 0):max(min(it["x"] + it["w"], W), 0)] = True
        else:
            s = it.get("scale", 1)
            if s < 1:
                continue
            text = it["text"] if it["kind"] == "text" else format_number(limits_of(it) if limits_of else it["limits"], it["tick"], it["ticks"])
            text = text.encode("utf-8") if isinstance(text, str) else bytes(text)
            width = 6 * s * len(text)
            left = it["x"] - (width if align[it.get("align", "left")] == 1 else width // 2 if align[it.get("align", "left")] == 2 else 0)
            for k, ch in enumerate(text):
                for gy in range(7):
                    bits = int(font[ch][gy]) if ch < 128 else 0x1f
                    for gx in range(5):
                        if (bits >> (4 - gx)) & 1:
                            x0, y0 = left + (6 * k + gx) * s, it["y"] + gy * s
                            mask[max(y0, 0):max(min(y0 + s, H), 0), max(x0, 0):max(min(x0 + s, W), 0)] = True
        blend(img, mask, color, alpha)


# ------------------------------------------------------------------------------------------------------------- the figure
def figure(plan, data, font):
    """The figure of utils.draw.plot_training_metrics composed the same way from ``utils.draw.figure_plan``'s plan and the
    host copies ``data`` of the series (by argument name) -> u8 [H, W, 3]."""
    img = np.zeros((plan["H"], plan["W"], 3), dtype=np.uint8)
    lims = [np.array(p["fixed_limits"], dtype=F) if p["fixed_limits"] is not None else limits([data[s["key"]] for s in p["series"]])
            for p in plan["panels"]]
    plot_items(img, plan["background"], font, lambda it: lims[it["panel"]])
    for p, lim in zip(plan["panels"], lims):
        if p["series"]:
            plot_series(img, p["rect"], [dict(s, y=data[s["key"]]) for s in p["series"]], p["x_range"], lim)
    plot_items(img, plan["legends"], font)
    return img
