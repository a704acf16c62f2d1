"""The detection overlay (include/tsod.h "detection overlay") restated in NumPy as a painter's algorithm:
item by item over whole arrays with masks - the structural opposite of the kernel's per-pixel walk over a culled list.  Integers
only beyond the one f32 multiply per coordinate and the score's rounding.  It carries no glyph table: ``font`` is passed in
(``tsod_draw_font5x7``'s [128,7] array), the glyph shapes are data with one copy.

``draw(img, groups, strings, font)`` paints ``img`` (u8 [B,H,W,3], possibly a view into a pitched buffer) in place.  A group is a
dict with the keys of ``hip_ops.draw_groups`` holding NumPy arrays: boxes [B,R,4|6], counts, keep, n_kept, labels, label_offset,
strings = (first, count), scale = (sx, sy), color, alpha, width, tag, text_color, tag_bg, tag_alpha, font_scale, padding,
score_line.  ``strings``: u8 [n,32] or None."""
import numpy as np

F32 = np.float32
LIMIT = F32(2.0 ** 24)


def to_pixel(s, v):
    v = F32(v)
    if not np.isfinite(v):
        return None
    with np.errstate(all="ignore"):
        p = F32(s) * v
    if np.isnan(p):
        return None
    return int(np.rint(min(max(p, -LIMIT), LIMIT)))


def rows_drawn(g, b):
    R = g["boxes"].shape[1]
    clamp = lambda n: min(max(int(n), 0), R)
    if g.get("keep") is not None:
        return [int(k) for k in g["keep"][b, :clamp(g["n_kept"][b])]]
    if g.get("counts") is not None:
        return list(range(clamp(g["counts"][b])))
    return list(range(R))


def box_pixels(g, b, r):
    """(X1, Y1, X2, Y2) inclusive, or None when the row draws nothing."""
    if not 0 <= r < g["boxes"].shape[1]:
        return None
    sx, sy = g.get("scale", (1.0, 1.0))
    x1, y1, x2, y2 = g["boxes"][b, r, :4]
    px = [to_pixel(sx, x1), to_pixel(sy, y1), to_pixel(sx, x2), to_pixel(sy, y2)]
    if any(p is None for p in px) or px[2] < px[0] or px[3] < px[1]:
        return None
    return tuple(px)


def blend(region, mask, rgb, a):
    """region u8 [h,w,3] (a view), mask bool [h,w]: out = (a c + (255 - a) src + 127) / 255 where the mask is set."""
    if a == 0 or not mask.any():
        return
    src = region.astype(np.int64)
    out = (a * np.asarray(rgb, dtype=np.int64)[None, None, :] + (255 - a) * src + 127) // 255
    region[mask] = out[mask].astype(np.uint8)


def label_index(g, b, r):
    """The row's label index, or None when it has no label."""
    if g.get("labels") is not None:
        idx = int(g["labels"][b, r])
    elif g["boxes"].shape[2] == 6:
        c = F32(g["boxes"][b, r, 5])
        if np.isnan(c):
            idx = 0
        elif c >= F32(2.0 ** 31):
            idx = 2 ** 31 - 1
        elif c <= F32(-2.0 ** 31):
            idx = -2 ** 31
        else:
            idx = int(np.trunc(c))
    else:
        return None
    return idx + int(g.get("label_offset", 0))


def tag_lines(g, b, r, strings):
    idx = label_index(g, b, r)
    if idx is None:
        return None
    first, count = g.get("strings", (0, 0 if strings is None else len(strings)))
    if 0 <= idx < count:
        row = bytes(strings[first + idx])[:31]
        line1 = row.split(b"\0")[0]
    else:
        line1 = f"class_{idx}".encode()
    lines = [line1]
    if g.get("score_line"):
        s = F32(g["boxes"][b, r, 4])
        if np.isnan(s):
            lines.append(b"Conf: -.---")
        else:
            m = int(np.rint(F32(min(max(s, F32(0)), F32(1))) * F32(1000)))
            lines.append(f"Conf: {m // 1000}.{m % 1000:03d}".encode())
    return lines


def text_bitmap(lines, font, s, pad):
    """bool [h,w]: the tag's glyph pixels."""
    cols = max(len(l) for l in lines)
    w, h = cols * 6 * s + 2 * pad, len(lines) * 8 * s + 2 * pad
    ink = np.zeros((h, w), dtype=bool)
    for l, line in enumerate(lines):
        for k, ch in enumerate(line):
            rows = font[ch] if ch < 128 else np.full(7, 0x1f, dtype=np.uint8)
            glyph = ((rows[:, None].astype(np.int64) >> (4 - np.arange(5))[None, :]) & 1).astype(bool)     # [7,5]
            big = np.kron(glyph, np.ones((s, s), dtype=bool))
            y, x = pad + 8 * l * s, pad + 6 * k * s
            ink[y:y + 7 * s, x:x + 5 * s] |= big
    return ink


def paint_outline(img, g, box):
    H, W = img.shape[:2]
    X1, Y1, X2, Y2 = box
    t = int(g.get("width", 1))
    xa, xb, ya, yb = max(X1, 0), min(X2, W - 1), max(Y1, 0), min(Y2, H - 1)
    if xa > xb or ya > yb:
        return
    x, y = np.arange(xa, xb + 1)[None, :], np.arange(ya, yb + 1)[:, None]
    mask = (x - X1 < t) | (X2 - x < t) | (y - Y1 < t) | (Y2 - y < t)
    blend(img[ya:yb + 1, xa:xb + 1], mask, g.get("color", (255, 0, 0)), int(g.get("alpha", 255)))


def paint_tag(img, g, box, lines, font):
    H, W = img.shape[:2]
    X1, Y1, X2, Y2 = box
    s, pad = int(g.get("font_scale", 1)), int(g.get("padding", 0))
    ink = text_bitmap(lines, font, s, pad)
    h, w = ink.shape
    left = X1
    if g["tag"] == "above":
        top = Y1 - h
        if top < 0:
            top = Y1
    else:
        top = Y2 + 1
        if top + h > H:
            top = Y2 - h + 1
    if left > 0 and left + w > W:
        left = max(W - w, 0)
    xa, xb, ya, yb = max(left, 0), min(left + w, W), max(top, 0), min(top + h, H)                 # clipped, exclusive ends
    if xa >= xb or ya >= yb:
        return
    region = img[ya:yb, xa:xb]
    blend(region, np.ones(region.shape[:2], dtype=bool), g.get("tag_bg", (255, 255, 255)), int(g.get("tag_alpha", 255)))
    region[ink[ya - top:yb - top, xa - left:xb - left]] = np.asarray(g.get("text_color", g.get("color", (255, 0, 0))), dtype=np.uint8)


def draw(img, groups, strings, font):
    B = img.shape[0]
    for b in range(B):
        items = [(g, r, box_pixels(g, b, r)) for g in groups for r in rows_drawn(g, b)]
        items = [it for it in items if it[2] is not None]
        for g, r, box in items:                                   # first every outline ...
            paint_outline(img[b], g, box)
        for g, r, box in items:                                   # ... then every tag, in the same order
            if g.get("tag", "none") in (None, "none"):
                continue
            lines = tag_lines(g, b, r, strings)
            if lines is not None:
                paint_tag(img[b], g, box, lines, font)
    return img
