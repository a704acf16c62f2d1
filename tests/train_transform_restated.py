"""The reference's training transform (dataset/transform.py:4-12) restated in float32 torch on the CPU, rule by rule as
DESIGN 4.15 writes torchvision v2's public behaviour down.  torchvision is not importable here, so this restatement is
the oracle the HIP kernels are checked against; its rules are pinned by the hand-derived cases of
tests/test_train_transform.py.  Resizes use torch's antialiased bilinear interpolate, the oracle of test_input_step.py."""
import torch
import torch.nn.functional as F

GRAY = (0.2989, 0.587, 0.114)


def draw_sequence(H, W, generator, size=(600, 600), scale_range=(0.8, 1.2), p=0.5, flip_p=0.5):
    """The torch calls of RandomPhotometricDistort, RandomHorizontalFlip and ScaleJitter, one after another."""
    g = generator
    b = torch.empty(1).uniform_(0.875, 1.125, generator=g).item() if torch.rand(1, generator=g) < p else None
    c = torch.empty(1).uniform_(0.5, 1.5, generator=g).item() if torch.rand(1, generator=g) < p else None
    s = torch.empty(1).uniform_(0.5, 1.5, generator=g).item() if torch.rand(1, generator=g) < p else None
    h = torch.empty(1).uniform_(-0.05, 0.05, generator=g).item() if torch.rand(1, generator=g) < p else None
    contrast_before = bool(torch.rand((), generator=g) < 0.5)
    perm = tuple(torch.randperm(3, generator=g).tolist()) if torch.rand(1, generator=g) < p else None
    flip = bool(torch.rand(1, generator=g) < flip_p)
    scale = scale_range[0] + torch.rand(1, generator=g) * (scale_range[1] - scale_range[0])
    r = min(size[1] / H, size[0] / W) * scale
    return dict(brightness=b, contrast=c, saturation=s, hue=h, contrast_before=contrast_before, perm=perm, flip=flip,
                size=(int(H * r), int(W * r)))


def gray(x):
    return x[0] * GRAY[0] + x[1] * GRAY[1] + x[2] * GRAY[2]


def blend(x, m, f):
    return (x * f + m * (1.0 - f)).clamp(0.0, 1.0)


def rgb_to_hsv(x):
    r, g, b = x[0], x[1], x[2]
    maxc = torch.maximum(torch.maximum(r, g), b)
    minc = torch.minimum(torch.minimum(r, g), b)
    eqc = maxc == minc
    one = torch.ones_like(maxc)
    rng = maxc - minc
    s = rng / torch.where(eqc, one, maxc)
    div = torch.where(eqc, one, rng)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = torch.where(maxc == r, bc - gc, torch.where(maxc == g, (rc + 2.0) - bc, (gc + 4.0) - rc))
    h = torch.fmod(h * (1.0 / 6.0) + 1.0, 1.0)
    return h, s, maxc


def hsv_to_rgb(h, s, v):
    h6 = h * 6.0
    fl = torch.floor(h6)
    f = h6 - fl
    i = torch.remainder(fl.to(torch.int32), 6)
    sxf = s * f
    oms = 1.0 - s
    q = ((1.0 - sxf) * v).clamp(0.0, 1.0)
    t = ((sxf + oms) * v).clamp(0.0, 1.0)
    p = (oms * v).clamp(0.0, 1.0)
    table = {0: (v, t, p), 1: (q, v, p), 2: (p, v, t), 3: (p, q, v), 4: (t, p, v), 5: (v, p, q)}
    out = torch.zeros((3,) + tuple(h.shape), dtype=torch.float32)
    for k, chans in table.items():
        for c in range(3):
            out[c] = torch.where(i == k, chans[c], out[c])
    return out


def hue(x, factor):
    h, s, v = rgb_to_hsv(x)
    h = torch.remainder(h + factor, 1.0)
    return hsv_to_rgb(h, s, v)


class _AtContrast(Exception):
    def __init__(self, x):
        self.x = x


def color(x, prm, white=1.0, mean=None, at_contrast=False):
    """The colour ops and permutation on an f32 [3,H,W] image.  ``mean``: contrast's mean if given, else taken over
    the image at the point contrast runs.  ``at_contrast``: return that image (in the 1/white domain) instead."""
    x = x.to(torch.float32)
    ops = [prm.get(k) is not None for k in ("brightness", "contrast", "saturation", "hue")]
    if any(ops):
        x = x / torch.full_like(x, white)               # a true division (torch turns "/ scalar" into "* (1/scalar)")
        if prm.get("brightness") is not None:
            x = (x * prm["brightness"]).clamp(0.0, 1.0)

        def contrast(x):
            if at_contrast:
                raise _AtContrast(x)
            m = gray(x).mean() if mean is None else torch.tensor(mean, dtype=torch.float32)
            return blend(x, m, prm["contrast"])
        try:
            if prm.get("contrast") is not None and prm["contrast_before"]:
                x = contrast(x)
            if prm.get("saturation") is not None:
                x = blend(x, gray(x), prm["saturation"])
            if prm.get("hue") is not None:
                x = hue(x, prm["hue"])
            if prm.get("contrast") is not None and not prm["contrast_before"]:
                x = contrast(x)
        except _AtContrast as e:
            return e.x
        x = x * white
    if prm.get("perm") is not None:
        x = x[list(prm["perm"])]
    return x


def contrast_mean(x, prm, white=1.0):
    """Contrast's grayscale mean: over the image as it stands when contrast runs."""
    return gray(color(x, prm, white, at_contrast=True)).mean()


def resize(x, size):
    return F.interpolate(x[None], size=tuple(size), mode="bilinear", antialias=True, align_corners=False)[0]


def image(img_u8_hwc, prm, out_size=(600, 600), white=1.0):
    """u8 [H,W,3] -> f32 [3,OH,OW]: colour ops, permutation, flip, ScaleJitter's resize, Resize."""
    x = img_u8_hwc.permute(2, 0, 1).to(torch.float32)
    x = color(x, prm, white)
    if prm["flip"]:
        x = x.flip(-1)
    return resize(resize(x, prm["size"]), out_size)


def boxes(b, labels, H, W, prm, out_size=(600, 600), min_size=1.0):
    """XYXY f32 boxes: flip, x * fl32(new_w/W), y * fl32(new_h/H), then the same for out_size, SanitizeBoundingBoxes."""
    b = torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4).clone()
    labels = torch.as_tensor(labels, dtype=torch.int64).reshape(-1)
    if prm["flip"]:
        b = torch.stack([W - b[:, 2], b[:, 1], W - b[:, 0], b[:, 3]], 1)
    (nh, nw), (OH, OW) = prm["size"], out_size
    for (h0, w0), (h1, w1) in (((H, W), (nh, nw)), ((nh, nw), (OH, OW))):
        b = b * torch.tensor([w1 / w0, h1 / h0, w1 / w0, h1 / h0], dtype=torch.float32)
    keep = ((b[:, 2] - b[:, 0]) >= min_size) & ((b[:, 3] - b[:, 1]) >= min_size) & (b >= 0).all(1)
    keep &= (b[:, 0] <= OW) & (b[:, 2] <= OW) & (b[:, 1] <= OH) & (b[:, 3] <= OH)
    return b[keep], labels[keep]
