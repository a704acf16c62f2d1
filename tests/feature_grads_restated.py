"""Plain CPU restatements of the RoI pooling backward (csrc/feature_grads.hip): d feature map of the fused RoIPool + mean and of
the fused RoIAlign + mean, in float64, with the per-element bars tests/test_feature_grads_gpu.py holds the kernels to.  Nothing
here imports the package under test.

Positions are exact.  Every decision about WHERE a gradient goes - the RoI's map coordinates, spatial_scale, round half away
from zero, the bin edges, the sample coordinates, the [-1, H] skip, the clamp at 0 and at the far border, (int), and RoIPool's
first-maximum rule (strict '>', from -FLT_MAX, h outer, w inner; NaN never wins) - is restated op for op in f32 (numpy float32,
one rounding per operation), and the library is built with -ffp-contract=off, so the kernels and this module take the same
decision at every sample.  Only the sums round.

The bars are derived, not measured.  With u = 2^-24 (f32 round to nearest), for one element e of d_feat let
    T_e = the restatement applied to |d_out| (+ |base| under ``accumulate``): the sum of the magnitudes of the addends,
    N_e = the number of addends that reach e (non-zero weights only: a zero weight adds an exact 0).
The kernel owns e in one thread and adds its N_e terms in order to a register that starts at 0: the first add is exact, so
N_e - 1 roundings, and ``accumulate`` adds one more.  A term that took part in k rounded operations carries at most k u of its
magnitude (to first order), hence |got - exact| <= (N_e + r) u T_e, where r - 1 is the number of roundings inside one term:

  RoIPool    a term is d / (PH PW): one division.  N_e - 1 adds + 1 accumulate + 1 division = N_e + 1, and the bar is
                 POOL_BAR = (N_e + 2) u T_e                                        (one rounding of slack)
  RoIAlign   a term is gb * cw / count in the kernel's order, gb = d / nb, cw = (1 - ly | ly) * (1 - lx | lx):
                 d / nb (1), 1 - ly and 1 - lx (2; ly = y - (int)y itself is exact), the product of the two weights (1), the
                 product with gb (1), the division by count (1): six roundings, so r = ALIGN_R = 7 with the same one
                 rounding of slack, and the bar is
                 ALIGN_BAR = (N_e + 7) u T_e
  The slack covers the second-order terms ((N_e + r) u)^2 / 2 while N_e stays below about 5000; the one case beyond that
  (B R = 65535, N_e about 13107) keeps the same bar, which a correct f32 sum misses only if nearly all its roundings fall the
  same way.
  Where N_e == 0 nothing reaches the element: the kernel must write exactly 0, and under ``accumulate`` exactly the base.

``kernel_order_f32`` sums the same terms in f32 in the kernel's order (RoI groups in order, RoIs ascending, bins, samples,
corners) - what a correct f32 implementation gives; a CPU test holds it to the bars.
"""
import numpy as np
import torch

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
POOL_R = 2
ALIGN_R = 7


# ------------------------------------------------------------------------------------------------------------ geometry
def _f32(v):
    return np.float32(v)


def _roundf(v):
    v = float(np.float32(v))
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def roi_to_map(r, img_h, img_w, Hf, Wf):
    """nets/classify.py:35-36 in f32: (x1, y1, x2, y2) image -> map coordinates."""
    x1, y1, x2, y2 = (np.float32(v) for v in r)
    return (_f32(x1 / _f32(img_w)) * _f32(Wf), _f32(y1 / _f32(img_h)) * _f32(Hf), _f32(x2 / _f32(img_w)) * _f32(Wf),
            _f32(y2 / _f32(img_h)) * _f32(Hf))


def pool_bins(fm, Hf, Wf, PH=7, PW=7, scale=1.0):
    """torchvision RoIPool's bins of one map-coordinate RoI: [(ph, pw, hs, he, ws, we)]."""
    s = _f32(scale)
    sw, sh, ew, eh = (_roundf(_f32(v) * s) for v in fm)
    rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
    bh, bw = _f32(rh) / _f32(PH), _f32(rw) / _f32(PW)
    out = []
    for ph in range(PH):
        hs = min(max(int(np.floor(_f32(ph) * bh)) + sh, 0), Hf)
        he = min(max(int(np.ceil(_f32(ph + 1) * bh)) + sh, 0), Hf)
        for pw in range(PW):
            ws = min(max(int(np.floor(_f32(pw) * bw)) + sw, 0), Wf)
            we = min(max(int(np.ceil(_f32(pw + 1) * bw)) + sw, 0), Wf)
            out.append((ph, pw, hs, he, ws, we))
    return out


def pool_extent(fm, Hf, Wf, PH=7, PW=7, scale=1.0):
    """roi_pool_argmax_kernel's ext record (y0, y1, x0, x1): first bin's start and last bin's end on each axis."""
    bins = pool_bins(fm, Hf, Wf, PH, PW, scale)
    return bins[0][2], bins[-1][3], bins[0][4], bins[-1][5]


# ------------------------------------------------------------------------------------------------------------- RoIPool
def pool_argmax(feat, rois, roi_indices, img_h, img_w, PH=7, PW=7, spatial_scale=1.0):
    """feat [B,C,Hf,Wf] f32, rois [B,R,4] image coords -> [(k, b, idx [PH*PW, C] long map index or -1)] by torchvision's rule
    (first maximum, h outer, w inner, above -FLT_MAX only, NaN never above anything; -1 for empty bins).  A group whose
    roi_indices entry names no image of the batch is left out: it reads and adds nothing."""
    B, C, Hf, Wf = feat.shape
    R = rois.shape[1]
    feat = torch.where(torch.isnan(feat), torch.full_like(feat, float("-inf")), feat)      # 'v > m' is false for a NaN
    out = []
    for k, r in enumerate(rois.reshape(-1, 4).tolist()):
        b = int(roi_indices[k // R])
        if not 0 <= b < B:
            continue
        idx = torch.full((PH * PW, C), -1, dtype=torch.long)
        for ph, pw, hs, he, ws, we in pool_bins(roi_to_map(r, img_h, img_w, Hf, Wf), Hf, Wf, PH, PW, spatial_scale):
            if he <= hs or we <= ws:
                continue
            win = feat[b, :, hs:he, ws:we].reshape(C, -1)
            j = torch.argmax(win, dim=1)
            ok = win.gather(1, j[:, None])[:, 0] > -FLT_MAX
            idx[ph * PW + pw] = torch.where(ok, (hs + j // (we - ws)) * Wf + ws + j % (we - ws), -1)
        out.append((k, b, idx))
    return out


def pool_avg_by_gather(X, argmax, K=None):
    """Differentiable RoIPool + mean: X [B,C,Hf,Wf] (any dtype) -> [K, C] gathering X at the f32 arg-max (rows of RoIs that
    pool_argmax left out are 0 when ``K``, the number of RoIs, is given)."""
    B, C = X.shape[:2]
    flat = X.reshape(B, C, -1)
    rows = {}
    for k, b, idx in argmax:
        ok = idx >= 0
        v = flat[b].gather(1, idx.clamp(min=0).T).T * ok                   # [bins, C]
        rows[k] = v.sum(0) / idx.shape[0]
    if K is None:
        return torch.stack([rows[k] for k in sorted(rows)])
    zero = X.new_zeros(C)
    return torch.stack([rows.get(k, zero) for k in range(K)])


def pool_avg_grad_f64(feat, rois, roi_indices, img_h, img_w, d_out, PH=7, PW=7, spatial_scale=1.0):
    """float64 d feat [B,C,Hf,Wf] of the fused RoIPool + mean (autograd through pool_avg_by_gather)."""
    X = feat.double().clone().requires_grad_(True)
    am = pool_argmax(feat, rois, roi_indices, img_h, img_w, PH, PW, spatial_scale)
    if not am:
        return torch.zeros_like(X)
    y = pool_avg_by_gather(X, am, rois.shape[0] * rois.shape[1])
    (y * d_out.double()).sum().backward()
    return X.grad


def pool_grad_ref(feat, rois, roi_indices, img_h, img_w, d_out, PH=7, PW=7, spatial_scale=1.0, argmax=None):
    """-> (want, T, N) [B,C,Hf,Wf]: the float64 gradient by a plain scatter over the arg-max record (the same numbers as
    pool_avg_grad_f64), the same scatter of |d_out| / (PH PW), and the number of bins every element wins."""
    B, C, Hf, Wf = feat.shape
    am = pool_argmax(feat, rois, roi_indices, img_h, img_w, PH, PW, spatial_scale) if argmax is None else argmax
    want = torch.zeros((B, C, Hf * Wf), dtype=torch.float64)
    T = torch.zeros_like(want)
    N = torch.zeros((B, C, Hf * Wf), dtype=torch.int64)
    g = d_out.double() / (PH * PW)
    for k, b, idx in am:
        ok = (idx >= 0).T                                                  # [C, bins]
        at = idx.clamp(min=0).T
        want[b].scatter_add_(1, at, g[k][:, None] * ok)
        T[b].scatter_add_(1, at, g[k].abs()[:, None] * ok)
        N[b].scatter_add_(1, at, ok.long())
    shape = (B, C, Hf, Wf)
    return want.view(shape), T.view(shape), N.view(shape)


def pool_terms(argmax, shape, PH, PW):
    """The addends of every element in the kernel's order -> (element index into [B,C,Hf,Wf] flat, RoI k, channel)."""
    B, C, Hf, Wf = shape
    elem, ks, cs = [], [], []
    ch = torch.arange(C)
    for k, b, idx in argmax:                                               # k ascending = group order, then RoI order
        ok = idx >= 0                                                      # [bins, C], bins in (ph, pw) order
        bins, c = torch.nonzero(ok, as_tuple=True)
        elem.append((b * C + ch[c]) * Hf * Wf + idx[bins, c])
        ks.append(torch.full_like(c, k))
        cs.append(c)
    if not elem:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    return torch.cat(elem).numpy(), torch.cat(ks).numpy(), torch.cat(cs).numpy()


# ------------------------------------------------------------------------------------------------------------ RoIAlign
def align_geom(fm, PH, PW, sampling_ratio, aligned, scale=1.0):
    """tsod_roi_align_geom in f32 -> (start_h, start_w, bin_h, bin_w, grid_h, grid_w, count)."""
    s = _f32(scale)
    x1, y1, x2, y2 = (_f32(v) * s for v in fm)
    off = _f32(0.5 if aligned else 0.0)
    sw_, sh_ = x1 - off, y1 - off
    rw, rh = (x2 - off) - sw_, (y2 - off) - sh_
    if not aligned:
        rw, rh = max(rw, _f32(1)), max(rh, _f32(1))
    bh, bw = rh / _f32(PH), rw / _f32(PW)
    gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rh / _f32(PH)))
    gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rw / _f32(PW)))
    return sh_, sw_, bh, bw, gh, gw, max(gh * gw, 1)


def align_axis(start, bin_, grid, P, n):
    """One axis of TSOD_ALIGN_SAMPLE + TSOD_ALIGN_BILINEAR_OR_CONTINUE for every (bin p, sample i), in f32 ->
    (coordinate, skipped, low, high, l) each [P, max(grid, 0)]."""
    p = np.arange(P, dtype=np.float32)[:, None]
    i = np.arange(max(grid, 0), dtype=np.float32)[None, :]
    with np.errstate(all="ignore"):
        c = _f32(start) + p * _f32(bin_) + (i + _f32(.5)) * _f32(bin_) / _f32(max(grid, 1))
    assert c.dtype == np.float32
    skip = (c < -1) | (c > n)
    cc = np.where(c <= 0, _f32(0), c)
    low = np.where(skip, 0, cc).astype(np.int64)                           # (int): truncation of a value >= 0
    edge = low >= n - 1
    low = np.where(edge, n - 1, low)
    high = np.where(edge, n - 1, low + 1)
    cc = np.where(edge, low.astype(np.float32), cc)
    l = (cc - low.astype(np.float32)).astype(np.float32)
    return c, skip, low, high, l


def align_roi_terms(fm, Hf, Wf, PH, PW, sampling_ratio, aligned, scale=1.0):
    """One map-coordinate RoI -> (pix, w64, w32, count): the map index h * Wf + w, the float64 weight and the kernel's f32
    weight of every (bin, sample, corner) that is not skipped, in the kernel's order (ph, pw, iy, ix, corner)."""
    sh_, sw_, bh, bw, gh, gw, count = align_geom(fm, PH, PW, sampling_ratio, aligned, scale)
    _, sky, yl, yh, ly = align_axis(sh_, bh, gh, PH, Hf)
    _, skx, xl, xh, lx = align_axis(sw_, bw, gw, PW, Wf)
    if sky.size == 0 or skx.size == 0:
        z = np.zeros(0)
        return z.astype(np.int64), z, z.astype(np.float32), count
    hy, hx = (_f32(1) - ly).astype(np.float32), (_f32(1) - lx).astype(np.float32)
    ly64, lx64 = ly.astype(np.float64), lx.astype(np.float64)
    hy64, hx64 = 1 - ly64, 1 - lx64
    Y = lambda a: a[:, None, :, None]                                      # noqa: E731  [PH, 1, gh, 1]
    X = lambda a: a[None, :, None, :]                                      # noqa: E731  [1, PW, 1, gw]
    full = (PH, PW, max(gh, 0), max(gw, 0))
    keep = np.broadcast_to(~Y(sky) & ~X(skx), full)
    cy = np.stack([np.broadcast_to(Y(v), full) for v in (yl, yl, yh, yh)], -1)
    cx = np.stack([np.broadcast_to(X(v), full) for v in (xl, xh, xl, xh)], -1)
    w64 = np.stack([Y(hy64) * X(hx64), Y(hy64) * X(lx64), Y(ly64) * X(hx64), Y(ly64) * X(lx64)], -1)
    w32 = np.stack([Y(hy) * X(hx), Y(hy) * X(lx), Y(ly) * X(hx), Y(ly) * X(lx)], -1)
    assert w32.dtype == np.float32
    m = np.broadcast_to(keep[..., None], cy.shape)
    return (cy * Wf + cx)[m], w64[m], w32[m], count


def align_walk(shape, rois, roi_indices, img_h, img_w, PH=7, PW=7, sampling_ratio=2, aligned=False, spatial_scale=1.0):
    """Every RoI whose group names an image of the batch -> [(k, b, pix, w64, w32, count)], k ascending."""
    B, C, Hf, Wf = shape
    R = rois.shape[1]
    out = []
    for k, r in enumerate(rois.reshape(-1, 4).tolist()):
        b = int(roi_indices[k // R])
        if not 0 <= b < B:
            continue
        fm = roi_to_map(r, img_h, img_w, Hf, Wf)
        out.append((k, b) + align_roi_terms(fm, Hf, Wf, PH, PW, sampling_ratio, aligned, spatial_scale))
    return out


def align_maps(walk, shape, K):
    """The walk as two matrices [K, B*Hf*Wf]: W = the sum of a RoI's weights on every pixel / count (float64), and
    Nn = the number of its non-zero weights there.  They depend on the geometry alone, not on d_out or C."""
    B, C, Hf, Wf = shape
    npix = Hf * Wf
    W = torch.zeros((K, B * npix), dtype=torch.float64)
    Nn = torch.zeros((K, B * npix), dtype=torch.float64)
    for k, b, pix, w64, w32, count in walk:
        W[k, b * npix:(b + 1) * npix] = torch.from_numpy(np.bincount(pix, weights=w64, minlength=npix) / count)
        Nn[k, b * npix:(b + 1) * npix] = torch.from_numpy(np.bincount(pix[w64 != 0], minlength=npix).astype(np.float64))
    return W, Nn


def align_grad_ref(shape, rois, roi_indices, img_h, img_w, d_out, PH=7, PW=7, sampling_ratio=2, aligned=False,
                   spatial_scale=1.0, maps=None):
    """-> (want, T, N) [B,C,Hf,Wf]: float64 d feat of the fused RoIAlign + mean, the same walk on |d_out| (every weight is
    >= 0), and the number of non-zero addends of every element."""
    B, C, Hf, Wf = shape
    K = rois.shape[0] * rois.shape[1]
    if maps is None:
        maps = align_maps(align_walk(shape, rois, roi_indices, img_h, img_w, PH, PW, sampling_ratio, aligned, spatial_scale),
                          shape, K)
    W, Nn = maps
    g = d_out.double() / (PH * PW)
    nchw = lambda m: m.view(B, Hf, Wf, -1).permute(0, 3, 1, 2).contiguous()   # noqa: E731
    N = Nn.sum(0).view(B, 1, Hf, Wf).expand(B, C, Hf, Wf).round().long()
    return nchw(W.T @ g), nchw(W.T @ g.abs()), N


def align_avg_grad_f64(shape, rois, roi_indices, img_h, img_w, d_out, PH=7, PW=7, sampling_ratio=2, aligned=False,
                       spatial_scale=1.0):
    """float64 d feat [B,C,Hf,Wf] of the fused RoIAlign + mean: torchvision's roi_align backward (positions, skips, clamps in
    f32 as the kernels compute them; the weights and sums in float64)."""
    return align_grad_ref(shape, rois, roi_indices, img_h, img_w, d_out, PH, PW, sampling_ratio, aligned, spatial_scale)[0]


def align_span(start, bin_, P, n):
    """feature_grads.hip's align_span in f32: the [lo, hi) superset of the pixels that samples between start and
    start + P bin touch -> (lo, hi, clamped) where ``clamped`` says that the +-4 clamp cut an end."""
    end = _f32(start) + _f32(P) * _f32(bin_)
    lo_raw, hi_raw = min(_f32(start), end), max(_f32(start), end)
    a = min(max(lo_raw, _f32(-4)), _f32(n) + _f32(4))
    z = min(max(hi_raw, _f32(-4)), _f32(n) + _f32(4))
    return max(int(np.floor(a)) - 1, 0), min(int(np.floor(z)) + 3, n), bool(a != lo_raw or z != hi_raw)


# -------------------------------------------------------------------------------------------------------------- the bars
def pool_bar(T, N):
    return (N.double() + POOL_R) * U * T


def align_bar(T, N):
    return (N.double() + ALIGN_R) * U * T


def with_base(want, T, N, base):
    """``accumulate`` onto ``base`` [B,C,Hf,Wf]: the sum gains the base, T its magnitude (the count stays: the accumulate add
    is one of the roundings the bars already hold)."""
    return want + base.double(), T + base.double().abs(), N


# --------------------------------------------------------------------------------------------- f32 in the kernel's order
def ordered_f32_sums(elem, vals, n):
    """out[e] = the f32 sum, from 0 and in the order given, of the vals whose elem is e ([n] f32): all elements advance in
    lockstep, one addend each per step, so the loop runs max N_e times."""
    out = np.zeros(n, dtype=np.float32)
    if elem.size == 0:
        return out
    order = np.argsort(elem, kind="stable")
    e, v = elem[order], vals[order].astype(np.float32)
    first = np.r_[True, e[1:] != e[:-1]]
    start = np.flatnonzero(first)
    rank = np.arange(e.size) - np.repeat(start, np.diff(np.r_[start, e.size]))
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2))
    for r in range(rank.max() + 1):
        sel = by_rank[bounds[r]:bounds[r + 1]]
        out[e[sel]] = out[e[sel]] + v[sel]
    return out


def kernel_order_f32(op, shape, d_out, PH, PW, argmax=None, walk=None, base=None):
    """[B,C,Hf,Wf] f32: every element's sum as a correct f32 implementation takes it, in the kernel's order and with the
    kernel's operations (d / nb first; for RoIAlign gb * cw / count with the f32 weights), ``base`` added last."""
    B, C, Hf, Wf = shape
    npix = Hf * Wf
    d = d_out.numpy().astype(np.float32)
    gb = (d / np.float32(PH * PW)).astype(np.float32)
    if op == "pool":
        elem, ks, cs = pool_terms(argmax, shape, PH, PW)
        vals = gb[ks, cs]
    else:
        elems, vs = [], []
        ch = np.arange(C)
        for k, b, pix, w64, w32, count in walk:
            elems.append(((b * C + ch[None, :]) * npix + pix[:, None]).reshape(-1))
            vs.append(((gb[k][None, :] * w32[:, None]).astype(np.float32) / np.float32(count)).astype(np.float32).reshape(-1))
        elem = np.concatenate(elems) if elems else np.zeros(0, dtype=np.int64)
        vals = np.concatenate(vs) if vs else np.zeros(0, dtype=np.float32)
    out = torch.from_numpy(ordered_f32_sums(elem, vals, B * C * npix)).view(B, C, Hf, Wf)
    return out if base is None else base.float() + out
