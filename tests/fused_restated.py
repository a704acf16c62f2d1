"""Float64 restatements of the two one-launch kernels, tsod_stem_fp16x2 (csrc/stem_fused.hip) and tsod_bottleneck_fp16x2
(csrc/bottleneck_fused.hip), in plain torch on the CPU; the per-element error bound E each output is held to; a CPU emulation
of the kernels' arithmetic (the check that the bound can be met at all, and - with a fault planted - that it bites); the
launchers' rules restated; and the case table of tests/test_fused_kernels_gpu.py.  No call into the library.

Layouts are the kernels' own: bottleneck activations are NHWC, w1 [64, Cin], w2 [64, 3, 3, 64] ([Cout][KH][KW][Cin]),
w3 [Cout, 64], the projection's wd [Cout, Cin]; the stem takes NCHW images and w [64, 3, 7, 7] and returns the pooled NHWC map.

How E is derived.  conv_restated's docstring gives, for ONE fp16x2 contraction of length K followed by scale, shift, residual
and PReLU,  |got - y| <= bar(FP16X2, K) T  with  T = |scale| conv(m(a), m(w)) + |shift| + |residual|,  m(v) = max(|v|, 2^-3 / s)
and s the power of two the operand was scaled by before it was split into two fp16 pieces.  The weights' s is 2^w_exp of their
matrix.  The activations' s is what each kernel takes it from:

  stem         one s per pooled 4 x 16 tile: 2^e with e = exp_from_max(abs-max of the tile's 23 x 71 input patch), pixels outside
               the image being zeros.  The max is over the inputs themselves, so the reference knows e exactly.
               E_conv = bar(147) T, and through the 3x3/2 max pool  E = maxpool(E_conv)  over the same windows (a max is
               1-Lipschitz in the sup norm; a window only holds conv pixels inside the conv output).
  bottleneck   x: 2^e_x from the tensor's range words (or the static exponent).  y1 and y2: tile-local, from the abs-max of what
               the workgroup computed - y1 over the halo rows of the tile that lie inside the image, y2 over all TH x 16 rows of the
               tile (rows past the image edge hold y2 of the zero-extended y1).  The kernel's y1 / y2 differ from the reference's
               by up to E1 / E2, so a maximum next to a power of two may give the kernel the neighbouring exponent: the floor is
               taken for ONE EXPONENT LESS than the reference's (twice as large), which covers both.
               Stage by stage (PReLU with |slope| <= 1 is 1-Lipschitz, so an input error passes through a stage multiplied by the
               absolute weights and scale):
                   E1 = bar(Cin) T1
                   E2 = bar(576) T2 + |s2| conv3x3(E1, |w2|)
                   E3 = bar(64)  T3 + |s3| conv1x1(E2, |w3|)        T3 includes |x| (the residual)
               and for the projection form, whose conv3 is ONE stacked contraction [y2 | x] . [W3 s3 | Wd sd]^T (scale 1, shift
               b3 + bd, one weight exponent for the stacked matrix; the accumulator's change of scale between the two operands is a
               power of two: exact)
                   E3 = bar(64 + Cin) T3 + conv1x1(E2, |W3 s3|)     T3 = m(y2) . m(W3 s3) + m(x) . m(Wd sd) + |b3 + bd|
               The reference contracts the SAME f32 stacked matrix and shift the kernel is handed (``stack_projection``).

What E does not promise: tightness at the K of real layers.  bar() is a worst case, linear in K, and E3 carries conv2's K = 576;
random data sits one to two orders of magnitude below it.  A wrong index, a missing tap, a wrong scale or a dropped piece on aligned
data is of order T or 2^-11 T and shows; the sqrt(K) bars of tests/test_hip_ops.py stay for the statistical side."""
import math
import zlib
from typing import NamedTuple, Optional

import torch

import conv_restated as R

FLOOR = R.FP16_FLOOR
TW, TPH, TPW = 16, 4, 16                  # bottleneck tile width; pooled rows / columns of a stem tile
PATCH_H, PATCH_W = 23, 71                 # the stem tile's input patch


# ----------------------------------------------------------------------------- exponents
def exp_from_max(m: float) -> int:
    """tsod_fp16x2_exp_from_bits on the value of an abs-max: 2^e m in [2^14, 2^15), e in [-24, 24]; zero: 24, inf: -24."""
    m = float(torch.tensor(m, dtype=torch.float64).float())           # (the kernel's maximum is an f32)
    if m == 0.0:
        return 24
    if not math.isfinite(m):
        return -24
    return max(-24, min(24, 14 - (math.frexp(m)[1] - 1)))


def weight_exp(w) -> int:
    """hip_ops.fp16x2_weight_scale_exp restated"""
    return R.fp16x2_exponents(1.0, float(w.abs().max()))[1]


def prelu(v, slope):
    return torch.where(v >= 0, v, v * slope)


def _f64(t):
    return t.detach().to("cpu", torch.float64)


# ----------------------------------------------------------------------------- launch rules
def bottleneck_wave_mfmas(TH: int, Cin: int, Cout: int, proj: bool) -> int:
    """MFMAs the slowest wave issues per tile: 3 per (16-k chunk, pixel block) - conv1 over its halo blocks (3 of 6 / 4 of 7),
    conv2's 36 chunks and conv3's chunks per 64-channel slice over its tile blocks (2 of 4 / 3 of 5)."""
    n1, nq = Cin // 32, Cout // 64
    c3 = 4 + 2 * n1 if proj else 4
    nb1, nb2 = (3, 2) if TH == 8 else (4, 3)
    return 3 * (nb1 * 2 * n1 + nb2 * 36 + nb2 * c3 * nq)


def bottleneck_rounds(TH: int, N: int, H: int, W: int, cus: int) -> int:
    tiles = N * (-(-W // TW)) * (-(-H // TH))
    return -(-tiles // (2 * cus))


def bottleneck_tile_height(N, H, W, Cin, Cout, proj, cus) -> int:
    """rounds of the launch (two workgroups per CU) x MFMAs of the slowest wave: 8 rows unless 10 are strictly cheaper"""
    c8 = bottleneck_rounds(8, N, H, W, cus) * bottleneck_wave_mfmas(8, Cin, Cout, proj)
    c10 = bottleneck_rounds(10, N, H, W, cus) * bottleneck_wave_mfmas(10, Cin, Cout, proj)
    return 8 if c8 < c10 else 10


def stem_out_hw(H, W):
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return oh, ow, (oh - 1) // 2 + 1, (ow - 1) // 2 + 1


class StemLaunch(NamedTuple):
    tiles_x: int
    tiles_y: int
    tiles: int
    slots: int
    rounds: int
    grid: int


def stem_launch(N, H, W, cus) -> StemLaunch:
    """persistent workgroups, two per CU; round r covers tiles [r grid, (r + 1) grid)"""
    _, _, ph, pw = stem_out_hw(H, W)
    tx, ty = -(-pw // TPW), -(-ph // TPH)
    tiles, slots = N * tx * ty, 2 * cus
    rounds = -(-tiles // slots)
    return StemLaunch(tx, ty, tiles, slots, rounds, -(-tiles // rounds))


# ----------------------------------------------------------------------------- pieces shared by reference and emulation
def _taps(xp, w, stride, OH, OW):
    """xp [N, Hp, Wp, C] already padded, w [Cout, KH, KW, C] -> [N, OH, OW, Cout]: a sum over taps of shifted slices"""
    acc = torch.zeros(xp.shape[0], OH, OW, w.shape[0], dtype=torch.float64)
    for kh in range(w.shape[1]):
        for kw in range(w.shape[2]):
            v = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
            acc += (v.reshape(-1, v.shape[-1]) @ w[:, kh, kw, :].T).view(acc.shape)      # (one plain matrix product per tap)
    return acc


def _pad(x, p, value=0.0):
    N, H, W, C = x.shape
    xp = torch.full((N, H + 2 * p, W + 2 * p, C), value, dtype=x.dtype)
    xp[:, p:p + H, p:p + W] = x
    return xp


def _pool(v, fill):
    """3x3 / 2 pad 1 maximum of [N, OH, OW, C]; ``fill`` stands outside the conv output"""
    N, OH, OW, C = v.shape
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    vp = torch.full((N, 2 * PH + 1, 2 * PW + 1, C), fill, dtype=v.dtype)
    vp[:, 1:1 + OH, 1:1 + OW] = v
    out = torch.full((N, PH, PW, C), -math.inf, dtype=v.dtype)
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, vp[:, dy:dy + 2 * PH - 1:2, dx:dx + 2 * PW - 1:2])
    return out


def split(v, e):
    """the two fp16 pieces of 2^e v as the kernels make them (tsod_split2_pair), returned as f64"""
    s = v.float() * (2.0 ** e)
    hi = s.half()
    lo = (s - hi.float()).half()
    return hi.double(), lo.double()


def _mm3(ah, al, wh, wl, fault):
    """the three piece products of tsod_mfma3, sums in f64: a [.., K], w [Cout, K]"""
    acc = ah @ wh.T + al @ wh.T
    return acc if fault == "drop_cross" else acc + ah @ wl.T


def _taps3(ah, al, wh, wl, stride, OH, OW, fault):
    acc = _taps(ah, wh, stride, OH, OW) + _taps(al, wh, stride, OH, OW)
    return acc if fault == "drop_cross" else acc + _taps(ah, wl, stride, OH, OW)


# ----------------------------------------------------------------------------- the stem
def stem_tile_exponents(x):
    """x [N, 3, H, W] -> int64 [N, PH, PW]: for every pooled pixel the exponent its tile takes from its input patch"""
    N, _, H, W = x.shape
    _, _, ph, pw = stem_out_hw(H, W)
    out = torch.zeros(N, ph, pw, dtype=torch.int64)
    ax = x.detach().abs().float()
    for ty in range(-(-ph // TPH)):
        for tx in range(-(-pw // TPW)):
            y0, x0 = 4 * TPH * ty - 5, 4 * TPW * tx - 5
            patch = ax[:, :, max(y0, 0):min(y0 + PATCH_H, H), max(x0, 0):min(x0 + PATCH_W, W)]
            mx = patch.reshape(N, -1).amax(dim=1)
            e = torch.tensor([exp_from_max(float(m)) for m in mx])
            out[:, TPH * ty:TPH * (ty + 1), TPW * tx:TPW * (tx + 1)] = e.view(N, 1, 1)
    return out


def stem_ref(x, w, scale, shift, slope):
    """-> (y, E), both f64 [N, PH, PW, 64]"""
    N, _, H, W = x.shape
    oh, ow, ph, pw = stem_out_hw(H, W)
    xg, wk = _f64(x).permute(0, 2, 3, 1), _f64(w).permute(0, 2, 3, 1)
    s, b = _f64(scale), _f64(shift)
    y = _pool(prelu(_taps(_pad(xg, 3), wk, 2, oh, ow) * s + b, slope), -math.inf)
    mw = wk.abs().clamp_min(FLOOR / 2.0 ** weight_exp(w))
    emap = stem_tile_exponents(x)
    E = torch.zeros_like(y)
    for e in emap.unique().tolist():
        # (the floor before the zero padding: a padding tap is no operand)
        T = _taps(_pad(xg.abs().clamp_min(FLOOR / 2.0 ** e), 3), mw, 2, oh, ow) * s.abs() + b.abs()
        E = torch.where((emap == e).unsqueeze(-1), _pool(R.bar(R.FP16X2, 147) * T, 0.0), E)
    return y, E


def stem_emulate(x, w, scale, shift, slope, fault=None):
    """the kernel's arithmetic on the CPU: pieces by .half() at the kernel's scales, piece products and sums in f64, the BN + PReLU
    result rounded to f32 (what the conv tile in LDS holds) -> f64 [N, PH, PW, 64]"""
    N, _, H, W = x.shape
    oh, ow, ph, pw = stem_out_hw(H, W)
    xg, wk = x.detach().float().permute(0, 2, 3, 1), w.detach().float().permute(0, 2, 3, 1)
    s, b = _f64(scale), _f64(shift)
    we = weight_exp(w)
    wh, wl = split(wk, we)
    emap = stem_tile_exponents(x)
    out = torch.zeros(N, ph, pw, 64, dtype=torch.float64)
    for e in emap.unique().tolist():
        xh, xl = split(xg, e)
        acc = _taps3(_pad(xh, 3), _pad(xl, 3), wh, wl, 2, oh, ow, fault) * 2.0 ** -(e + we)
        conv = prelu(acc * s + b, slope).float().double()
        out = torch.where((emap == e).unsqueeze(-1), _pool(conv, -math.inf), out)
    return out


# ----------------------------------------------------------------------------- the bottleneck
def stack_projection(w3, s3, wd, sd, b3, bd):
    """the stacked f32 matrix [W3 s3 | Wd sd] and the f32 shift b3 + bd the projection form is handed (folded in f64, rounded once)"""
    ws = torch.cat([_f64(w3) * _f64(s3).view(-1, 1), _f64(wd) * _f64(sd).view(-1, 1)], dim=1).float()
    return ws, (_f64(b3) + _f64(bd)).float()


def _tiles(N, H, W, TH):
    for n in range(N):
        for h0 in range(0, H, TH):
            for w0 in range(0, W, TW):
                yield n, h0, w0


def _extend(v, TH, ring):
    """[N, H, W, C] zero-extended to whole tiles plus ``ring`` pixels all round"""
    N, H, W, C = v.shape
    He, We = -(-H // TH) * TH, -(-W // TW) * TW
    out = torch.zeros(N, He + 2 * ring, We + 2 * ring, C, dtype=v.dtype)
    out[:, ring:ring + H, ring:ring + W] = v
    return out


def bottleneck_ref(x, w1, w2, w3, bn, slope, *, wd=None, bnd=None, e_x, TH):
    """x [N, H, W, Cin] -> (y, E), both f64 [N, H, W, Cout].  ``wd`` [Cout, Cin], ``bnd`` = (sd, bd): the projection form."""
    x, w1, w2 = _f64(x), _f64(w1), _f64(w2)
    s1, b1, s2, b2, s3, b3 = (_f64(v) for v in bn)
    N, H, W, Cin = x.shape
    proj = wd is not None
    if proj:
        ws, bs = stack_projection(w3, s3, wd, bnd[0], b3, bnd[1])
        w3k, s3, b3 = _f64(ws), torch.ones_like(b3), _f64(bs)
    else:
        w3k = _f64(w3)
    fx = FLOOR / 2.0 ** e_x
    mw1, mw2, mw3 = (m.abs().clamp_min(FLOOR / 2.0 ** weight_exp(m)) for m in (w1, w2, w3k))
    mx = x.abs().clamp_min(fx)
    # stage 1
    y1 = prelu((x @ w1.T) * s1 + b1, slope)
    E1 = R.bar(R.FP16X2, Cin) * ((mx @ mw1.T) * s1.abs() + b1.abs())
    # stage 2: y2 on the whole-tile extension of the image (what the workgroups compute), its bound per tile
    inside = _extend(torch.ones(N, H, W, 1, dtype=torch.float64), TH, 1)
    y1e = _extend(y1, TH, 1)
    He, We = y1e.shape[1] - 2, y1e.shape[2] - 2
    y2e = prelu(_taps(y1e, w2, 1, He, We) * s2 + b2, slope)
    prop2 = _taps(_extend(E1, TH, 1), w2.abs(), 1, He, We) * s2.abs()
    E2 = torch.zeros_like(y2e)
    F2 = torch.zeros(N, He, We, 1, dtype=torch.float64)              # y2's floor, per pixel of its tile
    for n, h0, w0 in _tiles(N, H, W, TH):
        blk = slice(h0, h0 + TH + 2), slice(w0, w0 + TW + 2)
        halo = y1e[n][blk].abs()
        f1 = FLOOR / 2.0 ** (exp_from_max(float(halo.max())) - 1)
        m1 = (halo.clamp_min(f1) * inside[n][blk]).unsqueeze(0)
        T2 = _taps(m1, mw2, 1, TH, TW)[0] * s2.abs() + b2.abs()
        own = slice(h0, h0 + TH), slice(w0, w0 + TW)
        E2[n][own] = R.bar(R.FP16X2, 576) * T2 + prop2[n][own]
        F2[n][own] = FLOOR / 2.0 ** (exp_from_max(float(y2e[n][own].abs().max())) - 1)
    y2, E2, m2 = y2e[:, :H, :W], E2[:, :H, :W], y2e[:, :H, :W].abs().clamp_min(F2[:, :H, :W])
    # stage 3
    if proj:
        y = prelu(y2 @ w3k[:, :64].T + x @ w3k[:, 64:].T + b3, slope)
        T3 = m2 @ mw3[:, :64].T + mx @ mw3[:, 64:].T + b3.abs()
        E = R.bar(R.FP16X2, 64 + Cin) * T3 + E2 @ w3k[:, :64].abs().T
    else:
        y = prelu((y2 @ w3k.T) * s3 + b3 + x, slope)
        T3 = (m2 @ mw3.T) * s3.abs() + b3.abs() + x.abs()
        E = R.bar(R.FP16X2, 64) * T3 + (E2 @ w3k.abs().T) * s3.abs()
    return y, E


FAULTS = ("pad_x", "drop_cross", "halo_lo")


def bottleneck_emulate(x, w1, w2, w3, bn, slope, *, wd=None, bnd=None, e_x, TH, fault=None):
    """The kernel's arithmetic on the CPU, tile by tile: pieces by .half() at the kernel's scales and tile-local exponents, piece
    products and sums in f64, y1 / y2 / out rounded to f32 where the kernel holds f32 -> f64 [N, H, W, Cout].  ``fault``:
      "pad_x"       x is zero-padded instead of y1: a halo pixel outside the image holds PReLU(b1), not 0
      "drop_cross"  tsod_mfma3 without its lo * hi product (weights' low piece times activations' high piece), in every conv
      "halo_lo"     y1's low piece is missing on the halo rows (every row of the halo that is no pixel of the tile itself)"""
    xf = x.detach().float()
    N, H, W, Cin = xf.shape
    s1, b1, s2, b2, s3, b3 = (_f64(v) for v in bn)
    proj = wd is not None
    if proj:
        w3m, bs = stack_projection(w3, s3, wd, bnd[0], b3, bnd[1])
        s3, b3 = torch.ones_like(b3), _f64(bs)
    else:
        w3m = w3.detach().float()
    we1, we2, we3 = weight_exp(w1), weight_exp(w2), weight_exp(w3m)
    w1h, w1l = split(w1, we1)
    w2h, w2l = split(w2, we2)
    w3h, w3l = split(w3m, we3)
    xh, xl = split(xf, e_x)
    y1 = prelu(_mm3(xh, xl, w1h, w1l, fault) * 2.0 ** -(e_x + we1) * s1 + b1, slope).float()
    y1e = _extend(y1, TH, 1)
    inside = _extend(torch.ones(N, H, W, 1), TH, 1)
    if fault == "pad_x":
        y1e = torch.where(inside > 0, y1e, prelu(b1, slope).float().expand_as(y1e))
    own_mask = torch.zeros(TH + 2, TW + 2, 1, dtype=torch.float64)
    own_mask[1:-1, 1:-1] = 1.0
    Cout = w3m.shape[0]
    out = torch.zeros(N, H, W, Cout, dtype=torch.float64)
    for n, h0, w0 in _tiles(N, H, W, TH):
        blk = slice(h0, h0 + TH + 2), slice(w0, w0 + TW + 2)
        halo = y1e[n][blk]
        e1 = exp_from_max(float((halo * inside[n][blk]).abs().max()))
        h, l = split(halo, e1)
        if fault == "halo_lo":
            l = l * own_mask
        acc2 = _taps3(h.unsqueeze(0), l.unsqueeze(0), w2h, w2l, 1, TH, TW, fault)[0] * 2.0 ** -(e1 + we2)
        y2 = prelu(acc2 * s2 + b2, slope).float()
        e2 = exp_from_max(float(y2.abs().max()))
        h, l = split(y2, e2)
        th, tw = min(TH, H - h0), min(TW, W - w0)
        own = slice(h0, h0 + th), slice(w0, w0 + tw)
        acc3 = _mm3(h, l, w3h[:, :64], w3l[:, :64], fault)[:th, :tw] * 2.0 ** -(e2 + we3)
        if proj:
            acc3 = acc3 + _mm3(xh[n][own], xl[n][own], w3h[:, 64:], w3l[:, 64:], fault) * 2.0 ** -(e_x + we3)
            o = acc3 * s3 + b3
        else:
            o = acc3 * s3 + (b3 + xf[n][own].double())
        out[n][own] = prelu(o, slope).float().double()
    return out


# ----------------------------------------------------------------------------- the case table
class BCase(NamedTuple):
    """A bottleneck launch.  ``th`` / ``rounds``: the tile height and the rounds of the launch its name claims (checked against the
    restated rule for 256 and 304 CUs).  ``x``: "randn" (PReLU-shaped randn), "bright" (one pixel 2^10 above the rest, on a tile border),
    "zero_tile" (tile (0, 1) and the ring round it exact zeros), "aligned" (rounding errors line up: see bottleneck_inputs).
    ``words_gain``: the range words hold this times the data's abs-max; ``static``: the static exponent instead of range words."""
    name: str
    N: int
    H: int
    W: int
    Cin: int
    Cout: int
    proj: bool
    slope: float = 0.25
    in_extra: int = 0
    out_extra: int = 0
    bn: str = "pos"
    x: str = "randn"
    gain: float = 1.0
    words_gain: float = 1.0
    static: Optional[int] = None
    shifts: bool = True
    th: int = 8
    rounds: int = 1

    @property
    def form(self):
        return "projection" if self.proj else "identity"


class SCase(NamedTuple):
    """A stem launch.  ``x``: "randn", "bright", "zero_image" (image 1 of the batch exact zeros), "copies" (every third image is
    image 0, the others randn at gains 2^(i mod 5)), "periodic" (rows repeat every 16: interior tiles see one patch)."""
    name: str
    N: int
    H: int
    W: int
    slope: float = 0.25
    out_extra: int = 0
    bn: str = "pos"
    x: str = "randn"
    gain: float = 1.0
    rounds: int = 1


def _both(name, N, H, W, cid=64, cproj=(64, 256), **kw):
    return (BCase(f"{name}/id{cid}", N, H, W, cid, cid, False, **kw),
            BCase(f"{name}/proj{cproj[0]}-{cproj[1]}", N, H, W, cproj[0], cproj[1], True, **kw))


def ten_row_case(cus: int, proj: bool) -> BCase:
    """``cus`` images of 19 x 5: three 8-row tiles or two 10-row tiles each - the 8-row tiling needs two rounds of the device
    (two workgroups per CU), the 10-row tiling one, and 2 x the 8-row wave's MFMAs exceed the 10-row wave's."""
    c = (64, 256) if proj else (64, 64)
    return BCase(f"ten-rows/{'proj64-256' if proj else 'id64'}", cus, 19, 5, c[0], c[1], proj, th=10)


def bottleneck_cases(cus: int) -> tuple:
    out = []
    for N, H, W in ((1, 1, 1), (1, 8, 16), (1, 9, 17), (1, 16, 32), (1, 8, 128), (1, 8, 144), (3, 5, 5), (2, 7, 15)):
        out += _both(f"geo-{N}x{H}x{W}", N, H, W)
    out += [ten_row_case(cus, False), ten_row_case(cus, True)]
    out += [BCase(f"chan/id{c}", 1, 9, 17, c, c, False) for c in (128, 256)]
    out += [BCase(f"chan/proj{a}-{b}", 1, 9, 17, a, b, True) for a, b in ((128, 64), (256, 128), (64, 192))]
    out += _both("pitch-in+8nan-out+12", 2, 7, 15, in_extra=8, out_extra=12)
    out += _both("bn-mixed-slope0", 1, 9, 17, bn="mixed", slope=0.0)
    out += _both("bn-mixed-slope1", 1, 9, 17, bn="mixed", slope=1.0)
    out += _both("gain-2^10", 1, 9, 17, gain=2.0 ** 10)
    out += _both("gain-2^-10", 1, 9, 17, gain=2.0 ** -10)
    out += _both("words-2^6-larger", 1, 9, 17, words_gain=2.0 ** 6)
    out += _both("bright-pixel", 1, 16, 32, x="bright")
    out += _both("zero-tile", 1, 16, 48, x="zero_tile", shifts=False)
    out += _both("zero-tile-shifts", 1, 16, 48, x="zero_tile")
    out += _both("static-exp-8", 2, 9, 17, static=8)
    out += _both("aligned", 1, 16, 32, x="aligned")
    return tuple(out)


def stem_rounds_cases(cus: int) -> tuple:
    col_h = 16 * (2 * cus + 2)                 # PH = 4 (2 cus + 2): that many tiles in one column
    return (SCase("rounds-2/images", 2 * cus + 1, 5, 6, x="copies", rounds=2),
            SCase("rounds-3/images", 4 * cus + 3, 5, 6, x="copies", rounds=3),
            SCase("rounds-2/column", 1, col_h, 3, x="periodic", rounds=2))


def stem_cases(cus: int) -> tuple:
    out = [SCase(f"geo-{N}x{H}x{W}", N, H, W) for N, H, W in ((1, 1, 1), (1, 15, 63), (1, 16, 64), (1, 17, 65), (2, 18, 66))]
    out += [SCase("pitch-out72", 1, 17, 65, out_extra=8),
            SCase("bn-mixed-slope0", 1, 17, 65, bn="mixed", slope=0.0),
            SCase("bn-mixed-slope1", 1, 17, 65, bn="mixed", slope=1.0),
            SCase("gain-2^10", 1, 17, 65, gain=2.0 ** 10),
            SCase("gain-2^-10", 1, 17, 65, gain=2.0 ** -10),
            SCase("bright-pixel", 1, 33, 130, x="bright"),
            SCase("zero-image", 3, 17, 65, x="zero_image")]
    return tuple(out) + stem_rounds_cases(cus)


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(repr(c._replace(name="")).encode()))


def _bn(g, n, mode, gain):
    s = torch.rand(n, generator=g) + 0.5
    if mode == "mixed":
        s = s * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        s[torch.arange(3, n, 19)] = 0.0
    b = torch.randn(n, generator=g) * 0.1 * gain
    return s, b


ALIGNED = 1.0 + 2.0 ** -11 - 2.0 ** -16   # 2^14 times it is 16384 + 7.75: the low fp16 piece (7.75, exact) is 0.97 * 2^-11 of the value


def bottleneck_inputs(c: BCase) -> dict:
    """CPU f32 operands of a case: x [N, H, W, Cin], w1, w2, w3, wd / bnd (projection), bn = [s1, b1, s2, b2, s3, b3], e_x.

    "aligned": every rounding error of conv2 has one sign - the worst case bar() is derived for.  x is zero but for channel 0 of
    the last 2 x 2 pixels of tile (0, 0), where four tiles meet; w1[:, 0] = 1, s1 = 1, b1 = ALIGNED: y1 = ALIGNED everywhere and
    exactly 0 on those four pixels, so the 3x3 window of the tile's corner pixel holds nothing but its five halo pixels.  w2 is ONE positive constant with the same significand, w3 (and the
    projection's wd, s3, sd) are positive, b2 = 0.  A missing low piece - of the weights or of the halo's y1 - is then an error of
    0.97 * 2^-11 of T there: nearly twice E."""
    g = _gen(c)
    Cin, Cout = c.Cin, c.Cout
    x = torch.randn(c.N, c.H, c.W, Cin, generator=g)
    x = torch.maximum(x, 0.25 * x) * c.gain
    w1 = torch.randn(64, Cin, generator=g) / math.sqrt(Cin)
    w2 = torch.randn(64, 3, 3, 64, generator=g) / 24.0
    w3 = torch.randn(Cout, 64, generator=g) / 8.0
    wd = torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin)
    (s1, b1), (s2, b2), (s3, b3), (sd, bd) = (_bn(g, n, c.bn, c.gain) for n in (64, 64, Cout, Cout))
    if not c.shifts:                                   # (b3 stays: a zero tile's output is PReLU(b3 + x))
        b1, b2 = torch.zeros(64), torch.zeros(64)
    if c.x == "bright":
        x[0, 3, 16] *= 2.0 ** 10             # (tile (0, 1)'s own pixel, and the pixel that sets tile (0, 0)'s y1 scale from its halo)
    elif c.x == "zero_tile":
        x[0, 0:9, 15:33] = 0.0
    elif c.x == "aligned":
        x.zero_()
        x[0, 6:8, 14:16, 0] = -ALIGNED
        w1[:, 0] = 1.0
        s1, b1 = torch.ones(64), torch.full((64,), ALIGNED)
        w2 = torch.full((64, 3, 3, 64), ALIGNED / 32.0)
        s2, b2 = s2.abs(), torch.zeros(64)
        w3, wd, s3, sd = w3.abs(), wd.abs(), s3.abs(), sd.abs()
    e_x = c.static if c.static is not None else exp_from_max(float(x.abs().max()) * c.words_gain)
    return dict(x=x, w1=w1, w2=w2, w3=w3, wd=wd if c.proj else None, bnd=(sd, bd) if c.proj else None,
                bn=[s1, b1, s2, b2, s3, b3], e_x=e_x, words_max=float(x.abs().max()) * c.words_gain)


def stem_inputs(c: SCase) -> dict:
    g = _gen(c)
    x = torch.randn(c.N, 3, c.H, c.W, generator=g) * c.gain
    if c.x == "bright":
        x[0, :, 20, 70] *= 2.0 ** 10
    elif c.x == "zero_image":
        x[1] = 0.0
    elif c.x == "copies":
        for i in range(c.N):
            x[i] = x[0] if i % 3 == 0 else x[i] * 2.0 ** (i % 5)
    elif c.x == "periodic":
        x = x[:, :, :16].repeat(1, 1, c.H // 16, 1)
    w = torch.randn(64, 3, 7, 7, generator=g) / math.sqrt(147)
    scale, shift = _bn(g, 64, c.bn, c.gain)
    return dict(x=x, w=w, scale=scale, shift=shift * 2.0)
