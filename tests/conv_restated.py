"""Float64 restatement of tsod_conv2d_dual_f32 (csrc/conv_igemm_f32.hip) in plain torch on the CPU, the error bars its three
arithmetics are held to, the host's launch rules restated (which gather path, which epilogue stores, which schedule a
(problem, tile) pair gets), and the case table of tests/test_conv_kernels_gpu.py.

Layouts are the library's own: the input is NHWC in a pixel of ``in_pitch`` floats, the contraction gathers the channel
segments ``segs`` = ((offset, length), ...) of it in that order, the weights are packed [Cout][KH][KW][Cin] (then the second
source's ``c2`` columns).  The restatement is a sum over filter taps of shifted, strided slices times one weight plane - no
call into torch's convolution - so that it can be checked against F.conv2d on a CPU-only machine and the kernels against it.

``conv_ref`` returns (y, T).  T is the same expression on absolute values, before the activation:
    T = |scale| conv(|x|, |w|) + |shift| + |residual|
and the pass condition of every GPU test is per element  |got - y| <= bar(arithmetic, K, S) T.

The bars.  u = 2^-24; K = contraction length; S = K-slices summed by the last arriver (1: a whole tile).
Two kinds of steps round:
  * a matrix-pipe accumulate step, counted as at most 2u of the running magnitude (the pipes' internal rounding is not
    documented as round-to-nearest); the running magnitude never exceeds conv(|x|, |w|) (1 + small);
  * a VALU step, at most u of its result's magnitude bound: the S - 1 slab adds, the scale multiply, the shift add, the
    residual add and PReLU's slope multiply: S - 1 + 4 steps, each on a value bounded by T (1 + small).
The activation is 1-Lipschitz for the slopes used (|slope| <= 1, ReLU, ReLU6), so it does not enlarge an error.

  f32      one accumulate step per k:                                             (2K + S + 4) u T     [S + 4 >= S - 1 + 4]
  bf16x3   hi + mid + lo == x exactly for the truncating split (the weights; the activations' round-to-nearest pieces leave
           at most 2^-27 |x|), piece products (8 x 8 significand bits) are exact in f32, six products per k are
           accumulated: 6K steps = 12K u.  The three dropped products: |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|, so
           mid*lo + lo*mid + lo*lo <= (2 + 2^-8) 2^-24 |a b|; with the split residuals (2 * 2^-27) that is < 3u |a b| per k,
           3u conv(|x|,|w|) in the sum:                                           (12K + 3 + S + 4) u T
  fp16x2   hi = rne16(s x), lo = rne16(s x - hi) with s a power of two (exact) and s x - hi exact in f32.
           |s x - hi| <= 2^-11 |s x|; when lo is a normal fp16, |s x - hi - lo| <= 2^-11 |s x - hi| <= 2^-22 |s x|; when
           it is subnormal the error is at most half the subnormal spacing, 2^-25.  2^-22 |s x| >= 2^-25 whenever
           |s x| >= 2^-3, so with m(x) = max(|x|, 2^-3 / s):  |x - (hi + lo) / s| <= 2^-22 m(x)  for EVERY x.
           Per k: the activation's residual times |w|, the weight's residual times |a| (1 + 2^-22) and the dropped
           |lo_a lo_w| <= 2^-22 |a w|: together < 3 * 2^-22 m(a) m(w) = 12u m(a) m(w).  Piece products (11 x 11 bits) are
           exact in f32, three are accumulated per k: 3K steps = 6K u:            (6K + 12 + S + 4) u T
           where for this arithmetic T is taken over the floored magnitudes m(x), m(w) (``floor_x``, ``floor_w`` of
           conv_ref: 2^-3 over the activation / weight scale), which is what makes the bar hold for values whose low piece
           is an fp16 subnormal.
Second-order terms ((1 + K u)^2 - 1 - 2 K u and the like) are covered by the factor 1.01: at the K <= 2052 of the case table
12 K u < 1.5e-3.

These are worst-case bars, linear in K.  They are only sharp at the small K used here (a wrong index is an error of order T,
10^4 bars away); at the K of real layers the sqrt(K) bars of tests/test_hip_ops.py (3e-6 sqrt(K) + 1e-5) are the useful ones
and stay as they are.
"""
import math
from typing import NamedTuple, Optional

import torch

U = 2.0 ** -24
ACT_NONE, ACT_PRELU, ACT_RELU6, ACT_RELU = 0, 1, 2, 3
F32, BF16X3, FP16X2 = 0, 1, 2
PREC_NAMES = {F32: "f32", BF16X3: "bf16x3", FP16X2: "fp16x2"}
SCHEDULES = (1, 2, 3, -1)            # desc.split_k every tile runs; the LDS-DMA tiles also run -2
FP16_FLOOR = 2.0 ** -3               # |s x| below which the low fp16 piece may be subnormal (module docstring)


def bar(prec: int, K: int, S: int = 1) -> float:
    """The factor of T an output may be off by: arithmetic ``prec``, contraction length K, S K-slices combined."""
    steps = {F32: 2 * K, BF16X3: 12 * K + 3, FP16X2: 6 * K + 12}[prec]
    return 1.01 * (steps + S + 4) * U


# ----------------------------------------------------------------------------- the cases
class Epi(NamedTuple):
    """An epilogue and where the output / residual live.  ``out_extra`` / ``res_extra``: floats the pixel is wider than Cout;
    ``out_shift`` / ``res_shift``: floats the base pointer sits past a 256-byte-aligned allocation; ``gain`` multiplies the
    activations (ReLU6: so that both clamps are reached)."""
    name: str = "plain"
    scale: bool = False
    shift: bool = False
    res: bool = False
    act: int = ACT_NONE
    slope: float = 0.0
    out_extra: int = 0
    out_off: int = 0
    res_extra: int = 0
    res_off: int = 0
    out_shift: int = 0
    res_shift: int = 0
    gain: float = 1.0


class Case(NamedTuple):
    name: str
    N: int
    H: int
    W: int
    in_pitch: int
    segs: tuple                       # ((channel offset, length), ...), contraction order
    Cout: int
    KH: int = 1
    KW: int = 1
    stride: int = 1
    pad_h: int = 0
    pad_w: int = 0
    src2: Optional[tuple] = None      # (c2, in2_pitch, in2_off, stride2, H2, W2)
    epi: Epi = Epi()
    border: bool = False              # image n is multiplied by 1000^n: a tap that leaks across an image border is gross

    @property
    def Cin(self):
        return sum(ln for _, ln in self.segs)

    @property
    def c2(self):
        return self.src2[0] if self.src2 else 0

    @property
    def K1(self):
        return self.KH * self.KW * self.Cin

    @property
    def K(self):
        return self.K1 + self.c2

    @property
    def OH(self):
        return (self.H + 2 * self.pad_h - self.KH) // self.stride + 1

    @property
    def OW(self):
        return (self.W + 2 * self.pad_w - self.KW) // self.stride + 1

    @property
    def M(self):
        return self.N * self.OH * self.OW

    @property
    def out_pitch(self):
        return self.Cout + self.epi.out_extra

    @property
    def res_pitch(self):
        return self.Cout + self.epi.res_extra


HARD_SEGS = ((40, 16), (8, 24), (64, 12))        # a HarDBlock's newest-first concat inside a pixel of 80 floats

G1 = Case("G1", 2, 5, 7, 32, ((0, 32),), 64, 3, 3, 1, 1, 1, border=True)
G3 = Case("G3", 2, 7, 5, 24, ((0, 24),), 54, 3, 3, 1, 0, 0, border=True)
FIXED_GEOMETRY = (
    G1,
    Case("G2", 3, 6, 8, 64, ((0, 64),), 68, 3, 3, 2, 1, 1, border=True),
    G3,
    Case("G4", 2, 4, 9, 80, HARD_SEGS, 20, 3, 3, 1, 1, 1, border=True),
    Case("G5", 2, 6, 9, 80, HARD_SEGS, 20, 3, 3, 2, 1, 1, border=True),
    Case("G6-2048", 1, 3, 5, 2064, ((1036, 1024), (4, 1024)), 8),
    Case("G6-2052", 1, 3, 5, 2064, ((1032, 1028), (4, 1024)), 8),
    Case("G7", 1, 1, 1, 32, ((0, 32),), 4, 3, 3, 1, 1, 1),
    Case("G8-1x3", 2, 5, 6, 40, ((4, 36),), 12, 1, 3, 1, 0, 1, border=True),
    Case("G8-3x1", 2, 5, 6, 40, ((4, 36),), 12, 3, 1, 1, 1, 0, border=True),
    Case("G8-3x3", 2, 5, 6, 40, ((4, 36),), 12, 3, 3, 1, 2, 0, border=True),
    Case("G9", 2, 7, 8, 40, ((0, 36),), 40, 1, 1, 2, 0, 0),
    # second source.  With C1 = c2 = 64 a 32-float tile has 4 K-steps: split_k = 2 cuts AT the seam and 3 resolves to the same
    # two slices (64-float tiles: one step per slice either way); only the 16-float LDS-DMA tiles cut beside it (48, 96).
    # G12-96 (C1 = c2 = 96, 6 steps of 32) puts split_k = 2 at 96 = the seam and 3 at 64 / 128 = beside it on the 32-float
    # tiles as well; the 64-float tiles refuse it (96 is no whole K-step).
    Case("G12", 2, 3, 4, 64, ((0, 64),), 68, src2=(64, 128, 32, 2, 6, 7)),
    Case("G12-96", 2, 3, 4, 96, ((0, 96),), 68, src2=(96, 128, 32, 2, 6, 7)),
)


def tile_geometry(bm: int, bn: int, bk: int) -> tuple:
    """G10 and G11: the cases whose extents are a tile's own (rows and columns exactly on a tile border and one past it; K of
    one 4-float chunk, and one chunk into a second K-step)."""
    out = []
    for m in (bm, bm + 1):
        for cout in (bn, bn + 4, bn + 1):
            out.append(Case(f"G10-{m}x{cout}", 1, 1, m, 32, ((0, 32),), cout))
    if bk > 32:                       # (32 channels are no whole K-step of these tiles - table path, or refused by the LDS-DMA one:
        #                               the one-past-the-border case again with two whole K-steps, so uniform and sliceable)
        for cout in (bn + 4, bn + 1):
            out.append(Case(f"G10-{bm + 1}x{cout}-cin{2 * bk}", 1, 1, bm + 1, 2 * bk, ((0, 2 * bk),), cout))
    for cin in (4, bk + 4):
        out.append(Case(f"G11-{cin}", 1, 3, 5, cin + 4, ((4, cin),), 8))
    return tuple(out)


EPILOGUES = (
    Epi("plain"),
    Epi("scale-shift", scale=True, shift=True),
    Epi("scale-shift-res8-prelu", scale=True, shift=True, res=True, act=ACT_PRELU, slope=0.25, res_extra=24, res_off=8),
    Epi("shift-relu6", shift=True, act=ACT_RELU6, gain=6.0),
    Epi("res-relu", res=True, act=ACT_RELU),
    Epi("out-off12", out_extra=32, out_off=12),
)
# every documented trigger of the scalar stores, each alone on G1's (otherwise vector) geometry
SCALAR_TRIGGERS = (
    Epi("out_off=2", scale=True, shift=True, out_extra=4, out_off=2),
    Epi("out_pitch%4=1", scale=True, shift=True, out_extra=5, out_off=0),
    Epi("res_pitch%4=1", scale=True, shift=True, res=True, res_extra=5, res_off=0),
    Epi("res_off=2", scale=True, shift=True, res=True, res_extra=4, res_off=2),
    Epi("out+4B", scale=True, shift=True, out_shift=1),
    Epi("res+4B", scale=True, shift=True, res=True, res_shift=1),
)


def epilogue_cases() -> tuple:
    out = []
    for g in (G1, G3):
        for e in EPILOGUES[1:]:                              # (plain is the geometry table's own G1 / G3)
            out.append(g._replace(name=f"{g.name}/{e.name}", epi=e))
    for e in SCALAR_TRIGGERS:
        out.append(G1._replace(name=f"G1/{e.name}", epi=e))
    return tuple(out)


def cases_for(tile: int) -> tuple:
    t = TILES[tile]
    return FIXED_GEOMETRY + tile_geometry(t.bm, t.bn, t.bk) + epilogue_cases()


# ----------------------------------------------------------------------------- the reference
def _f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def activation(v, act, slope=0.0):
    if act == ACT_NONE:
        return v
    if act == ACT_PRELU:
        return torch.where(v >= 0, v, v * slope)
    if act == ACT_RELU6:
        return v.clamp(0.0, 6.0)
    return v.clamp_min(0.0)


def gather_segments(x, segs):
    return torch.cat([x[..., o:o + ln] for o, ln in segs], dim=-1)


def _contract(xg, w, KH, KW, stride, pad_h, pad_w, OH, OW):
    """sum over taps of a shifted, strided slice [N,OH,OW,Cin] times the tap's weight plane [Cin,Cout]"""
    N, H, W, Cin = xg.shape
    xp = torch.zeros((N, H + 2 * pad_h, W + 2 * pad_w, Cin), dtype=torch.float64)
    xp[:, pad_h:pad_h + H, pad_w:pad_w + W] = xg
    acc = torch.zeros((N, OH, OW, w.shape[0]), dtype=torch.float64)
    for kh in range(KH):
        for kw in range(KW):
            v = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
            acc += v @ w[:, kh, kw, :].T
    return acc


def conv_ref(x, w, *, segs, KH=1, KW=1, stride=1, pad_h=0, pad_w=0, x2=None, c2=0, in2_off=0, stride2=1, scale=None, shift=None,
             residual=None, res_off=0, act=ACT_NONE, slope=0.0, floor_x=0.0, floor_w=0.0):
    """x [N,H,W,in_pitch], w [Cout, KH*KW*Cin + c2], x2 [N,H2,W2,in2_pitch] or None, scale / shift [Cout] or None, residual
    [N,OH,OW,res_pitch] or None (its channels [res_off, res_off + Cout) are added) -> (y, T), both f64 [N,OH,OW,Cout].
    ``floor_x`` / ``floor_w``: magnitudes below them count as them in T (the fp16x2 bar, module docstring)."""
    x, w = _f64(x), _f64(w)
    Cout = w.shape[0]
    xg = gather_segments(x, segs)
    N, H, W, Cin = xg.shape
    K1 = KH * KW * Cin
    OH, OW = (H + 2 * pad_h - KH) // stride + 1, (W + 2 * pad_w - KW) // stride + 1
    w1 = w[:, :K1].reshape(Cout, KH, KW, Cin)
    geo = (KH, KW, stride, pad_h, pad_w, OH, OW)
    y = _contract(xg, w1, *geo)
    # (the floor is applied before the zero padding: a padding tap is not an operand and adds nothing to T)
    T = _contract(xg.abs().clamp_min(floor_x), w1.abs().clamp_min(floor_w), *geo)
    if c2 > 0:
        v = _f64(x2)[:, 0:(OH - 1) * stride2 + 1:stride2, 0:(OW - 1) * stride2 + 1:stride2, in2_off:in2_off + c2]
        w2 = w[:, K1:K1 + c2]
        y = y + v @ w2.T
        T = T + v.abs().clamp_min(floor_x) @ w2.abs().clamp_min(floor_w).T
    if scale is not None:
        y, T = y * _f64(scale), T * _f64(scale).abs()
    if shift is not None:
        y, T = y + _f64(shift), T + _f64(shift).abs()
    if residual is not None:
        r = _f64(residual).reshape(N, OH, OW, -1)[..., res_off:res_off + Cout]
        y, T = y + r, T + r.abs()
    return activation(y, act, slope), T


# ----------------------------------------------------------------------------- the tile catalogue (kTiles)
class TileRow(NamedTuple):
    name: str
    bm: int
    bn: int
    bk: int
    nbuf: int
    resident: int
    dma: bool
    precs: tuple


_A, _F, _S, _B, _H = (F32, BF16X3, FP16X2), (F32,), (BF16X3, FP16X2), (BF16X3,), (FP16X2,)
TILES = {
    1: TileRow("128x128", 128, 128, 32, 2, 2, False, _F),
    2: TileRow("128x64", 128, 64, 32, 2, 2, False, _F),
    3: TileRow("64x64", 64, 64, 32, 2, 4, False, _A),
    4: TileRow("64x128", 64, 128, 32, 2, 2, False, _F),
    5: TileRow("128x128w8", 128, 128, 32, 2, 2, False, _F),
    6: TileRow("128x64w8", 128, 64, 32, 2, 2, False, _F),
    7: TileRow("256x128w8", 256, 128, 32, 2, 1, False, _F),
    8: TileRow("64x64s1", 64, 64, 32, 1, 6, False, _A),
    9: TileRow("128x64w8s1", 128, 64, 32, 1, 3, False, _A),
    10: TileRow("64x64s1k64", 64, 64, 64, 1, 4, False, _A),
    11: TileRow("128x64w8s1k64", 128, 64, 64, 1, 2, False, _F),
    12: TileRow("64x64w1s1", 64, 64, 32, 1, 8, False, _F),
    13: TileRow("128x64w2s1", 128, 64, 32, 1, 4, False, _F),
    14: TileRow("128x64s1", 128, 64, 32, 1, 4, False, _A),
    15: TileRow("64x128s1", 64, 128, 32, 1, 4, False, _A),
    16: TileRow("128x128s1", 128, 128, 32, 1, 2, False, _A),
    17: TileRow("d128x128", 128, 128, 16, 4, 2, True, _S),
    18: TileRow("d64x128", 64, 128, 32, 3, 1, True, _B),
    19: TileRow("d256x128", 256, 128, 16, 4, 1, True, _S),
    20: TileRow("d64x128s2", 64, 128, 32, 2, 2, True, _B),
    21: TileRow("d128x256", 128, 256, 16, 4, 1, True, _S),
    22: TileRow("d128x128k32", 128, 128, 32, 3, 1, True, _S),
    23: TileRow("d192x128", 192, 128, 16, 4, 1, True, _H),
    24: TileRow("d64x128k64", 64, 128, 64, 3, 1, True, _H),
}
PAIRS = tuple((p, t) for p in (F32, BF16X3, FP16X2) for t, row in TILES.items() if p in row.precs)
CHAN_TAB = 512                      # kChanTab: 4-float chunks the pointwise table holds (K <= 2048)
DMA_TAB_ENTRIES = 640               # kDmaTabEntries
TICKET_BYTES = 256 * 1024           # kTicketBytes
FALLBACK_CUS = 256                  # cu_count() without a device


def residency(tile: int, prec: int) -> int:
    """Workgroups per CU: the catalogue's figure, for the split arithmetics capped by 160 KB over their LDS footprint (three
    planes per operand; the LDS-DMA tiles: ring stages of an f32 activation block and three bf16 weight planes)."""
    t = TILES[tile]
    if prec == F32:
        return t.resident
    lds = t.nbuf * (t.bm * t.bk * 4 + 3 * t.bn * t.bk * 2) if t.dma else t.nbuf * 3 * (t.bm + t.bn) * (t.bk // 2) * 4
    fit = 160 * 1024 // lds
    return max(fit, 1) if fit < t.resident else t.resident


def _dma_chan_case(c: Case, prec: int) -> bool:
    return (prec == FP16X2 and len(c.segs) > 1 and c.KH == 1 and c.KW == 1 and c.stride == 1 and c.pad_h == 0 and c.pad_w == 0
            and c.c2 == 0)


def gather_path(c: Case, tile: int, prec: int = F32) -> str:
    """Which address path the host gives (problem, tile): "uniform" (one segment, Cin a multiple of the K-step: tap and channel
    base on the scalar unit), "table" (1x1, stride 1, unpadded, K <= 2048: chunk offsets from an LDS table), "generic" (the
    reciprocal split + the segment select chain), "dma" / "dma_chan" (the LDS-DMA kernel's tap form / its fp16x2 multi-segment
    1x1 form), or "unsupported" (the call returns TSOD_ERR_UNSUPPORTED)."""
    t = TILES[tile]
    if c.c2 > 0 and not (len(c.segs) == 1 and c.K1 % 32 == 0 and c.Cin % 32 == 0):
        return "unsupported"                                      # validate: K-steps must not straddle the two sources
    if t.dma:
        if _dma_chan_case(c, prec):
            return "dma_chan" if c.K <= 2048 and c.K // t.bk + 9 <= DMA_TAB_ENTRIES else "unsupported"
        ok = (len(c.segs) == 1 and c.Cin % t.bk == 0 and (c.c2 == 0 or c.c2 % t.bk == 0) and c.KH * c.KW <= 31
              and c.K // t.bk + 8 <= DMA_TAB_ENTRIES)
        return "dma" if ok else "unsupported"
    uniform = len(c.segs) == 1 and c.Cin % t.bk == 0
    if c.c2 > 0:
        return "uniform" if uniform and c.K1 % t.bk == 0 and c.c2 % t.bk == 0 else "unsupported"
    if uniform:
        return "uniform"
    if c.KH == 1 and c.KW == 1 and c.pad_h == 0 and c.pad_w == 0 and c.stride == 1 and c.K <= 4 * CHAN_TAB:
        return "table"
    return "generic"


def epilogue_path(c: Case) -> str:
    """ "vec" (dwordx4 stores) or "scalar".  The single statement of the host's rule for the tests; vector needs ALL of:

        Cout % 4 == 0            out_pitch % 4 == 0           out_off % 4 == 0           out 16-byte aligned
        and with a residual:     res_pitch % 4 == 0           res_off % 4 == 0           residual 16-byte aligned

    (scale / shift 16-byte aligned as well; the tests keep them at the allocator's alignment).  Scalar triggers in the table:

        Cout = 54, bn + 1        G3, G10             out_off = 2            G1/out_off=2
        out_pitch % 4 = 1        G1/out_pitch%4=1    res_pitch % 4 = 1      G1/res_pitch%4=1
        res_off = 2              G1/res_off=2        out base + 4 bytes     G1/out+4B
        residual base + 4 bytes  G1/res+4B
    """
    e = c.epi
    vec = ((c.Cout | c.out_pitch | e.out_off) & 3) == 0 and e.out_shift % 4 == 0
    if e.res:
        vec = vec and ((c.res_pitch | e.res_off) & 3) == 0 and e.res_shift % 4 == 0
    return "vec" if vec else "scalar"


class Sched(NamedTuple):
    tiles_m: int
    tiles_n: int
    tiles: int
    dp_tiles: int                    # whole tiles
    split: int                       # K-slices of each of the other tiles
    kps: int
    grid: int
    ws_bytes: int

    @property
    def rem_tiles(self):
        return self.tiles - self.dp_tiles

    @property
    def reported_split_k(self):      # what tsod_conv2d_resolve hands back
        return 1 if self.rem_tiles == 0 else (self.split if self.dp_tiles == 0 else -1)

    @property
    def bodies(self):                # the epilogue bodies the launch runs
        return (("whole",) if self.dp_tiles else ()) + (("combine",) if self.rem_tiles else ())


def make_sched(c: Case, tile: int, prec: int, mode: int, cus: int = FALLBACK_CUS) -> Sched:
    """make_sched's uniform branch: mode 1 = whole tiles, S > 1 = every tile in S K-slices, -1 = hybrid."""
    assert mode >= 1 or mode == -1
    t = TILES[tile]
    ksteps = -(-c.K // t.bk)
    tiles_m, tiles_n = -(-c.M // t.bm), -(-c.Cout // t.bn)
    tiles = tiles_m * tiles_n
    slots = cus * residency(tile, prec)
    split, dp = 1, tiles
    if mode > 1:
        split, dp = min(mode, ksteps), 0
    elif mode == -1:
        full = tiles // slots * slots
        rem = tiles - full
        if rem > 0:
            split = max(min(slots // rem, ksteps // 2), 1)
            if split > 1:
                dp = full
    kps = -(-ksteps // split)
    split = -(-ksteps // kps)
    if split <= 1 or (tiles - dp) * 4 > TICKET_BYTES:
        split, dp, kps = 1, tiles, ksteps
    rem_tiles = tiles - dp
    ws = (TICKET_BYTES if rem_tiles else 0) + rem_tiles * split * t.bm * t.bn * 4
    return Sched(tiles_m, tiles_n, tiles, dp, split, kps, dp + rem_tiles * split, ws)


def hybrid_case(tile: int, prec: int, cus: int) -> Case:
    """A 1x1 conv with K = 128 and a few more tiles than the chip has slots for, so that split_k = -1 launches whole tiles AND
    K-sliced tiles in one grid (a partial last row tile, a partial second channel tile)."""
    t = TILES[tile]
    cout = t.bn + 8
    tiles_m = cus * residency(tile, prec) // 2 + 1
    m = tiles_m * t.bm - 3
    return Case(f"hybrid-{m}", 1, 1, m, 128, ((0, 128),), cout)


def schedules_for(tile: int) -> tuple:
    return SCHEDULES + ((-2,) if TILES[tile].dma else ())


def runs(c: Case, tile: int, prec: int, mode: int) -> bool:
    """Whether (problem, tile, arithmetic, schedule) launches; everything else is TSOD_ERR_UNSUPPORTED."""
    path = gather_path(c, tile, prec)
    if path == "unsupported":
        return False
    if mode == -2:                                                # balanced K ranges: the LDS-DMA tap form only
        return path == "dma" and TILES[tile].dma
    return True


def predicted_runs(tile: int, prec: int) -> int:
    return sum(runs(c, tile, prec, m) for c in cases_for(tile) for m in schedules_for(tile))


# ----------------------------------------------------------------------------- the reciprocal split (load_global)
def reciprocal_split_mismatches(cin: int, limit: int = 1 << 21) -> int:
    """k -> k // cin as the kernel does it, (int)((k + 0.5f) * (1.0f / cin)) in float32, at k = q cin - 4, q cin, q cin + 4 for
    every such k below ``limit``: the number of k where it differs from the integer division."""
    import numpy as np
    inv = np.float32(1.0) / np.float32(cin)
    q = np.arange(0, limit // cin + 2, dtype=np.int64) * cin
    k = np.concatenate([q - 4, q, q + 4])
    k = k[(k >= 0) & (k < limit)]
    seg = ((k.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)
    return int((seg != k // cin).sum())


def fp16x2_exponents(x_max: float, w_max: float) -> tuple:
    """(a_scale_exp, w_scale_exp): the powers of two that bring the largest activation / weight just below 2^14."""
    def e(m, lo, hi):
        return 0 if m == 0.0 or not math.isfinite(m) else max(lo, min(hi, int(math.floor(math.log2(16384.0 / m)))))
    return e(x_max, -24, 24), e(w_max, -40, 40)
