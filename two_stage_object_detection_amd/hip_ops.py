"""Tensor-level wrappers over the C ABI (one per entry point of include/tsod.h).

Every function takes CUDA/ROCm f32 tensors, allocates outputs with torch (device memory plumbing
only) and launches the HIP kernel on torch's current stream.  No fallback of any kind.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import threading
from ctypes import byref, c_int32

import torch
from torch.autograd.function import once_differentiable

from . import _ffi
from ._ffi import ACT_NONE, TsodError, check, lib, make_conv_desc, ptr, require_cuda, stream_ptr


# ----------------------------------------------------------------------------- workspace arena
class _Arena:
    """Growable scratch tensors (split-K slabs of the RPN / head GEMMs, NMS masks).

    Keyed by an explicit OWNER when one is in scope (``with ARENA.scope(owner)``: the detector enters one per
    (model, in-flight slot), so two slots or two detectors never share scratch whatever streams their graphs are
    replayed on), else by (device, current stream): stand-alone eager calls on one stream are ordered by that stream,
    and torch handing the same handle out twice means it IS the same HIP stream.
    A buffer that has been handed out is never freed or replaced under a HIP graph that may have its pointer baked in:
    outgrown buffers are retired, not released (``release(owner)`` drops an owner's buffers explicitly)."""

    def __init__(self, zero: bool = False):
        self._buf = {}
        self._retired = {}
        self._zero = zero            # conv workspaces start with arrival tickets that must be zero when first used

    def _key(self, device):
        owner = getattr(_OWNER_TLS, "owner", None)
        if owner is not None:
            return (device, "owner", owner)
        return (device, "stream", torch.cuda.current_stream(device).cuda_stream)

    def get(self, device, nbytes: int) -> torch.Tensor:
        nbytes = max(int(nbytes), 256)
        key = self._key(device)
        cur = self._buf.get(key)
        if cur is None or cur.numel() < nbytes:
            if cur is not None:
                self._retired.setdefault(key, []).append(cur)
            alloc = torch.zeros if self._zero else torch.empty
            cur = alloc(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
            self._buf[key] = cur
        return cur

    def release(self, owner) -> None:
        """Drop every buffer of ``owner`` (only once no graph captured under that owner will be replayed again)."""
        for key in [k for k in self._buf if k[1] == "owner" and k[2] == owner]:
            self._buf.pop(key, None)
            self._retired.pop(key, None)

    def scope(self, owner):                                   # both arenas share one owner scope
        return _owner_scope(owner)


_OWNER_TLS = threading.local()


@contextlib.contextmanager
def _owner_scope(owner):
    prev = getattr(_OWNER_TLS, "owner", None)
    _OWNER_TLS.owner = owner
    try:
        yield
    finally:
        _OWNER_TLS.owner = prev


ARENA = _Arena()
# K-sliced GEMM workspaces (tsod_conv2d_f32 / tsod_linear_f32): [arrival tickets | partial slabs].  The tickets must be
# zero when a launch starts and every launch leaves them zero, so these buffers are zero-filled once at allocation and
# never lent to any other kernel (the NMS masks live in ARENA).
CONV_ARENA = _Arena(zero=True)
TOPK_ARENA = _Arena()           # the selection handed from the top-k's select pass to its rank pass


# ----------------------------------------------------------------------------- layout
def nchw_to_nhwc(x: torch.Tensor, c_pad: int | None = None) -> torch.Tensor:
    """[N,C,H,W] -> [N,H,W,c_pad] (channels >= C zero-filled)."""
    require_cuda(x, "nchw_to_nhwc")
    x = x.contiguous()
    N, C, H, W = x.shape
    c_pad = C if c_pad is None else c_pad
    out = torch.empty((N, H, W, c_pad), dtype=torch.float32, device=x.device)
    check(lib().tsod_nchw_to_nhwc_f32(ptr(x), N, C, H, W, ptr(out), c_pad, c_pad, stream_ptr()), "nchw_to_nhwc")
    return out


def nhwc_to_nchw(x: torch.Tensor, C: int | None = None, c_off: int = 0) -> torch.Tensor:
    """[N,H,W,P] (channel slice [c_off, c_off+C)) -> [N,C,H,W]."""
    require_cuda(x, "nhwc_to_nchw")
    assert x.is_contiguous()
    N, H, W, P = x.shape
    C = P - c_off if C is None else C
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    check(lib().tsod_nhwc_to_nchw_f32(ptr(x), N, C, H, W, P, c_off, ptr(out), stream_ptr()), "nhwc_to_nchw")
    return out


# ----------------------------------------------------------------------------- conv / linear
def pack_conv_weight(w: torch.Tensor, cin_pad: int | None = None, kw_pad: int | None = None) -> torch.Tensor:
    """torch [Cout,Cin,KH,KW] -> packed [Cout,KH,KW_pad,Cin_pad] on the device (zero-filled padding)."""
    require_cuda(w, "pack_conv_weight")
    w = w.detach().contiguous()
    Cout, Cin, KH, KW = w.shape
    cin_pad = Cin if cin_pad is None else cin_pad
    kw_pad = KW if kw_pad is None else kw_pad
    out = torch.empty((Cout, KH, kw_pad, cin_pad), dtype=torch.float32, device=w.device)
    check(lib().tsod_pack_conv_weight_f32(ptr(w), Cout, Cin, KH, KW, cin_pad, kw_pad, ptr(out), stream_ptr()),
          "pack_conv_weight")
    return out


def pack_conv_weight_bf16x3(w_packed: torch.Tensor) -> torch.Tensor:
    """f32 packed weights [Cout,KH,KW,Cin] -> the pre-split bf16x3 image tsod_conv2d_f32 reads with precision = bf16x3
    (uint8 tensor of tsod_conv_weight_bf16x3_bytes: [Cout][ceil(K/8)][hi|mid|lo][8] bf16)."""
    require_cuda(w_packed, "pack_conv_weight_bf16x3")
    w_packed = w_packed.contiguous()
    cout = w_packed.shape[0]
    K = w_packed.numel() // cout
    out = torch.empty(lib().tsod_conv_weight_bf16x3_bytes(cout, K), dtype=torch.uint8, device=w_packed.device)
    check(lib().tsod_pack_conv_weight_bf16x3(ptr(w_packed), cout, K, ptr(out), stream_ptr()), "pack_conv_weight_bf16x3")
    return out


def fp16x2_weight_scale_exp(w_packed: torch.Tensor) -> int:
    """The power of two that brings max |w| just below 2^14 (fp16's largest finite value is 65504; the low pieces of weights
    scaled like this stay out of its subnormals): the ``w_scale_exp`` of pack_conv_weight_fp16x2 and of the conv descriptor."""
    m = float(w_packed.abs().max())
    return 0 if m == 0.0 or not math.isfinite(m) else max(-40, min(40, int(math.floor(math.log2(16384.0 / m)))))


def pack_conv_weight_fp16x2(w_packed: torch.Tensor, w_scale_exp: int) -> torch.Tensor:
    """f32 packed weights [Cout,KH,KW,Cin] -> the fp16x2 image tsod_conv2d_f32 reads with precision = fp16x2
    (uint8 tensor of tsod_conv_weight_fp16x2_bytes: [Cout][ceil(K/8)][hi|lo][8] fp16 of 2^w_scale_exp * w)."""
    require_cuda(w_packed, "pack_conv_weight_fp16x2")
    w_packed = w_packed.contiguous()
    cout = w_packed.shape[0]
    K = w_packed.numel() // cout
    out = torch.empty(lib().tsod_conv_weight_fp16x2_bytes(cout, K), dtype=torch.uint8, device=w_packed.device)
    check(lib().tsod_pack_conv_weight_fp16x2(ptr(w_packed), cout, K, int(w_scale_exp), ptr(out), stream_ptr()), "pack_conv_weight_fp16x2")
    return out


_W3_CACHE: dict = {}


def _w3_for(w_packed: torch.Tensor) -> torch.Tensor:
    """Pre-split image of a weight tensor for the tensor-level wrapper when the caller did not bring one (``w3=`` of
    conv2d_nhwc; the engine, the RPN and the RoI head keep theirs beside the packed f32 weights).
    Cached per (storage address, shape, version counter); the entry holds the tensor's BASE strongly, so the address cannot be
    handed to another tensor while the entry lives, and a fresh ``w.view(...)`` of the same weights (a new Python object on
    every call) hits.  Inference tensors carry no version counter - an in-place edit would be invisible - so they are
    never cached: packed on every call (correct, slower; bring ``w3=`` on a hot path)."""
    if w_packed.is_inference():
        return pack_conv_weight_bf16x3(w_packed)
    key = (w_packed.data_ptr(), tuple(w_packed.shape), w_packed._version)
    hit = _W3_CACHE.get(key)
    if hit is None:
        if len(_W3_CACHE) >= 64:
            _W3_CACHE.clear()
        base = w_packed._base if w_packed._base is not None else w_packed
        from .engine import _publish
        hit = _W3_CACHE[key] = (base, _publish(pack_conv_weight_bf16x3(w_packed)))
    return hit[1]


def conv2d_nhwc(x: torch.Tensor, w_packed: torch.Tensor, *, stride=1, pad=0, kw_logical=None, scale=None, shift=None,
                residual=None, act=ACT_NONE, slope=0.0, segs=None, out=None, out_off=0, tile=0, split_k=0,
                precision=0, x2=None, stride2=1, x2_off=0, w3=None, a_scale_exp=4, w2=None, w_scale_exp=None,
                range_flag=None, amax_in=None, amax_in2=None, amax_out=None) -> torch.Tensor:
    """Implicit-GEMM convolution on an NHWC tensor [N,H,W,P].  ``w_packed`` is [Cout,KH,KW,Cin]
    (see pack_conv_weight); ``kw_logical`` is the filter width before zero-tap padding (it fixes OW).
    ``segs`` = [(channel offset, length), ...] inside the P-wide pixel (default: the first Cin
    channels).  Returns / fills an NHWC output [N,OH,OW,Pout].
    ``x2`` [N,H2,W2,P2] is the optional second source of tsod_conv2d_dual_f32: ``w_packed`` is then [Cout, K1 + C2] with the
    last C2 columns contracting channels [x2_off, x2_off + C2) of pixel (oh*stride2, ow*stride2) of ``x2`` (``kernel`` =
    (KH, KW, Cin) of the first source must be given through ``segs`` / a 1x1 filter: only 1x1 first sources here).
    ``w3``: the pre-split bf16x3 image of ``w_packed`` (pack_conv_weight_bf16x3) when the caller keeps one; used with
    ``precision`` = bf16x3 instead of the wrapper's own cache.  ``precision`` = fp16x2: activations are split as
    2^``a_scale_exp`` * x (|that| must stay below 65504), ``w2`` / ``w_scale_exp`` = the fp16x2 weight image and the exponent it
    was packed with (made on the spot from ``w_packed`` when not given); ``range_flag``: an int32 device word the launch sets to 1
    when an activation left that range.  ``amax_out`` / ``amax_in`` / ``amax_in2``: range words (``new_amax_words``; a tensor or
    a raw device pointer): the launch adds its outputs' abs-max to ``amax_out``; an fp16x2 launch takes its activation exponent
    from ``amax_in`` (and ``amax_in2`` for ``x2``) instead of ``a_scale_exp``."""
    require_cuda(x, "conv2d")
    assert x.is_contiguous() and w_packed.is_contiguous()
    N, H, W, P = x.shape
    src2 = None
    if x2 is not None:                         # stacked [Cout, Cin1 + C2] weights of a 1x1 conv + a strided 1x1 tap of x2
        assert w_packed.dim() == 2 and x2.is_contiguous() and segs is not None and len(segs) == 1
        Cout, KH, KW, Cin = w_packed.shape[0], 1, 1, segs[0][1]
        src2 = (w_packed.shape[1] - Cin, x2.shape[3], x2_off, stride2, x2.shape[1], x2.shape[2])
    else:
        Cout, KH, KW, Cin = w_packed.shape
    segs = [(0, Cin)] if segs is None else segs
    assert sum(s[1] for s in segs) == Cin, "segments must add up to the packed Cin"
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - (KW if kw_logical is None else kw_logical)) // stride + 1
    if out is None:
        out = torch.empty((N, OH, OW, Cout), dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and out.shape[:3] == (N, OH, OW)
    d = make_conv_desc(N=N, H=H, W=W, in_pitch=P, segs=segs, Cout=Cout, out_pitch=out.shape[3], out_off=out_off,
                       KH=KH, KW=KW, stride=stride, pad_h=pad, pad_w=pad, OH=OH, OW=OW, act=act, slope=slope,
                       res_pitch=0 if residual is None else residual.shape[-1], res_off=0, tile=tile, split_k=split_k,
                       precision=precision, src2=src2)
    if precision == _ffi.PREC_FP16X2:
        if w2 is None:
            w_scale_exp = fp16x2_weight_scale_exp(w_packed)
            w2 = pack_conv_weight_fp16x2(w_packed, w_scale_exp)
        d.a_scale_exp, d.w_scale_exp = int(a_scale_exp), int(w_scale_exp)
        d.range_flag = ptr(range_flag)                            # optional int32 [1] device tensor: 1 = an activation left the range
        d.amax_in, d.amax_in2 = _word_ptr(amax_in), _word_ptr(amax_in2)
    d.amax_out = _word_ptr(amax_out)
    ws_bytes = lib().tsod_conv2d_workspace_bytes(byref(d))
    ws = CONV_ARENA.get(x.device, ws_bytes) if ws_bytes else None
    # bf16x3 / fp16x2 read their pre-split weight images
    w_arg = (w3 if w3 is not None else _w3_for(w_packed)) if precision == _ffi.PREC_BF16X3 else (w2 if precision == _ffi.PREC_FP16X2 else w_packed)
    check(lib().tsod_conv2d_dual_f32(byref(d), ptr(x), ptr(x2), ptr(w_arg), ptr(scale), ptr(shift), ptr(residual), ptr(out),
                                     ptr(ws), ws_bytes, stream_ptr()), "conv2d")
    return out


def pack_bottleneck_wstream(w1: torch.Tensor, w2: torch.Tensor, w3: torch.Tensor, projection: bool = False):
    """The weight stream of tsod_bottleneck_fp16x2 (include/tsod.h): w1 [64, Cin], w2 [64, 3, 3, 64] (packed conv layout:
    [Cout][KH][KW][Cin]), w3 [Cout, 64], f32 -> (uint8 tensor of tsod_bottleneck_wstream_bytes, (e1, e2, e3)).
    ``projection``: w3 is the stacked [Cout, 64 + Cin] matrix [W3 s3 | Wd sd] of desc.projection == 1 (2 + Cin / 32 steps per 64
    output channels, one exponent for the whole matrix).
    Pure index arithmetic on the three matrices (done once per model; the fp16 roundings are torch's round-to-nearest-even,
    the same bits as the device's v_cvt_pk_f16_f32).  A step (64 output channels x 32 k) is stored as the MFMA fragments the
    kernel's lanes load: [channel block cb (2)][lane (64) = 32 hh + j][chunk c (2)][hi | lo][8 k] fp16, where lane (j, hh) holds
    output channel 32 cb + pi(j) and k = 16 c + 8 hh .. + 7."""
    dev = w1.device
    cin, cout = w1.shape[1], w3.shape[0]
    i = torch.arange(32)
    pi = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3)
    rows = torch.cat([pi, 32 + pi]).to(dev)                                 # fragment row 32 cb + j  <-  channel 32 cb + pi(j)

    def steps(w2d, e):
        """w2d [n_rows (multiple of 64), K (multiple of 32)] -> [n_rows/64 * K/32 steps, 8192 bytes], row-block-major then k"""
        sc = w2d.float() * (2.0 ** e)
        hi = sc.half()
        lo = (sc - hi.float()).half()
        nb, ks = sc.shape[0] // 64, sc.shape[1] // 32
        # [nb, cb, j, ks, c, hh, 8] for each plane
        pl = torch.stack([t.view(nb, 64, ks, 2, 2, 8)[:, rows].view(nb, 2, 32, ks, 2, 2, 8) for t in (hi, lo)], dim=0)   # [plane, nb, cb, j, ks, c, hh, 8]
        # -> [nb, ks, cb, hh, j, c, plane, 8]
        out = pl.permute(1, 4, 2, 6, 3, 5, 0, 7).contiguous()
        return out.view(nb * ks, 64 * 64).view(torch.uint8)                  # 4096 halves = 8192 bytes per step

    e1, e2, e3 = (fp16x2_weight_scale_exp(w) for w in (w1, w2, w3))
    s1 = steps(w1.reshape(64, cin), e1)
    # conv2: step = (tap, channel half): K order of the packed layout is (kh, kw, ci), so k = 32 * (2 tap + half) already
    s2 = steps(w2.reshape(64, 9 * 64), e2)
    s3 = steps(w3.reshape(cout, 64 + cin if projection else 64), e3)         # row blocks of 64 output channels, 2 (+ Cin / 32) k-steps each
    stream = torch.cat([s1, s2, s3], dim=0).contiguous().view(-1)
    assert stream.numel() == (lib().tsod_bottleneck_proj_wstream_bytes if projection else lib().tsod_bottleneck_wstream_bytes)(cin, cout)
    return stream, (e1, e2, e3)


def bottleneck_fused(x: torch.Tensor, wstream: torch.Tensor, w_exps, bn: torch.Tensor, cout: int, slope: float, *, out=None,
                     a_scale_exp=4, amax_in=None, amax_out=None, range_flag=None, cin=None) -> torch.Tensor:
    """tsod_bottleneck_fp16x2 on an NHWC tensor x [N,H,W,P] (channels [0, cout) are the block's input; ``cin``: the projection
    form, channels [0, cin) in, cout out): see include/tsod.h."""
    require_cuda(x, "bottleneck_fused")
    N, H, W, P = x.shape
    if out is None:
        out = torch.empty((N, H, W, cout), dtype=torch.float32, device=x.device)
    d = _ffi.make_bottleneck_desc(N=N, H=H, W=W, Cin=cout if cin is None else cin, in_pitch=P, Cout=cout, out_pitch=out.shape[3],
                                  slope=slope, w_exps=w_exps, projection=cin is not None, a_scale_exp=a_scale_exp,
                                  range_flag=ptr(range_flag), amax_in=_word_ptr(amax_in), amax_out=_word_ptr(amax_out))
    check(lib().tsod_bottleneck_fp16x2(byref(d), ptr(x), ptr(wstream), ptr(bn), ptr(out), stream_ptr()), "bottleneck_fused")
    return out


def pack_stem_wfrag(w: torch.Tensor):
    """The weight fragments of tsod_stem_fp16x2 (include/tsod.h): conv1's weight [64, 3, 7, 7] f32 -> (uint8 tensor of
    tsod_stem_wfrag_bytes, w_exp).  K = (kh, kw padded to 8, ci padded to 4) = 224; [channel block cb (2)][chunk c (14)][hi | lo]
    [lane (64) = 32 hh + j][8 k] fp16, lane (j, hh) holding output channel 32 cb + pi(j) and k = 16 c + 8 hh .. + 7.  Index
    arithmetic only; the fp16 roundings are torch's round-to-nearest-even (the bits of the device's conversions)."""
    assert tuple(w.shape) == (64, 3, 7, 7), tuple(w.shape)
    dev = w.device
    e = fp16x2_weight_scale_exp(w)
    wk = torch.zeros((64, 7, 8, 4), dtype=torch.float32, device=dev)
    wk[:, :, :7, :3] = w.detach().float().permute(0, 2, 3, 1)
    sc = wk.reshape(64, 224) * (2.0 ** e)
    hi = sc.half()
    lo = (sc - hi.float()).half()
    i = torch.arange(32)
    pi = (16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3)).to(dev)
    pl = torch.stack([hi, lo], dim=0).view(2, 2, 32, 14, 2, 8)[:, :, pi]     # [plane, cb, j, c, hh, 8]: row j <- channel 32 cb + pi(j)
    out = pl.permute(1, 3, 0, 4, 2, 5).contiguous().view(-1).view(torch.uint8)   # [cb, c, plane, hh, j, 8]
    assert out.numel() == lib().tsod_stem_wfrag_bytes()
    return out, e


def stem_fused(x, wfrag: torch.Tensor, w_exp: int, bn: torch.Tensor, slope: float, *, out=None, amax_out=None, range_flag=None):
    """tsod_stem_fp16x2: conv1 7x7/2 + BN + PReLU + max pool 3x3/2 of ResNet in one launch.  ``x``: an NCHW tensor [N,3,H,W] or
    ``NHWC4Images``; returns the pooled NHWC map [N,PH,PW,64]."""
    nhwc4 = isinstance(x, _ffi.NHWC4Images)
    t = x.data if nhwc4 else x.contiguous()
    require_cuda(t, "stem_fused")
    if nhwc4:
        N, H, W, _ = t.shape
    else:
        N, _, H, W = t.shape
    _, _, ph, pw = _ffi.stem_out_hw(H, W)
    if out is None:
        out = torch.empty((N, ph, pw, 64), dtype=torch.float32, device=t.device)
    d = _ffi.make_stem_desc(N=N, H=H, W=W, in_layout=_ffi.STEM_NHWC4 if nhwc4 else _ffi.STEM_NCHW, out_pitch=out.shape[3],
                            slope=slope, w_exp=w_exp, range_flag=ptr(range_flag), amax_out=_word_ptr(amax_out))
    check(lib().tsod_stem_fp16x2(byref(d), ptr(t), ptr(wfrag), ptr(bn), ptr(out), stream_ptr()), "stem_fused")
    return out


def _word_ptr(w):
    """None / a raw device pointer / a tensor of range words -> what the descriptor takes."""
    if w is None:
        return None
    return (int(w) if not isinstance(w, torch.Tensor) else w.data_ptr()) or None


def new_amax_words(device, n: int = 1) -> torch.Tensor:
    """Zeroed range words for ``n`` tensors (include/tsod.h "Range words"): int32 [n, AMAX_BYTES / 4]; row i is one tensor's."""
    return torch.zeros((n, _ffi.AMAX_BYTES // 4), dtype=torch.int32, device=device)


def amax_value(words: torch.Tensor) -> float:
    """The abs-max a set of range words holds (host read; tests and diagnostics)."""
    w = words.reshape(-1)[:: _ffi.AMAX_STRIDE // 4][: _ffi.AMAX_WORDS]
    return float(w.max().view(1).view(torch.float32))


def absmax(x: torch.Tensor, words: torch.Tensor) -> torch.Tensor:
    """Add the abs-max of ``x`` to ``words`` (tsod_absmax_f32)."""
    require_cuda(x, "absmax")
    check(lib().tsod_absmax_f32(ptr(x), x.numel(), ptr(words), stream_ptr()), "absmax")
    return words


def tune_conv(x: torch.Tensor, w_packed: torch.Tensor, reps: int = 5, precisions=(0, 1), **kw) -> tuple[int, int, int]:
    """Time every (tile, K-slice schedule, arithmetic) of ONE conv2d_nhwc call on its real operands with HIP events and return
    the fastest as (tile, split_k, precision) - for the few GEMMs outside a backbone plan (the fused RPN conv, the fused head
    GEMM).  A speed choice only: every candidate is f32-accurate.  Precision 2 (fp16x2) among ``precisions`` needs ``w2`` /
    ``w_scale_exp`` and - for a range-proof scale - ``amax_in`` in ``kw`` (they are ignored by the other arithmetics)."""
    K = w_packed.numel() // w_packed.shape[0]
    ksteps = (K + 31) // 32
    best = None
    for prec in precisions:
        for tile in _ffi.tile_ids(prec):
            for split in (1, -1, -2, 2, 3, 4, 6, 8, 12, 16, 24, 32):
                if split > 1 and ksteps // split < 2:
                    continue
                try:
                    conv2d_nhwc(x, w_packed, tile=tile, split_k=split, precision=prec, **kw)          # warm (and validity)
                except _ffi.TsodError:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    conv2d_nhwc(x, w_packed, tile=tile, split_k=split, precision=prec, **kw)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1) / reps
                if best is None or t < best[0]:
                    best = (t, tile, split, prec)
    return best[1], best[2], best[3]


def conv2d_resolve(d) -> tuple[int, int]:
    t, s = c_int32(0), c_int32(0)
    check(lib().tsod_conv2d_resolve(byref(d), byref(t), byref(s)), "conv2d_resolve")
    return t.value, s.value


def linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """nn.Linear: x [M,K] @ weight[N,K]^T + bias."""
    require_cuda(x, "linear")
    x = x.contiguous()
    weight = weight.detach().contiguous()
    M, K = x.shape
    N = weight.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ws_bytes = lib().tsod_linear_workspace_bytes(M, K, N)
    ws = CONV_ARENA.get(x.device, ws_bytes) if ws_bytes else None
    check(lib().tsod_linear_f32(ptr(x), M, K, K, ptr(weight), ptr(bias), N, ptr(out), N, ptr(ws), ws_bytes,
                                stream_ptr()), "linear")
    return out


# ----------------------------------------------------------------------------- HBM-bound layers
def maxpool3x3s2_nhwc(x: torch.Tensor) -> torch.Tensor:
    require_cuda(x, "maxpool")
    N, H, W, C = x.shape
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.float32, device=x.device)
    check(lib().tsod_maxpool3x3s2_f32(ptr(x), N, H, W, C, C, ptr(out), C, stream_ptr()), "maxpool")
    return out


def dwconv3x3_nhwc(x: torch.Tensor, w33c: torch.Tensor, scale=None, shift=None, stride=1, relu=False, C=None,
                   in_off=0, out=None, out_off=0) -> torch.Tensor:
    """Depthwise 3x3 pad 1 on channels [in_off, in_off+C) of x [N,H,W,P]; w33c is [3,3,C].

    Differentiable in x, w33c, scale and shift (``_DWConv3x3``: tsod_dwconv3x3_grad_f32) when grad mode is on, one of them
    requires grad and the call is on whole tensors (no C / in_off / out / out_off); a call with any of those keeps the plain,
    non-differentiable path whatever requires grad, as before."""
    require_cuda(x, "dwconv3x3")
    whole = C is None and not in_off and out is None and not out_off and x.shape[3] == w33c.shape[2]
    if whole and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w33c, scale, shift)):
        return _DWConv3x3.apply(x, w33c, scale, shift, int(stride), bool(relu))
    N, H, W, P = x.shape
    C = w33c.shape[2] if C is None else C
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((N, OH, OW, C), dtype=torch.float32, device=x.device)
    check(lib().tsod_dwconv3x3_f32(ptr(x), N, H, W, C, P, in_off, ptr(w33c), ptr(scale), ptr(shift), stride,
                                   1 if relu else 0, ptr(out), out.shape[3], out_off, stream_ptr()), "dwconv3x3")
    return out


def gconv3x3_nhwc(x: torch.Tensor, w_packed: torch.Tensor, groups: int, scale=None, shift=None, stride=1, act=ACT_NONE,
                  slope=0.0) -> torch.Tensor:
    """Grouped 3x3 pad-1 conv on NHWC [N,H,W,C] -> [N,OH,OW,C]; w_packed is [C,3,3,C/groups] (ResNeXt's conv2)."""
    require_cuda(x, "gconv3x3")
    N, H, W, C = x.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((N, OH, OW, C), dtype=torch.float32, device=x.device)
    check(lib().tsod_gconv3x3_f32(ptr(x), N, H, W, C, C, int(groups), ptr(w_packed.contiguous()), ptr(scale), ptr(shift),
                                  int(stride), int(act), float(slope), ptr(out), C, stream_ptr()), "gconv3x3")
    return out


def dwconv3x3_grad(x, w33c, scale, shift, stride, relu, dy, *, want_dx=True, want_params=True, dx=None, accumulate=False,
                   in_off=0, dy_off=0, act_dx=False):
    """The backward of ``dwconv3x3_nhwc`` (tsod_dwconv3x3_grad_f32) -> (dx or None, dw [3,3,C], dscale [C] or None, dshift [C]).
    x [N,H,W,P] (channels [in_off, in_off+C)), dy [N,OH,OW,>= dy_off + C] contiguous (channels [dy_off, dy_off+C)).  ``dx``
    [N,H,W,C]: written, or added to with ``accumulate``; allocated when ``want_dx`` and none is given.  ``want_params`` False:
    dx only (dw, dscale, dshift None; without a ReLU that is the gather launch alone).  ``act_dx``: x is a ReLU6 output and dx
    is kept only where 0 < x < 6 (tsod_dwconv3x3_grad_act_f32: the masked gradient of the layer that made x)."""
    require_cuda(x, "dwconv3x3_grad")
    N, H, W, P = x.shape
    C = w33c.shape[2]
    dy = dy.contiguous()
    dev = x.device
    if dx is None and want_dx:
        dx, accumulate = torch.empty((N, H, W, C), dtype=torch.float32, device=dev), False
    dw = torch.empty((3, 3, C), dtype=torch.float32, device=dev) if want_params else None
    dscale = torch.empty(C, dtype=torch.float32, device=dev) if want_params and scale is not None else None
    dshift = torch.empty(C, dtype=torch.float32, device=dev) if want_params else None
    L = lib()
    ws_bytes = L.tsod_dwconv3x3_grad_workspace_bytes(N, H, W, C, int(stride), 1 if relu and dx is not None else 0)
    ws = ARENA.get(dev, ws_bytes)
    fn = L.tsod_dwconv3x3_grad_act_f32 if act_dx else L.tsod_dwconv3x3_grad_f32
    check(fn(ptr(x), N, H, W, C, P, int(in_off), ptr(w33c), ptr(scale), ptr(shift), int(stride), 1 if relu else 0, ptr(dy),
             dy.shape[3], int(dy_off), ptr(dx), 0 if dx is None else dx.shape[3], 0, 1 if accumulate else 0, ptr(dw), ptr(dscale),
             ptr(dshift), ptr(ws), ws_bytes, stream_ptr()), "dwconv3x3_grad")
    return dx, dw, dscale, dshift


def pw_segs(segs, real=None, want=None) -> _ffi.PwSegs:
    """``tsod_pw_segs`` from [(channel offset, padded width), ...], the real widths (default: the padded ones) and the
    per-segment "dx wanted" switches (default: all)."""
    if not 1 <= len(segs) <= _ffi.PW_MAX_SEGMENTS:
        raise ValueError(f"pw_segs: 1..{_ffi.PW_MAX_SEGMENTS} segments, got {len(segs)}")
    sg = _ffi.PwSegs()
    sg.n_seg = len(segs)
    for i, (off, ln) in enumerate(segs):
        sg.off[i], sg.len[i] = int(off), int(ln)
        sg.real[i] = int(ln if real is None else real[i])
        sg.want[i] = 1 if want is None or want[i] else 0
    return sg


def relu6_grad_mask(y: torch.Tensor, dy: torch.Tensor, dy_off: int = 0) -> torch.Tensor:
    """g = dy[..., dy_off:dy_off + C] * [0 < y < 6] (tsod_relu6_grad_mask_f32); y [..., C] and dy [..., P] contiguous."""
    require_cuda(y, "relu6_grad_mask")
    y, dy = y.contiguous(), dy.contiguous()
    C = y.shape[-1]
    g = torch.empty_like(y)
    check(lib().tsod_relu6_grad_mask_f32(ptr(y), y.numel() // C, C, C, ptr(dy), dy.shape[-1], int(dy_off), ptr(g), C, stream_ptr()),
          "relu6_grad_mask")
    return g


def conv1x1_bn_relu6_grad(x, segs, w, scale, y, dy, *, seg_real=None, seg_want=None, cout=None, dy_off=0, dx=None,
                          accumulate=False, want_dx=True, want_dw=True, want_dscale=True, want_dshift=True):
    """The backward of a 1x1 ConvLayer y = relu6(scale * (w . gather(x, segs)) + shift) ->
    (dx or None, dW [cout, sum(seg_real)] or None, dscale [cout] or None, dshift [cout] or None).

    x [..., P]: the NHWC buffer the forward gathered from; ``segs`` [(channel offset, padded width)] in the K order of ``w``
    [cout_pad, K] (or [cout_pad,1,1,K]; zero columns at pad channels), ``seg_real`` the real widths (default: no padding),
    ``cout`` the real output channels (default cout_pad).  ``scale`` [cout_pad]: the folded BN scale.  ``y`` [..., cout_pad]: the
    forward's saved output, the ReLU6 mask is taken from it (strict 0 < y < 6); ``y`` None: ``dy`` is already the masked
    gradient g (what ``dwconv3x3_grad(act_dx=True)`` returns).  dy [..., >= dy_off + cout_pad] contiguous.
    ``dx`` [..., Pd] (default: zeros like x, written): segments with ``seg_want`` (default all) are written, or added to with
    ``accumulate``, at the offsets of ``segs``; their pad channels become exact zeros; nothing else is touched; segments nobody
    wants are not computed.  Launches: the mask pass (with ``y``), tsod_pw_wgrad_f32 when any of dW / dscale / dshift is wanted,
    tsod_pw_dgrad_f32 when ``want_dx``."""
    require_cuda(x, "conv1x1_bn_relu6_grad")
    dev = x.device
    w2 = w.reshape(w.shape[0], -1)
    if not (x.is_contiguous() and w2.is_contiguous() and scale.is_contiguous()):
        raise ValueError("conv1x1_bn_relu6_grad: x, w and scale must be contiguous")
    n_pad, K = w2.shape
    cout = n_pad if cout is None else int(cout)
    sg = pw_segs(segs, seg_real, seg_want)
    if sum(ln for _, ln in segs) != K:
        raise ValueError(f"conv1x1_bn_relu6_grad: the segments add up to {sum(ln for _, ln in segs)} columns, w has {K}")
    P = x.shape[-1]
    M = x.numel() // P
    if y is not None:
        g = relu6_grad_mask(y, dy, dy_off)
    else:
        g = dy.contiguous()
        if dy_off or g.shape[-1] != n_pad:
            raise ValueError("conv1x1_bn_relu6_grad: a masked gradient (y=None) must be a contiguous [..., cout_pad] tensor")
    if g.numel() != M * n_pad:
        raise ValueError(f"conv1x1_bn_relu6_grad: {M} pixel rows of x, gradient of shape {tuple(g.shape)}")
    L = lib()
    k_real = sum(sg.real[i] for i in range(sg.n_seg))
    dw = torch.empty((cout, k_real), dtype=torch.float32, device=dev) if want_dw else None
    dscale = torch.empty(cout, dtype=torch.float32, device=dev) if want_dscale else None
    dshift = torch.empty(cout, dtype=torch.float32, device=dev) if want_dshift else None
    if want_dw or want_dscale or want_dshift:
        ws_bytes = L.tsod_pw_wgrad_workspace_bytes(M, n_pad, K)
        ws = ARENA.get(dev, ws_bytes)
        check(L.tsod_pw_wgrad_f32(ptr(g), M, n_pad, n_pad, ptr(x), P, byref(sg), ptr(w2), ptr(scale), cout, ptr(dw), ptr(dscale),
                                  ptr(dshift), ptr(ws), ws_bytes, stream_ptr()), "pw_wgrad")
    if want_dx:
        if dx is None:
            dx, accumulate = torch.zeros_like(x), False
        if not dx.is_contiguous() or dx.numel() // dx.shape[-1] != M:
            raise ValueError("conv1x1_bn_relu6_grad: dx must be a contiguous buffer with x's pixel rows")
        check(L.tsod_pw_dgrad_f32(ptr(g), M, n_pad, n_pad, ptr(w2), ptr(scale), byref(sg), ptr(dx), dx.shape[-1],
                                  1 if accumulate else 0, stream_ptr()), "pw_dgrad")
    return (dx if want_dx else None), dw, dscale, dshift


def conv3x3_bn_relu6_grad(x4, w, scale, y, dy, *, stride=2, cout=None, dy_off=0, want_dw=True, want_dscale=True,
                          want_dshift=True, raw=False):
    """The parameter gradients of HarDNet's first layer y = relu6(scale * conv3x3(x4, w, stride, pad 1) + shift) (DESIGN.md
    section 4.19; tsod_conv3x3_wgrad_f32) -> (dW [cout,3,3,3] in torch's layout or None, dscale [cout] or None, dshift [cout]
    or None).  There is no dx: the image has no gradient.

    x4 [N,H,W,4]: the image padded to four channels (channel 3 is never read).  w [cout_pad,3,3,4]: the unscaled packed weight,
    scale [cout_pad] the folded BN scale, ``cout`` the real output channels (default cout_pad).  y [N,OH,OW,cout_pad]: the
    forward's saved output, the ReLU6 mask is taken from it inside the kernel (strict 0 < y < 6).  dy [N,OH,OW,>= dy_off +
    cout_pad] contiguous (channels [dy_off, dy_off + cout_pad)).  ``raw``: the kernel's own padded outputs instead, dW
    [cout_pad,3,3,4] and [cout_pad] vectors (pad rows and channel 3 are exact zeros)."""
    require_cuda(x4, "conv3x3_bn_relu6_grad")
    if not (x4.is_contiguous() and w.is_contiguous() and scale.is_contiguous() and y.is_contiguous() and dy.is_contiguous()):
        raise ValueError("conv3x3_bn_relu6_grad: x4, w, scale, y and dy must be contiguous")
    N, H, W, P = x4.shape
    cp = w.shape[0]
    if P != 4 or tuple(w.shape[1:]) != (3, 3, 4):
        raise ValueError(f"conv3x3_bn_relu6_grad: x4 must be [N,H,W,4] and w [cout_pad,3,3,4], got {tuple(x4.shape)}, {tuple(w.shape)}")
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if tuple(y.shape) != (N, OH, OW, cp) or tuple(dy.shape[:3]) != (N, OH, OW):
        raise ValueError(f"conv3x3_bn_relu6_grad: y {tuple(y.shape)} / dy {tuple(dy.shape)} do not match [{N},{OH},{OW},{cp}]")
    if not (want_dw or want_dscale or want_dshift):
        raise ValueError("conv3x3_bn_relu6_grad: nothing is wanted")
    cout = cp if cout is None else int(cout)
    dev = x4.device
    dw = torch.empty((cp, 3, 3, 4), dtype=torch.float32, device=dev) if want_dw else None
    dscale = torch.empty(cp, dtype=torch.float32, device=dev) if want_dscale else None
    dshift = torch.empty(cp, dtype=torch.float32, device=dev) if want_dshift else None
    L = lib()
    ws_bytes = L.tsod_conv3x3_wgrad_workspace_bytes(N, H, W, cp, int(stride))
    ws = ARENA.get(dev, ws_bytes) if ws_bytes else None
    check(L.tsod_conv3x3_wgrad_f32(ptr(x4), N, H, W, ptr(y), ptr(dy), dy.shape[3], int(dy_off), ptr(w), ptr(scale), cp, cout,
                                   int(stride), ptr(dw), ptr(dscale), ptr(dshift), ptr(ws), ws_bytes, stream_ptr()), "conv3x3_wgrad")
    if raw:
        return dw, dscale, dshift
    return (None if dw is None else dw[:cout, :, :, :3].permute(0, 3, 1, 2).contiguous(),
            None if dscale is None else dscale[:cout], None if dshift is None else dshift[:cout])


def prelu_grad(y: torch.Tensor, dy: torch.Tensor, slope: float, dy_off: int = 0, want_dslope: bool = True, g=None):
    """The backward of y = prelu(z) with one slope > 0, from the saved OUTPUT (tsod_prelu_grad_f32) ->
    (g, dslope_num): g = dy[..., dy_off:dy_off + C] * (y > 0 ? 1 : slope), dslope_num [1] = sum dy * y * [y < 0] (the slope's
    gradient is dslope_num / slope) or None without ``want_dslope``.  y [..., C] and dy [..., P] contiguous; ``g``: where to
    write ([..., Pg], columns [0, C); default a fresh [..., C])."""
    require_cuda(y, "prelu_grad")
    if not (y.is_contiguous() and dy.is_contiguous() and (g is None or g.is_contiguous())):
        raise ValueError("prelu_grad: y, dy and g must be contiguous")
    C = y.shape[-1]
    rows = y.numel() // C
    if g is None:
        g = torch.empty_like(y)
    for what, t, first in (("dy", dy, int(dy_off)), ("g", g, 0)):
        if t.dim() < 1 or first < 0 or first + C > t.shape[-1] or t.numel() != rows * t.shape[-1] or t.device != y.device \
                or t.dtype != torch.float32:
            raise ValueError(f"prelu_grad: {what} {tuple(t.shape)} does not hold columns [{first}, {first + C}) of y's {rows} rows "
                             f"(y {tuple(y.shape)}) as float32 on {y.device}")
    num = torch.empty(1, dtype=torch.float32, device=y.device) if want_dslope else None
    L = lib()
    ws_bytes = L.tsod_prelu_grad_workspace_bytes(rows, C) if want_dslope else 0
    ws = ARENA.get(y.device, ws_bytes) if ws_bytes else None
    check(L.tsod_prelu_grad_f32(ptr(y), rows, C, C, ptr(dy), dy.shape[-1], int(dy_off), float(slope), ptr(g), g.shape[-1], ptr(num),
                                ptr(ws), ws_bytes, stream_ptr()), "prelu_grad")
    return g, num


def conv3x3_dense_wgrad(g, x, w, scale, *, stride=1, want_dw=True, want_dscale=True, want_dshift=True):
    """The parameter gradients of z = scale * conv3x3(x, w, pad 1) + shift from the masked gradient g (DESIGN.md section 4.21;
    tsod_conv3x3_dense_wgrad_f32) -> (dW [Cout,3,3,C] in the pack's layout or None, dscale [Cout] or None, dshift [Cout] or None).
    g [N,H,W,Cout], x [N,H,W,C], w [Cout,3,3,C] (the forward's f32 pack, unscaled), scale [Cout]; all contiguous."""
    require_cuda(x, "conv3x3_dense_wgrad")
    if not (g.is_contiguous() and x.is_contiguous() and w.is_contiguous() and scale.is_contiguous()):
        raise ValueError("conv3x3_dense_wgrad: g, x, w and scale must be contiguous")
    N, H, W, C = x.shape
    Cout = w.shape[0]
    if tuple(w.shape) != (Cout, 3, 3, C) or tuple(g.shape) != (N, H, W, Cout) or scale.numel() != Cout:
        raise ValueError(f"conv3x3_dense_wgrad: g {tuple(g.shape)}, x {tuple(x.shape)}, w {tuple(w.shape)} do not belong together")
    if not (want_dw or want_dscale or want_dshift):
        raise ValueError("conv3x3_dense_wgrad: nothing is wanted")
    dev = x.device
    dw = torch.empty_like(w) if want_dw else None
    dscale = torch.empty(Cout, dtype=torch.float32, device=dev) if want_dscale else None
    dshift = torch.empty(Cout, dtype=torch.float32, device=dev) if want_dshift else None
    L = lib()
    ws_bytes = L.tsod_conv3x3_dense_wgrad_workspace_bytes(N, H, W, C, Cout)
    ws = ARENA.get(dev, ws_bytes) if ws_bytes else None
    check(L.tsod_conv3x3_dense_wgrad_f32(ptr(g), N, H, W, Cout, Cout, ptr(x), C, C, ptr(w), ptr(scale), int(stride), ptr(dw),
                                         ptr(dscale), ptr(dshift), ptr(ws), ws_bytes, stream_ptr()), "conv3x3_dense_wgrad")
    return dw, dscale, dshift


def rotate_conv3x3_weight(w: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """w [Cout,3,3,C] (a 3x3 conv's f32 pack), scale [Cout] -> w_rot [C,3,3,Cout] = scale[o] * w[o][2 - kh][2 - kw][c]: the pack
    with which ``conv2d_nhwc(g, w_rot, pad=1)`` is that conv's dx (stride 1, pad 1)."""
    return (w * scale.view(-1, 1, 1, 1)).flip(1, 2).permute(3, 1, 2, 0).contiguous()


def s2d_conv3x3_weight(w: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """w [Cout,3,3,C] (a 3x3 conv's f32 pack), scale [Cout] -> w_s2d [4 C,2,2,Cout], the 2x2 phase pack of that conv's dx at
    stride 2, pad 1: row ((ih & 1) 2 + (iw & 1)) C + c holds, per axis, for an even phase tap offset
    d = 0 <-> k = 1, for an odd phase d = 0 <-> k = 2 and d = 1 <-> k = 0; an entry is scale[o] * w[o][kh][kw][c] or zero.
    With P = ``conv2d_nhwc(g, w_s2d, pad=1)`` [N,OH+1,OW+1,4 C]: dx[n,ih,iw,c] = P[n, (ih >> 1) + 1, (iw >> 1) + 1,
    ((ih & 1) 2 + (iw & 1)) C + c]."""
    Cout, _, _, C = w.shape
    ws = w * scale.view(-1, 1, 1, 1)
    out = torch.zeros((2, 2, C, 2, 2, Cout), dtype=w.dtype, device=w.device)
    taps = (((0, 1),), ((0, 2), (1, 0)))                          # per phase parity: (tap offset d, filter index k)
    for ph in (0, 1):
        for pw in (0, 1):
            for dh, kh in taps[ph]:
                for dw, kw in taps[pw]:
                    out[ph, pw, :, dh, dw, :] = ws[:, kh, kw, :].t()
    return out.view(4 * C, 2, 2, Cout)


def conv3x3_strided_wgrad(g, x, w, scale, *, stride, want_dw=True, want_dscale=True, want_dshift=True):
    """``conv3x3_dense_wgrad`` for a 3x3 at stride 1 or 2, pad 1 (tsod_conv3x3_strided_wgrad_f32): g
    [N,OH,OW,>= Cout] over the output grid, OH = (H - 1) // stride + 1; x [N,H,W,>= C]; the channels are the first Cout / C of
    each pixel.  With stride 1 the bits of ``conv3x3_dense_wgrad``."""
    require_cuda(x, "conv3x3_strided_wgrad")
    if not (g.is_contiguous() and x.is_contiguous() and w.is_contiguous() and scale.is_contiguous()):
        raise ValueError("conv3x3_strided_wgrad: g, x, w and scale must be contiguous")
    N, H, W, Px = x.shape
    Cout, C, stride = w.shape[0], w.shape[3], int(stride)
    if stride not in (1, 2):
        raise ValueError(f"conv3x3_strided_wgrad: stride 1 or 2, got {stride}")
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if tuple(w.shape) != (Cout, 3, 3, C) or tuple(g.shape[:3]) != (N, OH, OW) or g.shape[3] < Cout or Px < C or scale.numel() != Cout:
        raise ValueError(f"conv3x3_strided_wgrad: g {tuple(g.shape)}, x {tuple(x.shape)}, w {tuple(w.shape)} do not belong together "
                         f"at stride {stride}")
    if not (want_dw or want_dscale or want_dshift):
        raise ValueError("conv3x3_strided_wgrad: nothing is wanted")
    dev = x.device
    dw = torch.empty_like(w) if want_dw else None
    dscale = torch.empty(Cout, dtype=torch.float32, device=dev) if want_dscale else None
    dshift = torch.empty(Cout, dtype=torch.float32, device=dev) if want_dshift else None
    L = lib()
    ws_bytes = L.tsod_conv3x3_strided_wgrad_workspace_bytes(N, H, W, C, Cout, stride)
    ws = ARENA.get(dev, ws_bytes) if ws_bytes else None
    check(L.tsod_conv3x3_strided_wgrad_f32(ptr(g), N, H, W, Cout, g.shape[3], ptr(x), C, Px, ptr(w), ptr(scale), stride, ptr(dw),
                                           ptr(dscale), ptr(dshift), ptr(ws), ws_bytes, stream_ptr()), "conv3x3_strided_wgrad")
    return dw, dscale, dshift


def prelu_grad_d2s(y: torch.Tensor, p: torch.Tensor, slope: float, want_dslope: bool = True):
    """``prelu_grad`` for the input y [N,H,W,C] of a stride-2 3x3 whose dy is read from the phase-stacked image p
    [N,(H-1)//2+2,(W-1)//2+2,4 C] of ``s2d_conv3x3_weight`` (tsod_prelu_grad_d2s_f32) -> (g, dslope_num)."""
    require_cuda(y, "prelu_grad_d2s")
    if not (y.is_contiguous() and p.is_contiguous()) or y.dim() != 4:
        raise ValueError("prelu_grad_d2s: y [N,H,W,C] and p must be contiguous")
    N, H, W, C = y.shape
    if tuple(p.shape) != (N, (H - 1) // 2 + 2, (W - 1) // 2 + 2, 4 * C) or p.dtype != torch.float32 or p.device != y.device:
        raise ValueError(f"prelu_grad_d2s: p {tuple(p.shape)} is not the phase-stacked image of y {tuple(y.shape)}")
    g = torch.empty_like(y)
    num = torch.empty(1, dtype=torch.float32, device=y.device) if want_dslope else None
    L = lib()
    ws_bytes = L.tsod_prelu_grad_d2s_workspace_bytes(N, H, W, C) if want_dslope else 0
    ws = ARENA.get(y.device, ws_bytes) if ws_bytes else None
    check(L.tsod_prelu_grad_d2s_f32(ptr(y), N, H, W, C, C, ptr(p), 4 * C, float(slope), ptr(g), C, ptr(num), ptr(ws), ws_bytes,
                                    stream_ptr()), "prelu_grad_d2s")
    return g, num


def prelu_grad_pool(y: torch.Tensor, dp: torch.Tensor, slope: float, want_dslope: bool = True, C: int | None = None, g=None):
    """``prelu_grad`` for the input y [N,OH,OW,>= C] of ``MaxPool2d(3, 2, 1)`` whose dy is gathered from dp [N,PH,PW,>= C], the
    gradient of the pooled map (PH = (OH-1)//2+1; tsod_prelu_grad_pool_f32) -> (g, dslope_num): every
    element takes the dp of the windows whose first maximum it is.  The channels are the first ``C`` of each pixel (default
    y's last dimension); ``g``: where to write ([N,OH,OW,>= C]; default a fresh [N,OH,OW,C])."""
    require_cuda(y, "prelu_grad_pool")
    if y.dim() != 4 or dp.dim() != 4 or not (y.is_contiguous() and dp.is_contiguous() and (g is None or g.is_contiguous())):
        raise ValueError("prelu_grad_pool: y [N,OH,OW,P], dp [N,PH,PW,P] and g must be contiguous")
    N, OH, OW, Py = y.shape
    C = Py if C is None else int(C)
    if g is None:
        g = torch.empty((N, OH, OW, C), dtype=torch.float32, device=y.device)
    if (tuple(dp.shape[:3]) != (N, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1) or dp.shape[3] < C or Py < C or g.dim() != 4
            or tuple(g.shape[:3]) != (N, OH, OW) or g.shape[3] < C
            or any(t.dtype != torch.float32 or t.device != y.device for t in (y, dp, g))):
        raise ValueError(f"prelu_grad_pool: dp {tuple(dp.shape)} / g {tuple(g.shape)} do not belong to {C} channels of y "
                         f"{tuple(y.shape)} as float32 on {y.device}")
    num = torch.empty(1, dtype=torch.float32, device=y.device) if want_dslope else None
    L = lib()
    ws_bytes = L.tsod_prelu_grad_pool_workspace_bytes(N, OH, OW, C) if want_dslope else 0
    ws = ARENA.get(y.device, ws_bytes) if ws_bytes else None
    check(L.tsod_prelu_grad_pool_f32(ptr(y), N, OH, OW, C, Py, ptr(dp), dp.shape[3], float(slope), ptr(g), g.shape[3], ptr(num),
                                     ptr(ws), ws_bytes, stream_ptr()), "prelu_grad_pool")
    return g, num


def conv7x7s2_wgrad(g, x4, w, scale, want_dw=True, want_dscale=True, want_dshift=True, raw=False):
    """The parameter gradients of ResNet's conv1, z = scale * conv7x7(x4, w, stride 2, pad 3) + shift, from the masked gradient
    g (tsod_conv7x7s2_wgrad_f32) -> (dW [64,3,7,7] in torch's layout or None, dscale [64] or None,
    dshift [64] or None).  g [N,OH,OW,>= 64] (the first 64 columns), x4 [N,H,W,4] the staged image (channel 3 reaches nothing),
    w [64,7,8,4] the forward's f32 pack, scale [64]; all contiguous.  ``raw``: dW as the kernel writes it, [64,7,8,4] with exact
    zeros in the padding."""
    require_cuda(x4, "conv7x7s2_wgrad")
    if not (g.is_contiguous() and x4.is_contiguous() and w.is_contiguous() and scale.is_contiguous()):
        raise ValueError("conv7x7s2_wgrad: g, x4, w and scale must be contiguous")
    if x4.dim() != 4 or x4.shape[3] != 4 or w.dim() != 4 or tuple(w.shape[1:]) != (7, 8, 4):
        raise ValueError(f"conv7x7s2_wgrad: x4 must be [N,H,W,4] and w [Cout,7,8,4], got {tuple(x4.shape)}, {tuple(w.shape)}")
    N, H, W, _ = x4.shape
    Cout = w.shape[0]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if g.dim() != 4 or tuple(g.shape[:3]) != (N, OH, OW) or g.shape[3] < Cout or scale.numel() != Cout:
        raise ValueError(f"conv7x7s2_wgrad: g {tuple(g.shape)}, x4 {tuple(x4.shape)}, w {tuple(w.shape)} do not belong together")
    if not (want_dw or want_dscale or want_dshift):
        raise ValueError("conv7x7s2_wgrad: nothing is wanted")
    dev = x4.device
    dw = torch.empty_like(w) if want_dw else None
    dscale = torch.empty(Cout, dtype=torch.float32, device=dev) if want_dscale else None
    dshift = torch.empty(Cout, dtype=torch.float32, device=dev) if want_dshift else None
    L = lib()
    ws_bytes = L.tsod_conv7x7s2_wgrad_workspace_bytes(N, H, W, Cout)
    ws = ARENA.get(dev, ws_bytes) if ws_bytes else None
    check(L.tsod_conv7x7s2_wgrad_f32(ptr(g), N, H, W, Cout, g.shape[3], ptr(x4), ptr(w), ptr(scale), ptr(dw), ptr(dscale),
                                     ptr(dshift), ptr(ws), ws_bytes, stream_ptr()), "conv7x7s2_wgrad")
    if dw is not None and not raw:
        dw = dw[:, :, :7, :3].permute(0, 3, 1, 2).contiguous()
    return dw, dscale, dshift


def pixel_subsample(x: torch.Tensor, stride: int, C: int | None = None) -> torch.Tensor:
    """xs [N,OH,OW,C] = x[n, stride oh, stride ow, :C] (tsod_pixel_subsample_f32); x [N,H,W,P] contiguous, C default P."""
    require_cuda(x, "pixel_subsample")
    if not x.is_contiguous() or x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("pixel_subsample: x [N,H,W,P] must be contiguous float32")
    N, H, W, P = x.shape
    C, stride = P if C is None else int(C), int(stride)
    if stride < 1:
        raise ValueError(f"pixel_subsample: stride must be >= 1, got {stride}")
    xs = torch.empty((N, (H - 1) // stride + 1, (W - 1) // stride + 1, C), dtype=torch.float32, device=x.device)
    check(lib().tsod_pixel_subsample_f32(ptr(x), N, H, W, C, P, stride, ptr(xs), C, stream_ptr()), "pixel_subsample")
    return xs


def pixel_upsample_add(dx: torch.Tensor, d: torch.Tensor, stride: int, C: int | None = None) -> torch.Tensor:
    """dx[n, stride oh, stride ow, :C] += d[n, oh, ow, :C] in place (tsod_pixel_upsample_add_f32; dx the first operand); dx
    [N,H,W,P], d [N,OH,OW,Pd] contiguous, C default d's Pd.  Returns dx."""
    require_cuda(dx, "pixel_upsample_add")
    if not (dx.is_contiguous() and d.is_contiguous()) or dx.dim() != 4 or d.dim() != 4 or dx.dtype != torch.float32:
        raise ValueError("pixel_upsample_add: dx [N,H,W,P] and d [N,OH,OW,Pd] must be contiguous float32")
    N, H, W, P = dx.shape
    C, stride = d.shape[3] if C is None else int(C), int(stride)
    if stride < 1:
        raise ValueError(f"pixel_upsample_add: stride must be >= 1, got {stride}")
    if tuple(d.shape[:3]) != (N, (H - 1) // stride + 1, (W - 1) // stride + 1) or d.device != dx.device or d.dtype != torch.float32:
        raise ValueError(f"pixel_upsample_add: d {tuple(d.shape)} is not dx {tuple(dx.shape)} at stride {stride}")
    check(lib().tsod_pixel_upsample_add_f32(ptr(dx), N, H, W, C, P, stride, ptr(d), d.shape[3], stream_ptr()), "pixel_upsample_add")
    return dx


def _bn_rows(t: torch.Tensor, what: str):
    if t.dim() < 2 or not t.is_contiguous():
        raise ValueError(f"{what}: contiguous [..., channels] tensors only, got {tuple(t.shape)}")
    return t.numel() // t.shape[-1], t.shape[-1]


def _bn_channels(gamma, C_real):
    C_real = int(gamma.numel() if C_real is None else C_real)
    return C_real, (C_real + 3) // 4 * 4


def _bn_pitches(what: str, lead: str, M: int, dev, named) -> dict:
    """name -> pitch of the (name, tensor) pairs ``named`` (None: absent), each contiguous float32 on ``dev`` with M rows."""
    lds = {}
    for name, t in named:
        if t is None:
            continue
        Mt, lds[name] = _bn_rows(t, what)
        if Mt != M or t.device != dev or t.dtype != torch.float32:
            raise ValueError(f"{what}: {lead} has {M} float32 rows on {dev}, {name} is {tuple(t.shape)} {t.dtype} on {t.device}")
    return lds


def _bn_train_forward(what, z, gamma, beta, eps, momentum, running_mean, running_var, off, out, C_real, num_batches_tracked,
                      operands=()):
    """What both forwards do before their apply launch; ``operands``: (name, tensor) pairs with z's rows
    -> (M, C_real, C_pad, out, pitches by name, mean, invstd, scale, shift)."""
    require_cuda(z, what)
    M, ld = _bn_rows(z, what)
    if M < 2:
        raise ValueError(f"{what}: more than one value per channel is needed in training mode, got {M} row(s)")
    C_real, cp = _bn_channels(gamma, C_real)
    if out is None:
        out = torch.empty(z.shape[:-1] + (cp,), dtype=torch.float32, device=z.device)
    lds = dict(_bn_pitches(what, "z", M, z.device, (("out", out),) + operands), z=ld)
    return (M, C_real, cp, out, lds) + batch_norm_stats(z, gamma, beta, eps, momentum, running_mean, running_var, off=off,
                                                        C_real=C_real, num_batches_tracked=num_batches_tracked)


def _bn_train_backward(what, lead, t0, named, mean, invstd, gamma, C_real, dz, workspace_bytes):
    """What both backwards do before their three launches; ``t0`` is the tensor called ``lead``, ``named`` (name, tensor) pairs
    with its rows, ``workspace_bytes`` the entry point's query -> (M, C_real, C_pad, dz, pitches by name, dgamma, dbeta, ws, ws_bytes)."""
    require_cuda(t0, what)
    M, ld = _bn_rows(t0, what)
    cp, dev = mean.numel(), t0.device
    if M < 2 or invstd.numel() != cp:
        raise ValueError(f"{what}: {lead} has {M} rows (at least 2), mean {cp} / invstd {invstd.numel()} channels")
    if dz is None:
        dz = torch.empty(t0.shape[:-1] + (cp,), dtype=torch.float32, device=dev)
    lds = dict(_bn_pitches(what, lead, M, dev, named + (("dz", dz),)), **{lead: ld})
    dgamma, dbeta = (torch.empty(cp, dtype=torch.float32, device=dev) for _ in range(2))
    ws_bytes = workspace_bytes(M, cp)
    return M, _bn_channels(gamma, C_real)[0], cp, dz, lds, dgamma, dbeta, ARENA.get(dev, ws_bytes), ws_bytes


def batch_norm_train(z, gamma, beta, eps, momentum, running_mean=None, running_var=None, *, act=ACT_NONE, off=0, out=None,
                     out_off=0, C_real=None, num_batches_tracked=None, amax_out=None):
    """Train-mode BatchNorm of NHWC rows (tsod_bn_stats_f32, tsod_bn_apply_f32) -> (y, mean, invstd).

    z [..., ld] contiguous: the channels are [off, off + C_pad), C_pad = ``gamma``'s length rounded up to 4 (``C_real``: the real
    channels, default ``gamma``'s length; the columns up to C_pad must exist in z).  gamma, beta [C_real].  mean [C_pad] and
    invstd [C_pad] = 1 / sqrt(biased variance + eps) are the batch statistics over all rows, y = act(gamma * invstd * (z - mean)
    + beta) in its folded form scale * z + shift, ``act`` ACT_NONE or ACT_RELU6.  ``out`` [..., ld_out] (default: a new
    [..., C_pad] tensor) receives y at channels [out_off, out_off + C_pad), nothing else of it is touched; pad channels of y,
    mean and invstd are exact zeros.  ``running_mean`` / ``running_var`` [C_real] (each optional) are updated in place like
    torch's: (1 - momentum) * old + momentum * (mean | unbiased variance); ``num_batches_tracked`` (int64 scalar tensor) is
    incremented; ``amax_out``: the range words of ``out``'s tensor.  ValueError for fewer than 2 rows (torch refuses one value
    per channel in training mode).  Launches: two for the statistics (workgroup partials, their merge), one for y."""
    M, C_real, cp, out, lds, mean, invstd, scale, shift = _bn_train_forward(
        "batch_norm_train", z, gamma, beta, eps, momentum, running_mean, running_var, off, out, C_real, num_batches_tracked)
    check(lib().tsod_bn_apply_f32(ptr(z), M, C_real, cp, lds["z"], int(off), ptr(scale), ptr(shift), int(act), ptr(out), lds["out"],
                                  int(out_off), _word_ptr(amax_out), stream_ptr()), "bn_apply")
    return out, mean, invstd


def batch_norm_train_grad(g, z, mean, invstd, gamma, *, g_off=0, z_off=0, dz=None, dz_off=0, C_real=None):
    """The backward of ``batch_norm_train`` (tsod_bn_train_grad_f32) -> (dz, dgamma [C_pad], dbeta [C_pad]).

    g [..., ld_g] contiguous (channels [g_off, g_off + C_pad)): the gradient of the BatchNorm's output - where a ReLU6
    follows, already masked (what ``relu6_grad_mask`` / ``dwconv3x3_grad(act_dx=True)`` return).  z [..., ld_z] (channels
    [z_off, z_off + C_pad)): the saved input.  mean, invstd [C_pad]: what the forward returned; gamma [C_real] (``C_real``
    default: its length).  With xhat = (z - mean) * invstd: dgamma = sum g xhat, dbeta = sum g, dz = gamma * invstd * (g -
    dbeta / M - xhat * dgamma / M), written to channels [dz_off, dz_off + C_pad) of ``dz`` (default: a new [..., C_pad] tensor);
    pad channels of all three are exact zeros.  Launches: the workgroups' partial sums, their sum, the elementwise pass."""
    L = lib()
    M, C_real, cp, dz, lds, dgamma, dbeta, ws, ws_bytes = _bn_train_backward(
        "batch_norm_train_grad", "g", g, (("z", z),), mean, invstd, gamma, C_real, dz, L.tsod_bn_train_workspace_bytes)
    check(L.tsod_bn_train_grad_f32(ptr(g), lds["g"], int(g_off), ptr(z), lds["z"], int(z_off), M, C_real, cp, ptr(mean), ptr(invstd),
                                   ptr(gamma), ptr(dz), lds["dz"], int(dz_off), ptr(dgamma), ptr(dbeta), ptr(ws), ws_bytes,
                                   stream_ptr()), "bn_train_grad")
    return dz, dgamma, dbeta


def batch_norm_stats(z, gamma, beta, eps, momentum, running_mean=None, running_var=None, *, off=0, C_real=None,
                     num_batches_tracked=None):
    """The statistics half of a train-mode BatchNorm (tsod_bn_stats_f32) -> (mean, invstd, scale, shift).

    z, gamma, beta, the running statistics and ``num_batches_tracked`` as in ``batch_norm_train``.  mean, invstd [C_pad]; scale =
    gamma * invstd and shift = beta - mean * scale as [2, C_pad]: the float32 value and the float32 remainder of the float64 one
    (what ``batch_norm_prelu_train`` takes for its second operand).  ValueError for fewer than 2 rows.  Two launches."""
    require_cuda(z, "batch_norm_stats")
    M, ld = _bn_rows(z, "batch_norm_stats")
    if M < 2:
        raise ValueError(f"batch_norm_stats: more than one value per channel is needed in training mode, got {M} row(s)")
    C_real, cp = _bn_channels(gamma, C_real)
    dev = z.device
    mean, invstd = (torch.empty(cp, dtype=torch.float32, device=dev) for _ in range(2))
    scale, shift = (torch.empty((2, cp), dtype=torch.float32, device=dev) for _ in range(2))      # (value, f32 remainder)
    L = lib()
    ws_bytes = L.tsod_bn_train_workspace_bytes(M, cp)
    ws = ARENA.get(dev, ws_bytes)
    check(L.tsod_bn_stats_f32(ptr(z), M, C_real, cp, ld, int(off), ptr(gamma), ptr(beta), float(eps), float(momentum),
                              ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), ptr(mean), ptr(invstd), ptr(scale),
                              ptr(shift), ptr(ws), ws_bytes, stream_ptr()), "bn_stats")
    return mean, invstd, scale, shift


def batch_norm_prelu_train(z, gamma, beta, eps, momentum, slope, running_mean=None, running_var=None, *, off=0, residual=None,
                           residual_off=0, second=None, out=None, out_off=0, C_real=None, num_batches_tracked=None, amax_out=None):
    """Train-mode BatchNorm with ResNet's epilogue (tsod_bn_stats_f32, tsod_bn_apply_prelu_f32)
    -> (y, mean, invstd).

    y = prelu(gamma * invstd * (z - mean) + beta + R, slope) on the batch statistics of z, everything else as in
    ``batch_norm_train``: z [..., ld] contiguous with the channels at [off, off + C_pad), gamma, beta [C_real], the running
    statistics and ``num_batches_tracked`` updated in place, ``out`` [..., ld_out] receiving y at [out_off, out_off + C_pad)
    (default: a new [..., C_pad] tensor), pad channels exact zeros, ``amax_out`` the range words of ``out``'s tensor, ValueError
    for fewer than 2 rows.  R is at most one of
      ``residual``  a tensor [..., ld_r] with as many rows (channels [residual_off, residual_off + C_pad)): an identity block's x;
      ``second``    (z2, scale2, shift2, z2_off): another BatchNorm's input [..., ld_2] (channels [z2_off, z2_off + C_pad)) with
                    the scale / shift ``batch_norm_stats`` gave for it: a projection block's downsample.1.
    The BatchNorm's terms and R are added in float64 and rounded to float32 once; the PReLU (one ``slope``, by value, not
    checked here: the module keeps it finite and > 0) runs on that.  Launches: two for the statistics, one for y."""
    if residual is not None and second is not None:
        raise ValueError("batch_norm_prelu_train: a residual tensor or a second normalised operand, not both")
    z2, scale2, shift2, z2_off = (None, None, None, 0) if second is None else second
    if second is not None:
        cp = _bn_channels(gamma, C_real)[1]
        if tuple(scale2.shape) != (2, cp) or tuple(shift2.shape) != (2, cp):
            raise ValueError(f"batch_norm_prelu_train: the second operand's scale / shift must be [2, {cp}]")
    M, C_real, cp, out, lds, mean, invstd, scale, shift = _bn_train_forward(
        "batch_norm_prelu_train", z, gamma, beta, eps, momentum, running_mean, running_var, off, out, C_real, num_batches_tracked,
        (("residual", residual), ("second", z2)))
    check(lib().tsod_bn_apply_prelu_f32(ptr(z), M, C_real, cp, lds["z"], int(off), ptr(scale), ptr(shift), ptr(residual),
                                        lds.get("residual", 0), int(residual_off), ptr(z2), lds.get("second", 0), int(z2_off),
                                        ptr(scale2), ptr(shift2), float(slope), ptr(out), lds["out"], int(out_off),
                                        _word_ptr(amax_out), stream_ptr()), "bn_apply_prelu")
    return out, mean, invstd


def batch_norm_prelu_train_grad(y, dy, z, mean, invstd, gamma, slope, *, y_off=0, dy_off=0, z_off=0, dz=None, dz_off=0, C_real=None,
                                want_dslope=True, want_g=False, g=None, g_off=0):
    """The backward of ``batch_norm_prelu_train`` from its saved output (tsod_bn_prelu_train_grad_f32)
    -> (dz, dgamma [C_pad], dbeta [C_pad], dslope_num [1] or None, g or None).

    ``prelu_grad`` followed by ``batch_norm_train_grad`` as one group of three launches.  y [..., ld_y] (channels [y_off, y_off +
    C_pad)): the saved OUTPUT of the PReLU; dy [..., ld_dy] (channels [dy_off, ...)): its gradient; z [..., ld_z] (channels
    [z_off, ...)): the BatchNorm's saved input; mean, invstd [C_pad]: what the forward returned; gamma [C_real] (``C_real``
    default: its length); ``slope`` the forward's, finite and > 0.  g = dy * (y > 0 ? 1 : slope), an exact y == 0 taking the
    slope branch; with xhat = (z - mean) * invstd: dgamma = sum g xhat, dbeta = sum g, dz = gamma * invstd * (g - dbeta / M -
    xhat * dgamma / M), written to channels [dz_off, dz_off + C_pad) of ``dz`` (default: a new [..., C_pad] tensor).
    dslope_num = sum dy * y * [y < 0] over the real channels (the slope's gradient times the slope), None without
    ``want_dslope``.  ``want_g`` (or a ``g`` [..., ld_g] to write at channels [g_off, ...)): g itself - what the residual branch
    of a block's last stage reads.  Whatever R the forward added needs no term here: d(z_bn + R) = g for both.  Pad channels
    of every output are exact zeros.  All tensors contiguous float32 with as many rows, at least 2."""
    if g is None and want_g:
        g = torch.empty(y.shape[:-1] + (mean.numel(),), dtype=torch.float32, device=y.device)
    L = lib()
    M, C_real, cp, dz, lds, dgamma, dbeta, ws, ws_bytes = _bn_train_backward(
        "batch_norm_prelu_train_grad", "y", y, (("dy", dy), ("z", z), ("g", g)), mean, invstd, gamma, C_real, dz,
        L.tsod_bn_prelu_train_grad_workspace_bytes)
    num = torch.empty(1, dtype=torch.float32, device=y.device) if want_dslope else None
    check(L.tsod_bn_prelu_train_grad_f32(ptr(y), lds["y"], int(y_off), ptr(dy), lds["dy"], int(dy_off), ptr(z), lds["z"], int(z_off), M,
                                         C_real, cp, ptr(mean), ptr(invstd), ptr(gamma), float(slope), ptr(dz), lds["dz"],
                                         int(dz_off), ptr(dgamma), ptr(dbeta), ptr(num), ptr(g), lds.get("g", 0), int(g_off), ptr(ws),
                                         ws_bytes, stream_ptr()), "bn_prelu_train_grad")
    return dz, dgamma, dbeta, num, g


class _DWConv3x3(torch.autograd.Function):
    """``dwconv3x3_nhwc`` as an autograd node: forward tsod_dwconv3x3_f32, backward tsod_dwconv3x3_grad_f32 (one call gives
    all four gradients; d x is skipped when not asked for, the others are dropped)."""

    @staticmethod
    def forward(ctx, x, w33c, scale, shift, stride, relu):
        xd, wd = x.detach().contiguous(), w33c.detach().contiguous()
        sc = None if scale is None else scale.detach().contiguous()
        sh = None if shift is None else shift.detach().contiguous()
        ctx.save_for_backward(xd, wd, sc, sh)
        ctx.stride, ctx.relu = stride, relu
        with torch.no_grad():
            return dwconv3x3_nhwc(xd, wd, sc, sh, stride, relu)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w, sc, sh = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dw, dscale, dshift = dwconv3x3_grad(x, w, sc, sh, ctx.stride, ctx.relu, gy, want_dx=need[0],
                                                want_params=any(need[1:4]))
        return (dx if need[0] else None, dw if need[1] else None, dscale if need[2] else None,
                dshift if need[3] and sh is not None else None, None, None)


def dropout_key(device, lo: int, hi: int, out=None) -> torch.Tensor:
    """The two 32-bit key words of a dropout mask in device memory (an int32 [2] tensor; ``out``: written in place), by a kernel
    of tsod_dropout_key_set: stream-ordered, no copy, no synchronisation."""
    key = torch.empty(2, dtype=torch.int32, device=device) if out is None else out
    if not key.is_cuda or key.dtype != torch.int32 or key.numel() != 2 or not key.is_contiguous():
        raise ValueError("dropout_key: the key is a contiguous int32 [2] tensor on the GPU")
    check(lib().tsod_dropout_key_set(ptr(key), int(lo) & 0xFFFFFFFF, int(hi) & 0xFFFFFFFF, stream_ptr()), "dropout_key_set")
    return key


def dropout_seg_table(segs):
    """[(channel offset in the pixel, real width, first logical channel)] -> the ``tsod_dropout_seg`` array of the launch."""
    table = (_ffi.DropoutSeg * max(1, len(segs)))()
    for t, (off, real, first) in zip(table, segs):
        t.off, t.real, t.first = int(off), int(real), int(first)
    return table


def dropout(x: torch.Tensor, p: float, key, *, segs=None, C=None, out=None, ordinal: int = 0, e0: int = 0) -> torch.Tensor:
    """Active dropout (tsod_dropout_segs_f32): out = keep ? x / (1 - p) : 0 on channel slices of the NHWC
    tensor x [..., P], the mask from Philox4x32-10 words of every element's index in the LOGICAL tensor [pixels, C].

    ``key``: an int32 [2] device tensor (``dropout_key``) or two ints.  ``segs``: [(channel offset in the pixel, real width, first
    logical channel)], ``C`` the logical channels; default: the whole pixel as one slice (P % 4 == 0).  ``out`` [..., Pd]
    (default: like x, untouched outside the slices - zeros where it is allocated here): ``out is x`` works in place.  Lanes
    between a slice's real and padded width become 0.  The backward is the same call on the gradient with the same key."""
    require_cuda(x, "dropout")
    if not x.is_contiguous() or x.dim() < 2:
        raise ValueError("dropout: x must be a contiguous [..., P] tensor")
    P = x.shape[-1]
    if segs is None:
        segs, C = [(0, P, 0)], P
    if C is None:
        C = sum(real for _, real, _ in segs)
    if out is None:
        out = torch.zeros_like(x)
    require_cuda(out, "dropout")
    if not out.is_contiguous() or out.shape[:-1] != x.shape[:-1]:
        raise ValueError(f"dropout: out must be contiguous with x's leading dimensions, got {tuple(out.shape)} for {tuple(x.shape)}")
    if not isinstance(key, torch.Tensor):
        key = dropout_key(x.device, *key)
    if not key.is_cuda or key.dtype != torch.int32 or key.numel() != 2:
        raise ValueError("dropout: key is an int32 [2] tensor on the GPU or two ints")
    N, H, W = x.shape[:3] if x.dim() == 4 else (1, 1, x.numel() // P)
    check(lib().tsod_dropout_segs_f32(ptr(x), ptr(out), N, H, W, P, out.shape[-1], dropout_seg_table(segs), len(segs), int(C), float(p),
                                      ptr(key), int(ordinal), int(e0), stream_ptr()), "dropout")
    return out


def gconv1x1_pair_grad(x, w_g2, d_out, *, want_dx=True, want_dw=True, want_dbias=True):
    """The backward of ``gconv1x1_pair_nhwc`` (tsod_gconv1x1_pair_grad_f32) -> (d x [..., 2G], dw [G,2], dbias [G]; None where
    not wanted).  x [..., P] with P >= 2G, d_out [..., G] contiguous."""
    require_cuda(x, "gconv1x1_pair_grad")
    G, P = w_g2.shape[0], x.shape[-1]
    pixels = x.numel() // P
    d_out = d_out.contiguous()
    dev = x.device
    dx = torch.empty(tuple(x.shape[:-1]) + (2 * G,), dtype=torch.float32, device=dev) if want_dx else None
    dw = torch.empty((G, 2), dtype=torch.float32, device=dev) if want_dw else None
    db = torch.empty(G, dtype=torch.float32, device=dev) if want_dbias else None
    L = lib()
    ws_bytes = L.tsod_gconv1x1_pair_grad_workspace_bytes(pixels, G)
    ws = ARENA.get(dev, ws_bytes)
    check(L.tsod_gconv1x1_pair_grad_f32(ptr(x), pixels, G, P, ptr(w_g2), ptr(d_out), G, ptr(dx), 2 * G, ptr(dw), ptr(db), ptr(ws),
                                        ws_bytes, stream_ptr()), "gconv1x1_pair_grad")
    return dx, dw, db


class _GConv1x1Pair(torch.autograd.Function):
    """``gconv1x1_pair_nhwc`` as an autograd node (tsod_gconv1x1_pair_f32 / tsod_gconv1x1_pair_grad_f32)."""

    @staticmethod
    def forward(ctx, x, w_g2, bias):
        xd, wd = x.detach().contiguous(), w_g2.detach().contiguous()
        bd = None if bias is None else bias.detach().contiguous()
        ctx.save_for_backward(xd, wd)
        ctx.has_bias = bias is not None
        with torch.no_grad():
            return gconv1x1_pair_nhwc(xd, wd, bd)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dw, db = gconv1x1_pair_grad(x, w, gy, want_dx=need[0], want_dw=need[1], want_dbias=need[2] and ctx.has_bias)
        return dx, dw, db


def gconv1x1_pair_nhwc(x: torch.Tensor, w_g2: torch.Tensor, bias=None) -> torch.Tensor:
    """nn.Conv2d(2G, G, 1, groups=G) on NHWC x [N,H,W,P >= 2G]; w_g2 is [G,2].  Differentiable in x, w_g2 and bias
    (``_GConv1x1Pair``) when grad mode is on, one of them requires grad and x has exactly 2G channels (a wider x keeps the
    plain, non-differentiable path, as before)."""
    require_cuda(x, "gconv1x1_pair")
    if x.shape[3] == 2 * w_g2.shape[0] and torch.is_grad_enabled() and \
            any(t is not None and t.requires_grad for t in (x, w_g2, bias)):
        return _GConv1x1Pair.apply(x, w_g2, bias)
    N, H, W, P = x.shape
    G = w_g2.shape[0]
    out = torch.empty((N, H, W, G), dtype=torch.float32, device=x.device)
    check(lib().tsod_gconv1x1_pair_f32(ptr(x), N * H * W, G, P, ptr(w_g2), ptr(bias), ptr(out), G, stream_ptr()),
          "gconv1x1_pair")
    return out


# ----------------------------------------------------------------------------- proposal path
def rpn_decode(locs: torch.Tensor, scores: torch.Tensor, anchor_base: torch.Tensor, B, Hf, Wf, feat_stride,
               clamp_x, clamp_y, min_size, want_anchors=False):
    """locs [B*Hf*Wf, 4A] , scores [B*Hf*Wf, 2A] (rows may be slices of a wider buffer: row pitch = stride(0)) ->
    boxes [B,Hf*Wf*A,4], fg [B,n], keys [B,n] (+ anchors [n,4])."""
    require_cuda(locs, "rpn_decode")
    A = anchor_base.shape[0]
    assert locs.stride(1) == 1 and scores.stride(1) == 1 and locs.shape[1] == 4 * A and scores.shape[1] == 2 * A
    n = Hf * Wf * A
    dev = locs.device
    boxes = torch.empty((B, n, 4), dtype=torch.float32, device=dev)
    fg = torch.empty((B, n), dtype=torch.float32, device=dev)
    keys = torch.empty((B, n), dtype=torch.float32, device=dev)
    anchors = torch.empty((n, 4), dtype=torch.float32, device=dev) if want_anchors else None
    check(lib().tsod_rpn_decode_f32(ptr(locs), locs.stride(0), ptr(scores), scores.stride(0), ptr(anchor_base), A, B,
                                    Hf, Wf, feat_stride, float(clamp_x), float(clamp_y), float(min_size), ptr(boxes),
                                    ptr(fg), ptr(keys), ptr(anchors), stream_ptr()), "rpn_decode")
    return boxes, fg, keys, anchors


def proposal_decode(anchor: torch.Tensor, loc: torch.Tensor, score: torch.Tensor, clamp_x, clamp_y, min_size):
    """anchor [n,4], loc [n,4], score [n] -> boxes [n,4] (decoded + clamped), keys [n] (-inf = too small)."""
    require_cuda(loc, "proposal_decode")
    anchor, loc, score = anchor.float().contiguous(), loc.contiguous(), score.contiguous()
    n = loc.shape[0]
    boxes = torch.empty((n, 4), dtype=torch.float32, device=loc.device)
    keys = torch.empty((n,), dtype=torch.float32, device=loc.device)
    check(lib().tsod_proposal_decode_f32(ptr(anchor), ptr(loc), ptr(score), n, float(clamp_x), float(clamp_y),
                                         float(min_size), ptr(boxes), ptr(keys), stream_ptr()), "proposal_decode")
    return boxes, keys


def enumerate_anchors(anchor_base: torch.Tensor, feat_stride: int, height: int, width: int) -> torch.Tensor:
    require_cuda(anchor_base, "enumerate_anchors")
    base = anchor_base.contiguous()
    out = torch.empty((height * width * base.shape[0], 4), dtype=torch.float32, device=base.device)
    check(lib().tsod_enumerate_anchors_f32(ptr(base), base.shape[0], height, width, int(feat_stride), ptr(out),
                                           stream_ptr()), "enumerate_anchors")
    return out


def loc2bbox(src: torch.Tensor, loc: torch.Tensor) -> torch.Tensor:
    require_cuda(loc, "loc2bbox")
    src, loc = src.to(loc.dtype).contiguous(), loc.contiguous()
    out = torch.empty_like(loc)
    if loc.shape[0]:
        check(lib().tsod_loc2bbox_f32(ptr(src), ptr(loc), loc.shape[0], ptr(out), stream_ptr()), "loc2bbox")
    return out


def bbox2loc(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """src [n,4], dst [n,4] xyxy -> offsets [n,4] (tsod_bbox2loc_f32; utils/loc_bbox_iou.py:63-88)."""
    require_cuda(src, "bbox2loc")
    src, dst = src.float().contiguous(), dst.to(src.device, torch.float32).contiguous()
    out = torch.empty_like(src)
    if src.shape[0]:
        check(lib().tsod_bbox2loc_f32(ptr(src), ptr(dst), src.shape[0], ptr(out), stream_ptr()), "bbox2loc")
    return out


def sort_topk_desc(keys: torch.Tensor, boxes: torch.Tensor | None, n_pre: int):
    """keys [B,n] (-inf = filtered), boxes [B,n,4] -> counts [B] i32, idx [B,n_pre] i32,
    boxes_sorted [B,n_pre,4], keys_sorted [B,n_pre]."""
    require_cuda(keys, "sort_topk")
    B, n = keys.shape
    dev = keys.device
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    idx = torch.empty((B, n_pre), dtype=torch.int32, device=dev)
    bs = torch.empty((B, n_pre, 4), dtype=torch.float32, device=dev) if boxes is not None else None
    ks = torch.empty((B, n_pre), dtype=torch.float32, device=dev)
    ws_bytes = lib().tsod_sort_topk_workspace_bytes(B, n, n_pre)
    ws = TOPK_ARENA.get(dev, ws_bytes) if ws_bytes else None          # its own arena: the NMS mask of the same step lives in ARENA
    check(lib().tsod_sort_topk_desc_ws_f32(ptr(keys), ptr(boxes), B, n, n_pre, ptr(counts), ptr(idx), ptr(bs), ptr(ks),
                                           ptr(ws), ws_bytes, stream_ptr()), "sort_topk")
    return counts, idx, bs, ks


def nms_sorted(boxes_sorted: torch.Tensor, counts: torch.Tensor, iou_thr: float, n_post: int, status=None):
    """boxes_sorted [B,n_max,4] in descending-score order, counts [B] i32 ->
    keep_idx [B,n_post] i32, rois [B,n_post,4], n_kept [B] i32, status [1] i32."""
    require_cuda(boxes_sorted, "nms")
    B, n_max, _ = boxes_sorted.shape
    dev = boxes_sorted.device
    keep = torch.empty((B, n_post), dtype=torch.int32, device=dev)
    rois = torch.empty((B, n_post, 4), dtype=torch.float32, device=dev)
    n_kept = torch.empty((B,), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws_bytes = lib().tsod_nms_workspace_bytes(B, n_max)
    ws = ARENA.get(dev, ws_bytes)
    check(lib().tsod_nms_f32(ptr(boxes_sorted), ptr(counts), B, n_max, float(iou_thr), n_post, ptr(keep), ptr(rois),
                             ptr(n_kept), ptr(status), ptr(ws), ws_bytes, stream_ptr()), "nms")
    return keep, rois, n_kept, status


def bbox_iou(a: torch.Tensor, b: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    require_cuda(a, "bbox_iou")
    if a.shape[1] != 4 or b.shape[1] != 4:
        raise IndexError
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    if out.numel():
        check(lib().tsod_bbox_iou_f32(ptr(a), a.shape[0], ptr(b), b.shape[0], float(eps), ptr(out), stream_ptr()),
              "bbox_iou")
    return out


# ----------------------------------------------------------------------------- RoI head
def roi_pool_nhwc(feat: torch.Tensor, rois5: torch.Tensor, output_size=(7, 7), spatial_scale=1.0) -> torch.Tensor:
    """feat [B,Hf,Wf,C] NHWC, rois5 [K,5] -> [K,C,PH,PW] (torchvision layout)."""
    require_cuda(feat, "roi_pool")
    B, Hf, Wf, C = feat.shape
    K = rois5.shape[0]
    PH, PW = output_size
    out = torch.empty((K, C, PH, PW), dtype=torch.float32, device=feat.device)
    check(lib().tsod_roi_pool_f32(ptr(feat), B, Hf, Wf, C, C, ptr(rois5.contiguous()), K, float(spatial_scale), PH, PW,
                                  ptr(out), stream_ptr()), "roi_pool")
    return out


def roi_pool_avg_nhwc(feat: torch.Tensor, rois: torch.Tensor, roi_indices: torch.Tensor, img_h, img_w,
                      output_size=(7, 7), spatial_scale=1.0) -> torch.Tensor:
    """feat [B,Hf,Wf,C], rois [B,R,4] image coords, roi_indices [B] i32 -> [B*R, C]."""
    require_cuda(feat, "roi_pool_avg")
    B, Hf, Wf, C = feat.shape
    R = rois.shape[1]
    PH, PW = output_size
    out = torch.empty((rois.shape[0] * R, C), dtype=torch.float32, device=feat.device)
    check(lib().tsod_roi_pool_avg_f32(ptr(feat), B, Hf, Wf, C, C, ptr(rois.contiguous()),
                                      ptr(roi_indices.to(torch.int32).contiguous()), R, float(img_h), float(img_w),
                                      float(spatial_scale), PH, PW, ptr(out), C, stream_ptr()), "roi_pool_avg")
    return out


def _row_pitch(t: torch.Tensor, width: int) -> int | None:
    """Pitch (floats) of the [B*R, width] row matrix behind a [B,R,width] tensor whose rows may be slices of a wider
    buffer (the fused head GEMM writes both outputs into one [B*R, 408] matrix); None if it is not such a matrix."""
    B, R, w = t.shape
    if w != width or t.stride(2) != 1 or (B > 1 and t.stride(0) != R * t.stride(1)) or t.stride(1) < width:
        return None
    return t.stride(1)


def roi_align_nhwc(feat: torch.Tensor, rois5: torch.Tensor, output_size=(7, 7), spatial_scale=1.0, sampling_ratio=2,
                   aligned=False) -> torch.Tensor:
    """feat [B,Hf,Wf,C] NHWC, rois5 [K,5] -> [K,C,PH,PW] (torchvision.ops.roi_align semantics and layout)."""
    require_cuda(feat, "roi_align")
    B, Hf, Wf, C = feat.shape
    K = rois5.shape[0]
    PH, PW = output_size
    out = torch.empty((K, C, PH, PW), dtype=torch.float32, device=feat.device)
    check(lib().tsod_roi_align_f32(ptr(feat), B, Hf, Wf, C, C, ptr(rois5.contiguous()), K, float(spatial_scale), PH, PW,
                                   int(sampling_ratio), 1 if aligned else 0, ptr(out), stream_ptr()), "roi_align")
    return out


def roi_align_avg_nhwc(feat: torch.Tensor, rois: torch.Tensor, roi_indices: torch.Tensor, img_h, img_w, output_size=(7, 7),
                       spatial_scale=1.0, sampling_ratio=2, aligned=False) -> torch.Tensor:
    """feat [B,Hf,Wf,C], rois [B,R,4] image coords, roi_indices [B] i32 -> [B*R, C] (rescale + RoIAlign + mean over bins)."""
    require_cuda(feat, "roi_align_avg")
    B, Hf, Wf, C = feat.shape
    R = rois.shape[1]
    PH, PW = output_size
    out = torch.empty((rois.shape[0] * R, C), dtype=torch.float32, device=feat.device)
    check(lib().tsod_roi_align_avg_f32(ptr(feat), B, Hf, Wf, C, C, ptr(rois.contiguous()),
                                       ptr(roi_indices.to(torch.int32).contiguous()), R, float(img_h), float(img_w),
                                       float(spatial_scale), PH, PW, int(sampling_ratio), 1 if aligned else 0, ptr(out), C,
                                       stream_ptr()), "roi_align_avg")
    return out


def _grad_target(d_out: torch.Tensor, B: int, Hf: int, Wf: int, C: int, d_feat, what: str):
    if d_out.dim() != 2 or d_out.stride(1) != 1 or d_out.shape[1] < C or d_out.dtype != torch.float32:
        raise ValueError(f"{what}: d_out must be a float32 row matrix [B*R, >= {C}], got {tuple(d_out.shape)}")
    if d_feat is None:
        return torch.empty((B, Hf, Wf, C), dtype=torch.float32, device=d_out.device)
    if (d_feat.dim() != 4 or tuple(d_feat.shape[:3]) != (B, Hf, Wf) or d_feat.shape[3] < C or not d_feat.is_contiguous()
            or d_feat.dtype != torch.float32):
        raise ValueError(f"{what}: d_feat must be a contiguous float32 [{B},{Hf},{Wf},>={C}] tensor, got {tuple(d_feat.shape)}")
    return d_feat


def roi_pool_avg_grad_nhwc(feat: torch.Tensor, rois: torch.Tensor, roi_indices: torch.Tensor, img_h, img_w, d_out: torch.Tensor,
                           output_size=(7, 7), spatial_scale=1.0, d_feat=None, accumulate: bool = False) -> torch.Tensor:
    """The backward of roi_pool_avg_nhwc (tsod_roi_pool_avg_grad_f32): feat [B,Hf,Wf,P] (the forward's input; its first
    C = d_out's columns channels), rois [B,R,4], roi_indices [B], d_out [B*R, >= C] (row pitch = stride(0)) -> d_feat
    [B,Hf,Wf,C'] NHWC (``d_feat`` given: written, or with ``accumulate`` added to, in its first C channels)."""
    require_cuda(feat, "roi_pool_avg_grad")
    B, Hf, Wf, P = feat.shape
    R = rois.shape[1]
    C = P if d_feat is None else min(P, d_feat.shape[3])
    C = min(C, d_out.shape[1])
    PH, PW = output_size
    d_feat = _grad_target(d_out, B, Hf, Wf, C, d_feat, "roi_pool_avg_grad")
    if rois.shape[0] != B:
        raise ValueError(f"roi_pool_avg_grad: {rois.shape[0]} RoI groups for {B} feature maps")
    ws_bytes = lib().tsod_roi_pool_avg_grad_workspace_bytes(B, R, C, PH, PW)
    ws = ARENA.get(feat.device, ws_bytes)
    check(lib().tsod_roi_pool_avg_grad_f32(ptr(feat), B, Hf, Wf, C, P, ptr(rois.contiguous()),
                                           ptr(roi_indices.to(torch.int32).contiguous()), R, float(img_h), float(img_w),
                                           float(spatial_scale), PH, PW, ptr(d_out), d_out.stride(0), ptr(d_feat), d_feat.shape[3],
                                           1 if accumulate else 0, ptr(ws), ws_bytes, stream_ptr()), "roi_pool_avg_grad")
    return d_feat


def roi_align_avg_grad_nhwc(feat_shape, rois: torch.Tensor, roi_indices: torch.Tensor, img_h, img_w, d_out: torch.Tensor,
                            output_size=(7, 7), spatial_scale=1.0, sampling_ratio=2, aligned=False, d_feat=None,
                            accumulate: bool = False) -> torch.Tensor:
    """The backward of roi_align_avg_nhwc (tsod_roi_align_avg_grad_f32): ``feat_shape`` = (B, Hf, Wf, C) of the forward's input
    (its values are not needed), d_out [B*R, >= C] -> d_feat [B,Hf,Wf,C] NHWC (``d_feat`` / ``accumulate`` as for RoIPool)."""
    require_cuda(d_out, "roi_align_avg_grad")
    B, Hf, Wf, C = (int(v) for v in feat_shape)
    C = min(C, d_out.shape[1]) if d_feat is None else min(C, d_out.shape[1], d_feat.shape[3])
    R = rois.shape[1]
    PH, PW = output_size
    d_feat = _grad_target(d_out, B, Hf, Wf, C, d_feat, "roi_align_avg_grad")
    if rois.shape[0] != B:
        raise ValueError(f"roi_align_avg_grad: {rois.shape[0]} RoI groups for {B} feature maps")
    ws_bytes = lib().tsod_roi_align_avg_grad_workspace_bytes(B, R)
    ws = ARENA.get(d_out.device, ws_bytes)
    check(lib().tsod_roi_align_avg_grad_f32(B, Hf, Wf, C, ptr(rois.contiguous()), ptr(roi_indices.to(torch.int32).contiguous()), R,
                                            float(img_h), float(img_w), float(spatial_scale), PH, PW, int(sampling_ratio),
                                            1 if aligned else 0, ptr(d_out), d_out.stride(0), ptr(d_feat), d_feat.shape[3],
                                            1 if accumulate else 0, ptr(ws), ws_bytes, stream_ptr()), "roi_align_avg_grad")
    return d_feat


def detections(cls_locs: torch.Tensor, scores: torch.Tensor, rois: torch.Tensor) -> torch.Tensor:
    """[B,R,4*n_class], [B,R,n_class], [B,R,4] -> [B,R,6] (x1,y1,x2,y2,score,class)."""
    require_cuda(scores, "detections")
    B, R, n_class = scores.shape
    lp, sp = _row_pitch(cls_locs, 4 * n_class), _row_pitch(scores, n_class)
    if lp is None:
        cls_locs, lp = cls_locs.contiguous(), 4 * n_class
    if sp is None:
        scores, sp = scores.contiguous(), n_class
    out = torch.empty((B, R, 6), dtype=torch.float32, device=scores.device)
    check(lib().tsod_detections_f32(ptr(cls_locs), lp, ptr(scores), sp, ptr(rois.contiguous()), B * R, n_class, ptr(out),
                                    stream_ptr()), "detections")
    return out


def filter_detections(det: torch.Tensor, iou_thr: float = 0.1, score_thresh: float | None = None, per_class: bool = False,
                      background_class: int = -1):
    """Inference-time filtering of detection records [B,R,6] (multi_inference.py:80-87 + the two deployment switches):
    drop records below ``score_thresh`` / of ``background_class``, order by descending score (stable), greedy NMS
    (class-agnostic like the reference's demo, or per class).  Returns (det_sorted [B,R,6], keep [B,R] i32 rows of
    det_sorted in score order with -1 after n_kept[b], n_kept [B] i32)."""
    require_cuda(det, "filter_detections")
    det = det.contiguous()
    B, R, six = det.shape
    if six != 6:
        raise ValueError("detection records are [B,R,6]")
    dev = det.device
    L = lib()
    keys = torch.empty((B, R), dtype=torch.float32, device=dev)
    thr = float("-inf") if score_thresh is None else float(score_thresh)
    check(L.tsod_detection_keys_f32(ptr(det), B * R, thr, int(background_class), ptr(keys), stream_ptr()), "detection_keys")
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    idx = torch.empty((B, R), dtype=torch.int32, device=dev)
    ws_bytes = L.tsod_sort_topk_workspace_bytes(B, R, R)
    ws_sort = TOPK_ARENA.get(dev, ws_bytes) if ws_bytes else None
    check(L.tsod_sort_topk_desc_ws_f32(ptr(keys), None, B, R, R, ptr(counts), ptr(idx), None, None, ptr(ws_sort), ws_bytes,
                                       stream_ptr()), "sort_topk")
    det_sorted = torch.empty_like(det)
    check(L.tsod_gather_rows_f32(ptr(det), ptr(idx), B, R, R, 6, ptr(det_sorted), stream_ptr()), "gather_rows")
    keep = torch.empty((B, R), dtype=torch.int32, device=dev)
    n_kept = torch.empty((B,), dtype=torch.int32, device=dev)
    ws_bytes = L.tsod_nms_workspace_bytes(B, R)
    ws = ARENA.get(dev, ws_bytes)
    check(L.tsod_detection_nms_f32(ptr(det_sorted), ptr(counts), B, R, float(iou_thr), 1 if per_class else 0, ptr(keep),
                                   ptr(n_kept), ptr(ws), ws_bytes, stream_ptr()), "detection_nms")
    return det_sorted, keep, n_kept


# ----------------------------------------------------------------------------- detection mAP
EVAL_RECORD_INTS = 3                 # tsod_eval_record = (score f32, class i32, TP mask u32), one int32 row of three
EVAL_ARENA = _Arena()                # the evaluator's staging slots and sort / accumulate scratch


def _require_cuda_any(t, what: str, dtype) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _ffi.TsodError(f"{what}: this package is a HIP-only path and needs a CUDA/ROCm tensor "
                             "(the CPU restatement lives under oracle/ and is test infrastructure only)")
    if t.dtype != dtype:
        raise _ffi.TsodError(f"{what}: {dtype} required, got {t.dtype}")


def sort_pairs_u64(keys: torch.Tensor, vals: torch.Tensor | None = None, begin_bit: int = 0, end_bit: int = 64,
                   n_dev: torch.Tensor | None = None):
    """Stable ascending radix sort (tsod_sort_pairs_u64) of keys [n] int64 holding u64 bit patterns on bits
    [begin_bit, end_bit), with vals [n] int32 (None: 0..n-1).  ``n_dev`` (int64 [1] on the device) limits the live count
    without a host read; entries past it are left as they are.  -> (keys_sorted [n] int64, vals_sorted [n] int32)."""
    _require_cuda_any(keys, "sort_pairs_u64", torch.int64)
    if keys.dim() != 1:
        raise ValueError(f"sort_pairs_u64: keys must be [n], got {tuple(keys.shape)}")
    keys = keys.contiguous()
    n, dev = keys.shape[0], keys.device
    if vals is not None:
        _require_cuda_any(vals, "sort_pairs_u64", torch.int32)
        if tuple(vals.shape) != (n,):
            raise ValueError(f"sort_pairs_u64: vals {tuple(vals.shape)} for {n} keys")
        vals = vals.contiguous()
    keys_out = torch.empty_like(keys)
    vals_out = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return keys_out, vals_out
    L = lib()
    ws_bytes = L.tsod_sort_pairs_workspace_bytes(n)
    ws = EVAL_ARENA.get(dev, ws_bytes)
    check(L.tsod_sort_pairs_u64(ptr(keys), ptr(vals), n, ptr(n_dev), int(begin_bit), int(end_bit), ptr(keys_out), ptr(vals_out),
                                ptr(ws), ws_bytes, stream_ptr()), "sort_pairs_u64")
    return keys_out, vals_out


def _eval_match_args(what: str, workspace_bytes, det, gt_boxes, gt_labels, gt_counts, counts, keep, n_kept, per_gt=()):
    """The checks and arguments both match entry points share -> (the arguments up to G, the trailing workspace arguments).
    ``per_gt``: (name, [B,G] tensor or None, dtype) of the arrays an entry point takes beside gt_counts."""
    require_cuda(det, what)
    B, R, six = det.shape
    if six != 6:
        raise ValueError(f"{what}: detection records are [B,R,6], got {tuple(det.shape)}")
    G = gt_boxes.shape[1]
    for name, x, dtype in per_gt:
        if x is not None:
            _require_cuda_any(x, f"{what}: {name}", dtype)
            if tuple(x.shape) != (B, G) or not x.is_contiguous():
                raise ValueError(f"{what}: {name} must be a contiguous [{B},{G}] tensor, got {tuple(x.shape)}")
    ws_bytes = workspace_bytes(B, R)
    ws = EVAL_ARENA.get(det.device, ws_bytes)
    gt = [ptr(x) if G else None for x in (gt_boxes, gt_labels, gt_counts, *(x for _, x, _ in per_gt))]
    return (ptr(det), B, R, ptr(counts), ptr(keep), ptr(n_kept), *gt, G), (ptr(ws), ws_bytes, stream_ptr())


def eval_match(det: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_counts: torch.Tensor,
               iou_thr: torch.Tensor, num_classes: int, max_dets: int, ignore_class: int, records: torch.Tensor,
               n_records: torch.Tensor, npig: torch.Tensor, *, counts=None, keep=None, n_kept=None) -> None:
    """One update of the evaluator's device state (tsod_eval_match_f32): det [B,R,6] with counts [B] int32 or keep [B,R] +
    n_kept [B] int32; gt_boxes [B,G,4] f32, gt_labels [B,G] int64, gt_counts [B] int32; iou_thr [T] f32.  Appends to
    records [capacity,3] int32 at n_records [1] int64 and adds to npig [num_classes] int64, in place."""
    L = lib()
    head, tail = _eval_match_args("eval_match", L.tsod_eval_match_workspace_bytes, det, gt_boxes, gt_labels, gt_counts, counts,
                                  keep, n_kept)
    check(L.tsod_eval_match_f32(*head, ptr(iou_thr), iou_thr.shape[0], int(num_classes), int(max_dets), int(ignore_class),
                                ptr(records), records.shape[0], ptr(n_records), ptr(npig), *tail), "eval_match")


def _eval_accumulate(what: str, workspace_bytes, entry, records, n_records, npig, cells, shape) -> torch.Tensor:
    """One accumulate entry point over every record so far -> one int64 tensor [5, *shape] on the device: the bits of AP
    (f64), TP, FP, FN, the bits of recall (f64), in that order (one buffer, so the caller reads the results with one copy).
    ``cells``: the entry point's arguments between npig and its outputs."""
    out = torch.empty((5, *shape), dtype=torch.int64, device=records.device)
    ws_bytes = workspace_bytes(records.shape[0], shape[0])
    ws = EVAL_ARENA.get(records.device, ws_bytes)
    check(entry(ptr(records), records.shape[0], ptr(n_records), ptr(npig), *cells, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                ptr(out[3]), ptr(out[4]), ptr(ws), ws_bytes, stream_ptr()), what)
    return out


def eval_accumulate(records: torch.Tensor, n_records: torch.Tensor, npig: torch.Tensor, T: int) -> torch.Tensor:
    """tsod_eval_accumulate_f64 over every record so far -> one int64 tensor [5, C, T] on the device: the bits of AP (f64),
    TP, FP, FN, the bits of recall (f64), in that order (one buffer, so the caller reads the results with one copy)."""
    C = npig.shape[0]
    L = lib()
    return _eval_accumulate("eval_accumulate", L.tsod_eval_accumulate_workspace_bytes, L.tsod_eval_accumulate_f64, records,
                            n_records, npig, (C, int(T)), (C, T))


EVAL_COCO_RECORD_INTS = 11           # tsod_eval_record_coco = (score f32, class, rank, tp_mask[4], ig_mask[4]), int32 rows
EVAL_COCO_MAX_AREAS = 4              # area ranges of one match / words of a record's masks
EVAL_COCO_MAX_CAPS = 4               # detection caps of one accumulate


def eval_match_coco(det: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_counts: torch.Tensor,
                    iou_thr: torch.Tensor, area_lo: torch.Tensor, area_hi: torch.Tensor, num_classes: int, max_dets: int,
                    ignore_class: int, records: torch.Tensor, n_records: torch.Tensor, npig: torch.Tensor, *, gt_crowd=None,
                    gt_area=None, counts=None, keep=None, n_kept=None) -> None:
    """One update of the COCO evaluator's device state (tsod_eval_match_coco_f32): eval_match's inputs plus gt_crowd [B,G]
    uint8 and gt_area [B,G] f32 (either may be None) and the area ranges area_lo / area_hi [A] f32 on the device.  Appends to
    records [capacity,11] int32 at n_records [1] int64 and adds to npig [num_classes,A] int64, in place."""
    L = lib()
    head, tail = _eval_match_args("eval_match_coco", L.tsod_eval_match_coco_workspace_bytes, det, gt_boxes, gt_labels,
                                  gt_counts, counts, keep, n_kept,
                                  per_gt=(("gt_crowd", gt_crowd, torch.uint8), ("gt_area", gt_area, torch.float32)))
    check(L.tsod_eval_match_coco_f32(*head, ptr(iou_thr), iou_thr.shape[0], ptr(area_lo), ptr(area_hi), area_lo.shape[0],
                                     int(num_classes), int(max_dets), int(ignore_class), ptr(records), records.shape[0],
                                     ptr(n_records), ptr(npig), *tail), "eval_match_coco")


def eval_accumulate_coco(records: torch.Tensor, n_records: torch.Tensor, npig: torch.Tensor, T: int, max_dets_list,
                         max_dets: int) -> torch.Tensor:
    """tsod_eval_accumulate_coco_f64 over every record so far -> one int64 tensor [5, C, A, M, T] on the device: the bits of
    AP (f64), TP, FP, FN, the bits of recall (f64), in that order.  npig [C,A]; max_dets_list: the M ascending caps (host
    ints), the last at most ``max_dets``, the cap the records were matched with."""
    C, A = npig.shape
    caps = (c_int32 * len(max_dets_list))(*[int(m) for m in max_dets_list])
    M = len(caps)
    L = lib()
    return _eval_accumulate("eval_accumulate_coco", L.tsod_eval_accumulate_coco_workspace_bytes,
                            L.tsod_eval_accumulate_coco_f64, records, n_records, npig, (C, A, int(T), caps, M, int(max_dets)),
                            (C, A, M, int(T)))


# ----------------------------------------------------------------------------- training-side box ops
def anchor_targets(bbox: torch.Tensor, anchor: torch.Tensor, n_pos: int, n_sample: int, pos_iou_thresh: float,
                   neg_iou_thresh: float):
    """anchor [A,4], bbox [G,4] -> (loc [A,4] f32, label [A] int64, argmax [A] int32) (tsod_anchor_targets_f32)."""
    require_cuda(anchor, "anchor_targets")
    anchor, bbox = anchor.contiguous(), bbox.to(anchor.device, torch.float32).contiguous()
    A, G = anchor.shape[0], bbox.shape[0]
    dev = anchor.device
    loc = torch.empty((A, 4), dtype=torch.float32, device=dev)
    label = torch.empty((A,), dtype=torch.int64, device=dev)
    argmax = torch.empty((A,), dtype=torch.int32, device=dev)
    ws_bytes = lib().tsod_anchor_targets_workspace_bytes(A, G)
    ws = ARENA.get(dev, ws_bytes)
    check(lib().tsod_anchor_targets_f32(ptr(anchor), A, ptr(bbox) if G else None, G, float(pos_iou_thresh),
                                        float(neg_iou_thresh), int(n_pos), int(n_sample), ptr(loc), ptr(label), ptr(argmax),
                                        ptr(ws), ws_bytes, stream_ptr()), "anchor_targets")
    return loc, label, argmax


def _proposal_outputs(lead: tuple, n_sample: int, dev, want_src: bool):
    """The uninitialised outputs of a proposal-target call, ``lead`` = () or (B,): (sample_roi [..., n_sample, 4],
    gt_roi_loc [..., n_sample, 4], gt_roi_label [..., n_sample] int64, counts [..., 4] int32, sample_src [..., n_sample] int32
    or None)."""
    return (torch.empty((*lead, n_sample, 4), dtype=torch.float32, device=dev),
            torch.empty((*lead, n_sample, 4), dtype=torch.float32, device=dev),
            torch.empty((*lead, n_sample), dtype=torch.int64, device=dev),
            torch.empty((*lead, 4), dtype=torch.int32, device=dev),
            torch.empty((*lead, n_sample), dtype=torch.int32, device=dev) if want_src else None)


def _proposal_targets(what: str, want_src: bool, roi, bbox, label, n_sample, pos_per_image, pos_iou_thresh, neg_iou_thresh_high,
                      neg_iou_thresh_low):
    """One image through tsod_proposal_targets_f32 or, with ``want_src``, tsod_proposal_targets_src_f32, which takes
    sample_src after counts -> (sample_roi, gt_roi_loc, gt_roi_label, counts, sample_src or None)."""
    require_cuda(roi, what)
    dev = roi.device
    roi, bbox = roi.contiguous(), bbox.to(dev, torch.float32).contiguous()
    label = label.to(dev, torch.int64).contiguous()
    R, G = roi.shape[0], bbox.shape[0]
    out = _proposal_outputs((), n_sample, dev, want_src)
    ws_bytes = lib().tsod_proposal_targets_workspace_bytes(R, G, n_sample)
    ws = ARENA.get(dev, ws_bytes)
    entry = lib().tsod_proposal_targets_src_f32 if want_src else lib().tsod_proposal_targets_f32
    check(entry(ptr(roi) if R else None, R, ptr(bbox) if G else None, G, ptr(label) if G else None, int(n_sample),
                int(pos_per_image), float(pos_iou_thresh), float(neg_iou_thresh_high), float(neg_iou_thresh_low),
                *(ptr(t) for t in out if t is not None), ptr(ws), ws_bytes, stream_ptr()), what)
    return out


def proposal_targets(roi: torch.Tensor, bbox: torch.Tensor, label: torch.Tensor, n_sample: int, pos_per_image: int,
                     pos_iou_thresh: float, neg_iou_thresh_high: float, neg_iou_thresh_low: float):
    """roi [R,4], bbox [G,4], label [G] int64 -> (sample_roi [n_sample,4], gt_roi_loc [n_sample,4], gt_roi_label [n_sample]
    int64, counts [4] int32 = (rows kept, positives, negatives, status)) (tsod_proposal_targets_f32)."""
    return _proposal_targets("proposal_targets", False, roi, bbox, label, n_sample, pos_per_image, pos_iou_thresh,
                             neg_iou_thresh_high, neg_iou_thresh_low)[:4]


def _batch_ground_truth(what: str, bbox: torch.Tensor, gt_counts: torch.Tensor, dev):
    """Padded ground truth of a batched target call -> (bbox [B,Gmax,4] f32 contiguous, gt_counts [B] int32, B, Gmax), on ``dev``."""
    if bbox.dim() != 3 or bbox.shape[2] != 4:
        raise ValueError(f"{what}: bbox must be padded ground truth [B,Gmax,4], got {tuple(bbox.shape)}")
    B, Gmax = bbox.shape[:2]
    if not isinstance(gt_counts, torch.Tensor) or not gt_counts.is_cuda or tuple(gt_counts.shape) != (B,):
        raise ValueError(f"{what}: gt_counts must be a [B={B}] integer tensor on the GPU (the kernels read it there)")
    return bbox.to(dev, torch.float32).contiguous(), gt_counts.to(dev, torch.int32).contiguous(), B, Gmax


def anchor_targets_batch(bbox: torch.Tensor, gt_counts: torch.Tensor, anchor: torch.Tensor, n_pos: int, n_sample: int,
                         pos_iou_thresh: float, neg_iou_thresh: float):
    """``anchor_targets`` for a whole batch in four launches (tsod_anchor_targets_batch_f32): anchor [A,4] shared by the
    batch, bbox [B,Gmax,4] padded, gt_counts [B] int32 on the device (read there, clamped to [0, Gmax]; pad rows are never
    read) -> (loc [B,A,4] f32, label [B,A] int64, argmax [B,A] int32).  Image b's rows are bit for bit
    ``anchor_targets(bbox[b, :gt_counts[b]], anchor, ...)``.  No host synchronisation."""
    require_cuda(anchor, "anchor_targets_batch")
    dev = anchor.device
    anchor = anchor.contiguous()
    bbox, gt_counts, B, Gmax = _batch_ground_truth("anchor_targets_batch", bbox, gt_counts, dev)
    A = anchor.shape[0]
    loc = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    label = torch.empty((B, A), dtype=torch.int64, device=dev)
    argmax = torch.empty((B, A), dtype=torch.int32, device=dev)
    ws_bytes = lib().tsod_anchor_targets_batch_workspace_bytes(B, A, Gmax)
    ws = ARENA.get(dev, ws_bytes)
    check(lib().tsod_anchor_targets_batch_f32(ptr(anchor), A, ptr(bbox) if Gmax else None, ptr(gt_counts) if Gmax else None, B,
                                              Gmax, float(pos_iou_thresh), float(neg_iou_thresh), int(n_pos), int(n_sample),
                                              ptr(loc), ptr(label), ptr(argmax), ptr(ws), ws_bytes, stream_ptr()),
          "anchor_targets_batch")
    return loc, label, argmax


def proposal_targets_batch(roi: torch.Tensor, bbox: torch.Tensor, label: torch.Tensor, gt_counts: torch.Tensor, n_sample: int,
                           pos_per_image: int, pos_iou_thresh: float, neg_iou_thresh_high: float, neg_iou_thresh_low: float,
                           want_src: bool = False):
    """``proposal_targets`` / ``proposal_targets_src`` for a whole batch in two launches (tsod_proposal_targets_batch_f32):
    roi [B,R,4], bbox [B,Gmax,4] and label [B,Gmax] padded, gt_counts [B] int32 on the device ->
    (sample_roi [B,n_sample,4], gt_roi_loc [B,n_sample,4], gt_roi_label [B,n_sample] int64, counts [B,4] int32 = per image
    (rows kept, positives, negatives, status), sample_src [B,n_sample] int32 or None).  The first counts[b,0] rows of image b
    are bit for bit the single-image call's; the rows behind them are zeros (-1 in sample_src) - the single-image calls leave
    those untouched.  Nothing is read back: ``counts`` stays on the device."""
    require_cuda(roi, "proposal_targets_batch")
    dev = roi.device
    if roi.dim() != 3 or roi.shape[2] != 4:
        raise ValueError(f"proposal_targets_batch: roi must be [B,R,4], got {tuple(roi.shape)}")
    roi = roi.contiguous()
    bbox, gt_counts, B, Gmax = _batch_ground_truth("proposal_targets_batch", bbox, gt_counts, dev)
    if roi.shape[0] != B or tuple(label.shape) != (B, Gmax):
        raise ValueError(f"proposal_targets_batch: roi {tuple(roi.shape)} / label {tuple(label.shape)} for bbox {tuple(bbox.shape)}")
    label = label.to(dev, torch.int64).contiguous()
    R = roi.shape[1]
    sample_roi, gt_roi_loc, gt_roi_label, counts, src = _proposal_outputs((B,), n_sample, dev, want_src)
    ws_bytes = lib().tsod_proposal_targets_batch_workspace_bytes(B, R, Gmax, n_sample)
    ws = ARENA.get(dev, ws_bytes)
    gt = [ptr(t) if Gmax else None for t in (bbox, label, gt_counts)]
    check(lib().tsod_proposal_targets_batch_f32(ptr(roi) if R else None, R, *gt, B, Gmax, int(n_sample), int(pos_per_image),
                                                float(pos_iou_thresh), float(neg_iou_thresh_high), float(neg_iou_thresh_low),
                                                ptr(sample_roi), ptr(gt_roi_loc), ptr(gt_roi_label), ptr(counts),
                                                ptr(src) if want_src else None, ptr(ws), ws_bytes, stream_ptr()),
          "proposal_targets_batch")
    return sample_roi, gt_roi_loc, gt_roi_label, counts, src


def rpn_losses(rpn_out: torch.Tensor, A: int, gt_loc: torch.Tensor, gt_label: torch.Tensor, sigma: float = 1.0):
    """The RPN's two losses per image (tsod_rpn_losses_f32; nets/frcnn_training.py:220-238, 262-274).
    rpn_out [B*h*w, >= 6A] with row stride = pitch: the fused loc + score conv output (``RegionProposalNetwork.propose``),
    read in place; gt_loc [B, h*w*A, 4] f32, gt_label [B, h*w*A] int64 (-1 / 0 / 1) ->
    (out [B,2] f32 = (loc loss, cls loss), status [B] int32 = labels outside {-1, 0, 1})."""
    require_cuda(rpn_out, "rpn_losses")
    B, n = gt_label.shape
    if rpn_out.dim() != 2 or rpn_out.stride(1) != 1 or rpn_out.shape[1] < 6 * A or n % A or rpn_out.shape[0] != B * (n // A):
        raise ValueError(f"rpn_losses: rpn_out {tuple(rpn_out.shape)} does not hold B={B} images of {n} anchors at A={A}")
    if tuple(gt_loc.shape) != (B, n, 4):
        raise ValueError(f"rpn_losses: gt_loc {tuple(gt_loc.shape)}, expected {(B, n, 4)}")
    dev = rpn_out.device
    gt_loc = gt_loc.to(dev, torch.float32).contiguous()
    gt_label = gt_label.to(dev, torch.int64).contiguous()
    out = torch.empty((B, 2), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().tsod_rpn_losses_f32(ptr(rpn_out), rpn_out.stride(0), int(A), B, n // A, ptr(gt_loc), ptr(gt_label),
                                    float(sigma), ptr(out), ptr(status), stream_ptr()), "rpn_losses")
    return out, status


def roi_losses(cls_locs: torch.Tensor, scores: torch.Tensor, sample_roi: torch.Tensor, gt_roi_loc: torch.Tensor,
               gt_roi_label: torch.Tensor, sigma: float = 1.0):
    """The head's predictions and two losses per image (tsod_roi_losses_f32; nets/frcnn_training.py:300-331).
    cls_locs [B,S,4*n_class], scores [B,S,n_class] (rows may be slices of the fused head GEMM's output, as for
    ``detections``), sample_roi / gt_roi_loc [B,S,4], gt_roi_label [B,S] int64 ->
    (anchors_pred [B,S,4], classes_pred [B,S] int64, classes_score_pred [B,S], out [B,2] = (loc loss, cls loss),
    status [B] int32 = labels outside [0, n_class))."""
    require_cuda(scores, "roi_losses")
    B, S, n_class = scores.shape
    if tuple(cls_locs.shape) != (B, S, 4 * n_class):
        raise ValueError(f"roi_losses: cls_locs {tuple(cls_locs.shape)}, expected {(B, S, 4 * n_class)}")
    for name, t, shp in (("sample_roi", sample_roi, (B, S, 4)), ("gt_roi_loc", gt_roi_loc, (B, S, 4)),
                         ("gt_roi_label", gt_roi_label, (B, S))):
        if tuple(t.shape) != shp:
            raise ValueError(f"roi_losses: {name} {tuple(t.shape)}, expected {shp}")
    dev = scores.device
    lp, sp = _row_pitch(cls_locs, 4 * n_class), _row_pitch(scores, n_class)
    if lp is None:
        cls_locs, lp = cls_locs.contiguous(), 4 * n_class
    if sp is None:
        scores, sp = scores.contiguous(), n_class
    sample_roi = sample_roi.to(dev, torch.float32).contiguous()
    gt_roi_loc = gt_roi_loc.to(dev, torch.float32).contiguous()
    gt_roi_label = gt_roi_label.to(dev, torch.int64).contiguous()
    anchors_pred = torch.empty((B, S, 4), dtype=torch.float32, device=dev)
    classes_pred = torch.empty((B, S), dtype=torch.int64, device=dev)
    classes_score_pred = torch.empty((B, S), dtype=torch.float32, device=dev)
    out = torch.empty((B, 2), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().tsod_roi_losses_f32(ptr(cls_locs), lp, ptr(scores), sp, ptr(sample_roi), ptr(gt_roi_loc), ptr(gt_roi_label), B, S,
                                    n_class, float(sigma), ptr(anchors_pred), ptr(classes_pred), ptr(classes_score_pred),
                                    ptr(out), ptr(status), stream_ptr()), "roi_losses")
    return anchors_pred, classes_pred, classes_score_pred, out, status


# ----------------------------------------------------------------------------- head gradients (FasterRCNNTrainer(head_grads=True))
def proposal_targets_src(roi: torch.Tensor, bbox: torch.Tensor, label: torch.Tensor, n_sample: int, pos_per_image: int,
                         pos_iou_thresh: float, neg_iou_thresh_high: float, neg_iou_thresh_low: float):
    """``proposal_targets`` plus sample_src [n_sample] int32: the row of cat(roi, bbox) each sample came from (< R: a
    proposal; the reference's keep_index) (tsod_proposal_targets_src_f32)."""
    return _proposal_targets("proposal_targets_src", True, roi, bbox, label, n_sample, pos_per_image, pos_iou_thresh,
                             neg_iou_thresh_high, neg_iou_thresh_low)


def _upstream(up: torch.Tensor) -> torch.Tensor:
    up = up.to(torch.float32).contiguous()
    if up.numel() != 5:
        raise ValueError(f"upstream gradients: 5 values (rpn_loc, rpn_cls, roi_loc, roi_cls, total), got {up.numel()}")
    return up


def rpn_losses_grad(rpn_out: torch.Tensor, A: int, gt_loc: torch.Tensor, gt_label: torch.Tensor, sigma: float,
                    up: torch.Tensor, inv_B: float):
    """d (the two RPN losses) / d rpn_out (tsod_rpn_losses_grad_f32): rpn_out [B*h*w, pitch] as for ``rpn_losses``, ``up`` [5]
    device upstream gradients -> (d_rpn_out [B*h*w, pitch] (zero pad columns), n_rows [B,2] int32 = (positives, counted))."""
    require_cuda(rpn_out, "rpn_losses_grad")
    B, n = gt_label.shape
    if rpn_out.dim() != 2 or rpn_out.stride(1) != 1 or rpn_out.shape[1] < 6 * A or n % A or rpn_out.shape[0] != B * (n // A):
        raise ValueError(f"rpn_losses_grad: rpn_out {tuple(rpn_out.shape)} does not hold B={B} images of {n} anchors at A={A}")
    dev = rpn_out.device
    gt_loc = gt_loc.to(dev, torch.float32).contiguous()
    gt_label = gt_label.to(dev, torch.int64).contiguous()
    pitch = rpn_out.shape[1]
    d = torch.empty((rpn_out.shape[0], pitch), dtype=torch.float32, device=dev)
    n_rows = torch.empty((B, 2), dtype=torch.int32, device=dev)
    check(lib().tsod_rpn_losses_grad_f32(ptr(rpn_out), rpn_out.stride(0), int(A), B, n // A, ptr(gt_loc), ptr(gt_label),
                                         float(sigma), ptr(_upstream(up)), float(inv_B), ptr(n_rows), ptr(d), pitch,
                                         stream_ptr()), "rpn_losses_grad")
    return d, n_rows


def roi_losses_grad(both: torch.Tensor, n_class: int, sample_roi: torch.Tensor, gt_roi_loc: torch.Tensor,
                    gt_roi_label: torch.Tensor, sigma: float, up: torch.Tensor, inv_B: float):
    """d (the two head losses) / d both, d sample_roi (tsod_roi_losses_grad_f32).  ``both`` [B*S, pitch]: the fused head GEMM's
    output (cls_loc columns [0, 4 n_class), scores [4 n_class, 5 n_class)); sample_roi / gt_roi_loc [B,S,4], gt_roi_label [B,S]
    -> (d_both [B*S, pitch] (zero pad columns), d_sample_roi [B,S,4])."""
    require_cuda(both, "roi_losses_grad")
    B, S = gt_roi_label.shape
    if both.dim() != 2 or both.stride(1) != 1 or both.shape[0] != B * S or both.shape[1] < 5 * n_class:
        raise ValueError(f"roi_losses_grad: both {tuple(both.shape)} does not hold {B}x{S} rows of {5 * n_class} columns")
    dev = both.device
    sample_roi = sample_roi.to(dev, torch.float32).contiguous()
    gt_roi_loc = gt_roi_loc.to(dev, torch.float32).contiguous()
    gt_roi_label = gt_roi_label.to(dev, torch.int64).contiguous()
    pitch = both.shape[1]
    d = torch.empty((B * S, pitch), dtype=torch.float32, device=dev)
    d_roi = torch.empty((B, S, 4), dtype=torch.float32, device=dev)
    check(lib().tsod_roi_losses_grad_f32(ptr(both), both.stride(0), ptr(both[:, 4 * n_class:]), both.stride(0), ptr(sample_roi),
                                         ptr(gt_roi_loc), ptr(gt_roi_label), B, S, int(n_class), float(sigma),
                                         ptr(_upstream(up)), float(inv_B), ptr(d), pitch, ptr(d_roi), stream_ptr()),
          "roi_losses_grad")
    return d, d_roi


def rpn_roi_scatter(d_rpn_out: torch.Tensor, d_sample_roi: torch.Tensor, sample_src: torch.Tensor, keep_idx: torch.Tensor,
                    sort_idx: torch.Tensor, rpn_out: torch.Tensor, anchors: torch.Tensor, A: int, clamp_x, clamp_y):
    """Add d sample_roi into the loc columns of ``d_rpn_out`` (in place) along sample_src [B,S] -> keep_idx [B,R] ->
    sort_idx [B,n_pre] -> anchor, through the clamp mask and loc2bbox's backward (tsod_rpn_roi_scatter_f32)."""
    require_cuda(d_rpn_out, "rpn_roi_scatter")
    B, S = sample_src.shape
    R, n_pre = keep_idx.shape[1], sort_idx.shape[1]
    n_pix = rpn_out.shape[0] // B
    for name, v in (("sample_src", sample_src), ("keep_idx", keep_idx), ("sort_idx", sort_idx)):
        if v.dtype != torch.int32 or not v.is_contiguous() or v.shape[0] != B:
            raise ValueError(f"rpn_roi_scatter: {name} must be contiguous int32 [B, ...], got {v.dtype} {tuple(v.shape)}")
    if tuple(d_sample_roi.shape) != (B, S, 4) or anchors.shape[0] != n_pix * A or d_rpn_out.shape[0] != rpn_out.shape[0]:
        raise ValueError("rpn_roi_scatter: inconsistent shapes")
    check(lib().tsod_rpn_roi_scatter_f32(ptr(d_sample_roi.contiguous()), ptr(sample_src), B, S, R, ptr(keep_idx), ptr(sort_idx),
                                         n_pre, ptr(rpn_out), rpn_out.stride(0), ptr(anchors.contiguous()), int(A), n_pix,
                                         float(clamp_x), float(clamp_y), ptr(d_rpn_out), d_rpn_out.stride(0), stream_ptr()),
          "rpn_roi_scatter")
    return d_rpn_out


def wgrad(dy: torch.Tensor, x: torch.Tensor, dw0: torch.Tensor, db0=None, dw1=None, db1=None, accumulate: bool = False):
    """dW = dy^T x, db = dy summed over rows, on the f32 matrix cores (tsod_wgrad_f32).  dy [M, >= N] (row pitch = stride(0)),
    x [M, K] (rows may be pitched; 16-byte aligned).  Rows [0, n0) of the [N, K] result go to ``dw0`` [n0, K] / ``db0`` [n0],
    the next n1 rows to ``dw1`` / ``db1`` (N = dy.shape[1]; later rows are dropped).  ``accumulate``: add instead of write."""
    require_cuda(dy, "wgrad")
    if dy.dim() != 2 or x.dim() != 2 or dy.stride(1) != 1 or x.stride(1) != 1 or dy.shape[0] != x.shape[0]:
        raise ValueError(f"wgrad: dy {tuple(dy.shape)} and x {tuple(x.shape)} must be row matrices with the same rows")
    M, N = dy.shape
    K = x.shape[1]
    n0 = dw0.numel() // K
    n1 = 0 if dw1 is None else dw1.numel() // K
    for t in (dw0, db0, dw1, db1):
        if t is not None and (not t.is_contiguous() or t.dtype != torch.float32):
            raise ValueError("wgrad: outputs must be contiguous float32")
    ws_bytes = lib().tsod_wgrad_workspace_bytes(M, N, K)
    ws = ARENA.get(dy.device, ws_bytes)
    check(lib().tsod_wgrad_f32(ptr(dy), M, N, dy.stride(0), ptr(x), K, x.stride(0), n0, ptr(dw0), ptr(db0), n1, ptr(dw1),
                               ptr(db1), 1 if accumulate else 0, ptr(ws), ws_bytes, stream_ptr()), "wgrad")


# ----------------------------------------------------------------------------- input step
_RESIZE_TABLES: dict = {}


def resize_tables(n_in: int, n_out: int, device):
    """(first [n_out] i32, count [n_out] i32, weights [n_out,taps] f32) of one axis on ``device``; computed by the
    library's host function once per (n_in, n_out, device)."""
    import numpy as np
    key = (int(n_in), int(n_out), torch.device(device))
    t = _RESIZE_TABLES.get(key)
    if t is None:
        L = lib()
        taps = L.tsod_resize_aa_taps(n_in, n_out)
        first = np.zeros(n_out, np.int32)
        count = np.zeros(n_out, np.int32)
        w = np.zeros((n_out, taps), np.float32)
        check(L.tsod_resize_aa_tables_f32(n_in, n_out, first.ctypes.data, count.ctypes.data, w.ctypes.data), "resize_tables")
        t = _RESIZE_TABLES[key] = tuple(torch.from_numpy(a).to(device) for a in (first, count, w))
    return t


def _out_tensor(out, shape, dev, what):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise TsodError(f"{what}: out must be a contiguous f32 {shape} tensor on {dev}")
    return out


def _layout(layout, C, OH, OW):
    if layout == "nhwc4":
        return (OH, OW, 4), (4 * OW, 4, 1), 4
    if layout == "nchw":
        return (C, OH, OW), (OW, 1, OH * OW), C
    raise ValueError(layout)


def _resize(fn, what: str, src: tuple, H, W, C, OH, OW, mid: tuple, layout, out, dev):
    """One call of a resize entry point: its source arguments, the two axes' tap tables, OH, OW, ``mid``, the output
    of ``layout`` with its strides and channel count, the stream."""
    tables = [ptr(t) for n_in, n_out in ((H, OH), (W, OW)) for t in resize_tables(n_in, n_out, dev)]
    shape, strides, c_out = _layout(layout, C, OH, OW)
    out = _out_tensor(out, shape, dev, what)
    check(fn(*src, *tables, OH, OW, *mid, ptr(out), *strides, c_out, stream_ptr()), what)
    return out


def resize_bilinear_aa(img: torch.Tensor, OH: int, OW: int, layout: str = "nhwc4", mul: float = 1.0, out=None):
    """u8 [H,W,C<=4] CUDA image -> antialiased-bilinear resized f32 image: ``layout="nhwc4"`` -> [OH,OW,4] (extra channels
    zero), ``"nchw"`` -> [C,OH,OW]  (dataset/transform.py:14-17 on the GPU)."""
    if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3:
        raise TsodError("resize_bilinear_aa: a u8 [H,W,C] CUDA/ROCm tensor is required")
    H, W, C = img.shape
    if not 1 <= C <= 4 or img.stride(2) != 1 or img.stride(1) != C:
        raise TsodError("resize_bilinear_aa: pixels must be interleaved and contiguous along a row")
    return _resize(lib().tsod_resize_bilinear_aa_u8_f32, "resize_bilinear_aa", (ptr(img), H, W, C, img.stride(0)), H, W, C,
                   OH, OW, (float(mul),), layout, out, img.device)


# ----------------------------------------------------------------------------- training augmentation
def photometric(brightness=None, contrast=None, saturation=None, hue=None, contrast_before: bool = True, perm=None,
                white: float = 1.0) -> _ffi.Photometric:
    """The ``tsod_photometric`` of one image's RandomPhotometricDistort draws (None = the op was not drawn)."""
    p = _ffi.Photometric()
    flags = 0
    for bit, name, v in ((_ffi.AUG_BRIGHTNESS, "brightness", brightness), (_ffi.AUG_CONTRAST, "contrast", contrast),
                         (_ffi.AUG_SATURATION, "saturation", saturation), (_ffi.AUG_HUE, "hue", hue)):
        if v is not None:
            flags |= bit
            setattr(p, name, float(v))
    if contrast_before:
        flags |= _ffi.AUG_CONTRAST_FIRST
    if perm is not None:
        flags |= _ffi.AUG_PERMUTE
        p.perm[:] = [int(c) for c in perm]
    p.flags = flags
    p.white = float(white)
    return p


def _rgb_u8(img, what):
    if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise TsodError(f"{what}: a u8 [H,W,3] CUDA/ROCm tensor is required")
    if img.stride(2) != 1 or img.stride(1) != 3:
        raise TsodError(f"{what}: pixels must be interleaved and contiguous along a row")
    return img.shape[0], img.shape[1]


def augment_gray_mean_partials(img: torch.Tensor, params: _ffi.Photometric, out=None) -> torch.Tensor:
    """u8 [H,W,3] CUDA image -> f64 [TSOD_AUGMENT_MEAN_PARTS] partial sums of contrast's grayscale input (their sum /
    (H*W) is the mean; ``params`` must draw contrast)."""
    H, W = _rgb_u8(img, "augment_gray_mean_partials")
    if out is None:
        out = torch.empty(_ffi.AUG_MEAN_PARTS, dtype=torch.float64, device=img.device)
    if tuple(out.shape) != (_ffi.AUG_MEAN_PARTS,) or out.dtype != torch.float64 or out.device != img.device:
        raise TsodError(f"augment_gray_mean_partials: out must be f64 [{_ffi.AUG_MEAN_PARTS}] on {img.device}")
    check(lib().tsod_augment_gray_mean_partials(ptr(img), H, W, img.stride(0), byref(params), ptr(out), stream_ptr()),
          "augment_gray_mean_partials")
    return out


def augment_resize(img: torch.Tensor, OH: int, OW: int, params: _ffi.Photometric, flip: bool, mean_partials=None,
                   layout: str = "nchw", out=None) -> torch.Tensor:
    """u8 [H,W,3] CUDA image -> colour ops, channel permutation, optional horizontal flip and one antialiased bilinear
    resize to f32 (``layout="nchw"`` -> [3,OH,OW], ``"nhwc4"`` -> [OH,OW,4]).  ``mean_partials``: the output of
    ``augment_gray_mean_partials`` for the same image and params, required when contrast is drawn."""
    H, W = _rgb_u8(img, "augment_resize")
    dev = img.device
    if (params.flags & _ffi.AUG_CONTRAST) and mean_partials is None:
        raise TsodError("augment_resize: contrast is drawn but mean_partials is missing")
    return _resize(lib().tsod_augment_resize_u8_f32, "augment_resize",
                   (ptr(img), H, W, img.stride(0), byref(params), ptr(mean_partials), int(bool(flip))), H, W, 3, OH, OW, (),
                   layout, out, dev)


def resize_bilinear_aa_f32(src: torch.Tensor, OH: int, OW: int, layout: str = "nchw", out=None) -> torch.Tensor:
    """f32 [C<=4,H,W] CUDA image -> antialiased-bilinear resized f32 image (``layout`` as ``resize_bilinear_aa``); the
    same tap tables and tap order as the u8 kernel."""
    require_cuda(src, "resize_bilinear_aa_f32")
    if src.dim() != 3 or not 1 <= src.shape[0] <= 4:
        raise TsodError("resize_bilinear_aa_f32: an f32 [C<=4,H,W] tensor is required")
    C, H, W = src.shape
    return _resize(lib().tsod_resize_bilinear_aa_f32, "resize_bilinear_aa_f32",
                   (ptr(src), H, W, C, src.stride(1), src.stride(2), src.stride(0)), H, W, C, OH, OW, (), layout, out,
                   src.device)


def augment_boxes(boxes: torch.Tensor, labels: torch.Tensor, iparams: torch.Tensor, fparams: torch.Tensor):
    """Flip, two scalings and SanitizeBoundingBoxes for B images in one launch.  ``boxes`` f32 [N,4] / ``labels`` i64 [N]
    on the device; ``iparams`` i32 [B,4] = (first, count, flip, 0), ``fparams`` f32 [B,8] = (W, sx1, sy1, sx2, sy2, OW,
    OH, min_size).  -> (boxes_out [N,4], labels_out [N], kept i32 [B]): image b's kept boxes at [first, first + kept[b])."""
    require_cuda(boxes, "augment_boxes")
    dev = boxes.device
    if boxes.dim() != 2 or boxes.shape[1] != 4 or not boxes.is_contiguous():
        raise TsodError("augment_boxes: boxes must be a contiguous f32 [N,4] tensor")
    if labels.dtype != torch.int64 or labels.shape != (boxes.shape[0],) or labels.device != dev or not labels.is_contiguous():
        raise TsodError("augment_boxes: labels must be a contiguous i64 [N] tensor on the boxes' device")
    B = iparams.shape[0]
    if (iparams.dtype != torch.int32 or tuple(iparams.shape) != (B, 4) or fparams.dtype != torch.float32
            or tuple(fparams.shape) != (B, 8) or iparams.device != dev or fparams.device != dev
            or not iparams.is_contiguous() or not fparams.is_contiguous()):
        raise TsodError("augment_boxes: iparams must be i32 [B,4] and fparams f32 [B,8], contiguous, on the boxes' device")
    boxes_out = torch.empty_like(boxes)
    labels_out = torch.empty_like(labels)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib().tsod_augment_boxes_f32(ptr(boxes), ptr(labels), B, ptr(iparams), ptr(fparams), ptr(boxes_out),
                                       ptr(labels_out), ptr(kept), stream_ptr()), "augment_boxes")
    return boxes_out, labels_out, kept


def augment_color_host(rgb, params: _ffi.Photometric, mean: float = 0.0):
    """HOST: the colour ops and permutation of ``params`` on f32 [..., 3] pixels (a numpy array), given contrast's mean
    -- the per-pixel arithmetic the kernels run, for checking it without a GPU."""
    import numpy as np
    src = np.ascontiguousarray(rgb, dtype=np.float32)
    if src.shape[-1] != 3:
        raise ValueError("augment_color_host: pixels must be [..., 3]")
    out = np.empty_like(src)
    check(lib().tsod_augment_color_host(src.ctypes.data, src.size // 3, byref(params), float(mean), out.ctypes.data),
          "augment_color_host")
    return out


# ----------------------------------------------------------------------------- optimizer
def adamw_group(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: float) -> _ffi.AdamWGroup:
    """The scalars of step number ``step`` (1, 2, ...) for tensors that share these hyper-parameters: computed in double
    precision as torch's single-tensor AdamW computes them, each rounded once to f32 (by ctypes)."""
    bias1 = 1 - beta1 ** step
    bias2 = 1 - beta2 ** step
    return _ffi.AdamWGroup(1 - lr * weight_decay, 1 - beta1, beta2, 1 - beta2, lr / bias1, bias2 ** 0.5, eps, 0.0)


def adamw_chunks(numels, chunk: int = _ffi.ADAMW_CHUNK):
    """HOST: the work list of ``tsod_adamw_step_f32`` for tensors of ``numels`` elements: int32 [n_chunks, 2] rows
    (tensor, piece), tensor by tensor, piece = 0, 1, ... covering elements [piece * chunk, (piece + 1) * chunk) up to the
    tensor's end.  An empty tensor gets no row."""
    import numpy as np
    numels = np.asarray(numels, dtype=np.int64).reshape(-1)
    if (numels < 0).any() or chunk <= 0:
        raise ValueError("adamw_chunks: negative element count or chunk size")
    pieces = (numels + chunk - 1) // chunk
    total = int(pieces.sum())
    if total >= 2 ** 31 or len(numels) >= 2 ** 31:
        raise TsodError(f"adamw_chunks: {total} chunks do not fit one launch")
    out = np.empty((total, 2), dtype=np.int32)
    out[:, 0] = np.repeat(np.arange(len(numels)), pieces)
    out[:, 1] = np.arange(total) - np.repeat(np.cumsum(pieces) - pieces, pieces)
    return out


def adamw_table(pointers, numels, groups, n_groups: int):
    """HOST: ``tsod_adamw_tensor`` records as int64 [n, 6] words (param, grad, exp_avg, exp_avg_sq, n, group) from
    ``pointers`` [n, 4], checked here because the kernel only sees them in device memory: no null or misaligned pointer, no
    negative count, every group index inside [0, n_groups)."""
    import numpy as np
    pointers = np.asarray(pointers, dtype=np.int64).reshape(-1, 4)
    numels = np.asarray(numels, dtype=np.int64).reshape(-1)
    groups = np.asarray(groups, dtype=np.int64).reshape(-1)
    if not (len(pointers) == len(numels) == len(groups)):
        raise ValueError("adamw_table: pointers, numels and groups differ in length")
    if (numels < 0).any():
        raise TsodError("adamw_table: negative element count")
    if ((pointers == 0).any(axis=1) & (numels > 0)).any() or (pointers & 3).any():      # (an empty tensor has no storage)
        raise TsodError("adamw_table: null or misaligned tensor pointer")
    if len(groups) and (groups.min() < 0 or groups.max() >= n_groups):
        raise TsodError(f"adamw_table: group index outside [0, {n_groups})")
    table = np.empty((len(pointers), 6), dtype=np.int64)
    table[:, :4], table[:, 4], table[:, 5] = pointers, numels, groups      # (group in the low int32, reserved = 0)
    return table


def _check_work_list(table, chunks, what: str) -> None:
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.int64 and table.dim() == 2
            and table.shape[1] == 6 and table.is_contiguous()):
        raise TsodError(f"{what}: table must be a contiguous int64 [n, 6] CUDA/ROCm tensor (there is no CPU fallback)")
    if not (isinstance(chunks, torch.Tensor) and chunks.device == table.device and chunks.dtype == torch.int32
            and chunks.dim() == 2 and chunks.shape[1] == 2 and chunks.is_contiguous()):
        raise TsodError(f"{what}: chunks must be a contiguous int32 [n_chunks, 2] tensor on the table's device")


def adamw_step(table: torch.Tensor, chunks: torch.Tensor, groups, zero_grad: bool = False) -> None:
    """One AdamW update of every tensor of ``table`` (device copy of ``adamw_table``) over the work list ``chunks`` (device
    copy of ``adamw_chunks``) in ONE launch on the current stream.  ``groups``: a sequence of ``adamw_group`` records; they
    travel by value.  With ``zero_grad`` the gradients are cleared in the same pass."""
    _check_work_list(table, chunks, "adamw_step")
    arr = (_ffi.AdamWGroup * len(groups))(*groups)
    check(lib().tsod_adamw_step_f32(ptr(table), table.shape[0], ptr(chunks), chunks.shape[0], arr, len(groups),
                                    int(bool(zero_grad)), stream_ptr()), "adamw_step")


def adamw_step_host(param, grad, exp_avg, exp_avg_sq, group: _ffi.AdamWGroup, zero_grad: bool = False) -> None:
    """HOST: the kernel's per-element update, in place on four contiguous f32 numpy arrays of one size -- for checking the
    arithmetic without a GPU."""
    import numpy as np
    arrays = (param, grad, exp_avg, exp_avg_sq)
    for a in arrays:
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable
                and a.size == param.size):
            raise ValueError("adamw_step_host: four writeable contiguous float32 arrays of one size")
    check(lib().tsod_adamw_step_host_f32(*(a.ctypes.data for a in arrays), param.size, byref(group), int(bool(zero_grad))),
          "adamw_step_host")


# ----------------------------------------------------------------------------- gradient clipping
def _check_record(record, table, what: str) -> None:
    if not (isinstance(record, torch.Tensor) and record.device == table.device and record.dtype == torch.float64
            and record.shape == (2,) and record.is_contiguous()):
        raise TsodError(f"{what}: the result record must be a float64 [2] tensor on the table's device (grad_norm_record)")


def grad_norm_workspace_bytes(n_chunks: int) -> int:
    """Bytes of workspace ``grad_norm`` needs for a work list of ``n_chunks`` rows: one f64 partial per chunk."""
    return int(lib().tsod_grad_norm_workspace_bytes(int(n_chunks)))


def grad_norm_record(device) -> torch.Tensor:
    """A device buffer for one ``tsod_grad_norm_result`` (16 bytes), as float64 [2]: word 0 is ``sum_sq``, word 1 holds
    ``norm`` and ``coef`` (``grad_norm_fields`` views them)."""
    return torch.empty(2, dtype=torch.float64, device=device)


def grad_norm_fields(record: torch.Tensor):
    """(sum_sq, norm, coef) of a record as 0-d views into it: float64, float32, float32.  No copy, no synchronisation."""
    f = record.view(torch.float32)
    return record[0], f[2], f[3]


def grad_norm(table: torch.Tensor, chunks: torch.Tensor, max_norm: float, record: torch.Tensor,
              workspace: torch.Tensor) -> None:
    """The 2-norm over every gradient of ``table`` and the clip coefficient min(1, max_norm / (norm + 1e-6)) into ``record``
    (``grad_norm_record``), in two launches on the current stream: one f64 partial per row of ``chunks`` into
    ``workspace`` (a contiguous device tensor of at least ``grad_norm_workspace_bytes`` bytes), then one workgroup.  Every
    sum order depends on the element counts only (include/tsod.h); nothing is copied to the host."""
    _check_work_list(table, chunks, "grad_norm")
    _check_record(record, table, "grad_norm")
    if not (isinstance(workspace, torch.Tensor) and workspace.device == table.device and workspace.is_contiguous()):
        raise TsodError("grad_norm: workspace must be a contiguous tensor on the table's device")
    check(lib().tsod_grad_norm_f32(ptr(table), table.shape[0], ptr(chunks), chunks.shape[0], float(max_norm), ptr(record),
                                   ptr(workspace), workspace.numel() * workspace.element_size(), stream_ptr()), "grad_norm")


def adamw_step_clipped(table: torch.Tensor, chunks: torch.Tensor, groups, zero_grad: bool, record: torch.Tensor) -> None:
    """``adamw_step`` with every gradient multiplied by the coefficient of ``record`` (written by ``grad_norm`` earlier on
    the stream; the kernel reads it from device memory) in the same launch.  The gradients are cleared with ``zero_grad``
    and hold the clipped values otherwise."""
    _check_work_list(table, chunks, "adamw_step_clipped")
    _check_record(record, table, "adamw_step_clipped")
    arr = (_ffi.AdamWGroup * len(groups))(*groups)
    check(lib().tsod_adamw_step_clipped_f32(ptr(table), table.shape[0], ptr(chunks), chunks.shape[0], arr, len(groups),
                                            int(bool(zero_grad)), ptr(record), stream_ptr()), "adamw_step_clipped")


def grad_scale(table: torch.Tensor, chunks: torch.Tensor, record: torch.Tensor) -> None:
    """Every gradient of ``table`` times the coefficient of ``record``, in one launch over ``chunks``."""
    _check_work_list(table, chunks, "grad_scale")
    _check_record(record, table, "grad_scale")
    check(lib().tsod_grad_scale_f32(ptr(table), table.shape[0], ptr(chunks), chunks.shape[0], ptr(record), stream_ptr()),
          "grad_scale")


def grad_norm_host(grads, max_norm: float):
    """HOST: ``grad_norm`` over contiguous f32 numpy arrays, in the kernels' arithmetic and order -> (sum_sq, norm, coef) as
    numpy float64 / float32 / float32 scalars -- for checking the bits without a GPU."""
    import numpy as np
    grads = list(grads)
    for a in grads:
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous):
            raise ValueError("grad_norm_host: contiguous float32 arrays")
    pointers = (ctypes.c_void_p * max(len(grads), 1))(*(a.ctypes.data for a in grads))
    numels = (ctypes.c_int64 * max(len(grads), 1))(*(a.size for a in grads))
    out = _ffi.GradNormResult()
    check(lib().tsod_grad_norm_host_f32(pointers, numels, len(grads), float(max_norm), byref(out)), "grad_norm_host")
    return np.float64(out.sum_sq), np.float32(out.norm), np.float32(out.coef)


# ----------------------------------------------------------------------------- detection overlay
DRAW_TAGS = {None: _ffi.DRAW_TAG_NONE, "none": _ffi.DRAW_TAG_NONE, "above": _ffi.DRAW_TAG_ABOVE, "below": _ffi.DRAW_TAG_BELOW}


def draw_font5x7():
    """HOST: the overlay's font as a numpy u8 [128,7] array (``tsod_draw_font5x7``): row r of byte c's glyph in the 5 low
    bits, bit 4 the leftmost column."""
    import numpy as np
    out = np.zeros((128, 7), dtype=np.uint8)
    check(lib().tsod_draw_font5x7(out.ctypes.data), "draw_font5x7")
    return out


def draw_groups(images: torch.Tensor, groups, strings=None) -> torch.Tensor:
    """Paint up to ``_ffi.DRAW_MAX_GROUPS`` groups of boxes with their tags onto ``images`` (u8 [B,H,W,3] on the device, rows
    and images may be pitched) IN PLACE, in one launch (``tsod_draw_groups_u8``; the pixel rules are in include/tsod.h).

    ``groups``: dicts with ``boxes`` (f32 [B,R,4] or [B,R,6], contiguous) and optionally ``counts`` (i32 [B]), ``keep`` (i32
    [B,R]) with ``n_kept`` (i32 [B]), ``labels`` (i64 [B,R]), ``label_offset``, ``strings`` = (first, count) rows of the
    table (default: all of it), ``scale`` = (sx, sy), ``color`` (R, G, B),
    ``alpha``, ``width``, ``tag`` ("none" | "above" | "below"), ``text_color``, ``tag_bg``, ``tag_alpha``, ``font_scale``,
    ``padding``, ``score_line``.  ``strings``: u8 [n,32] zero-terminated rows on the device, or None.  Returns ``images``."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        require_cuda(images, "draw_groups")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError(f"draw_groups: images are u8 [B,H,W,3], got {images.dtype} {tuple(images.shape)}")
    B, H, W, _ = images.shape
    # (torch reports any stride for a dimension of size 1)
    row_bytes = images.stride(1) if H > 1 else 3 * W
    image_bytes = images.stride(0) if B > 1 else H * row_bytes
    if images.stride(3) != 1 or (W > 1 and images.stride(2) != 3) or row_bytes < 3 * W or image_bytes < H * row_bytes:
        raise ValueError("draw_groups: pixels must be interleaved, rows and images may only be padded at their ends")
    dev = images.device
    if len(groups) > _ffi.DRAW_MAX_GROUPS:
        raise ValueError(f"draw_groups: at most {_ffi.DRAW_MAX_GROUPS} groups in one launch, got {len(groups)}")
    n_strings = 0
    if strings is not None:
        if (not isinstance(strings, torch.Tensor) or strings.device != dev or strings.dtype != torch.uint8 or strings.dim() != 2
                or strings.shape[1] != _ffi.DRAW_STRING_BYTES or not strings.is_contiguous()):
            raise ValueError(f"draw_groups: strings are a contiguous u8 [n,{_ffi.DRAW_STRING_BYTES}] tensor on {dev}")
        n_strings = strings.shape[0]

    def opt(g, name, dtype, shape):
        t = g.get(name)
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"draw_groups: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}")
        return t

    arr = (_ffi.DrawGroup * max(len(groups), 1))()
    for rec, g in zip(arr, groups):
        boxes = g["boxes"]
        require_cuda(boxes, "draw_groups")
        if boxes.device != dev or boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] not in (4, 6) or not boxes.is_contiguous():
            raise ValueError(f"draw_groups: boxes are contiguous f32 [{B},R,4|6] on {dev}, got {tuple(boxes.shape)}")
        R = boxes.shape[1]
        rec.boxes, rec.R, rec.pitch = ptr(boxes), R, boxes.shape[2]
        rec.counts, rec.keep = ptr(opt(g, "counts", torch.int32, (B,))), ptr(opt(g, "keep", torch.int32, (B, R)))
        rec.n_kept, rec.labels = ptr(opt(g, "n_kept", torch.int32, (B,))), ptr(opt(g, "labels", torch.int64, (B, R)))
        rec.label_offset = int(g.get("label_offset", 0))
        rec.string_first, rec.string_count = (int(v) for v in g.get("strings", (0, n_strings)))
        rec.sx, rec.sy = (float(v) for v in g.get("scale", (1.0, 1.0)))
        tag = g.get("tag", "none")
        if tag not in DRAW_TAGS:
            raise ValueError(f"draw_groups: tag is 'none', 'above' or 'below', got {tag!r}")
        rec.tag = DRAW_TAGS[tag]
        for field, rgb, a in (("color", g.get("color", (255, 0, 0)), g.get("alpha", 255)),
                              ("text_rgb", g.get("text_color", g.get("color", (255, 0, 0))), 0),
                              ("tag_bg", g.get("tag_bg", (255, 255, 255)), g.get("tag_alpha", 255))):
            vals = tuple(int(v) for v in rgb) + (int(a),)
            if len(vals) != 4 or not all(0 <= v <= 255 for v in vals):
                raise ValueError(f"draw_groups: {field} is (R, G, B) with an alpha, each 0..255, got {vals}")
            setattr(rec, field, (ctypes.c_uint8 * 4)(*vals))
        rec.thickness, rec.font_scale = int(g.get("width", 1)), int(g.get("font_scale", 1))
        rec.padding, rec.score_line = int(g.get("padding", 0)), int(bool(g.get("score_line", False)))
    check(lib().tsod_draw_groups_u8(ptr(images), B, H, W, row_bytes, image_bytes, arr, len(groups), ptr(strings),
                                    n_strings, stream_ptr()), "draw_groups")
    return images


# ----------------------------------------------------------------------------- training curves
PLOT_MARKERS = {None: _ffi.PLOT_MARKER_NONE, "none": _ffi.PLOT_MARKER_NONE, "o": _ffi.PLOT_MARKER_CIRCLE,
                "circle": _ffi.PLOT_MARKER_CIRCLE, "s": _ffi.PLOT_MARKER_SQUARE, "square": _ffi.PLOT_MARKER_SQUARE,
                "^": _ffi.PLOT_MARKER_TRIANGLE, "triangle": _ffi.PLOT_MARKER_TRIANGLE}
PLOT_ITEM_KINDS = {"rect": _ffi.PLOT_ITEM_RECT, "text": _ffi.PLOT_ITEM_TEXT, "number": _ffi.PLOT_ITEM_NUMBER}
PLOT_ALIGN = {"left": 0, "right": 1, "center": 2}


def _rgba(what, rgb, alpha):
    vals = tuple(int(v) for v in rgb) + (int(alpha),)
    if len(vals) != 4 or not all(0 <= v <= 255 for v in vals):
        raise ValueError(f"{what}: a colour is (R, G, B) with an alpha, each 0..255, got {vals}")
    return (ctypes.c_uint8 * 4)(*vals)


def _plot_image(image, what):
    """-> (H, W, row_bytes) of one u8 [H,W,3] device image whose rows may be padded at their ends."""
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        require_cuda(image, what)
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise ValueError(f"{what}: the image is u8 [H,W,3], got {image.dtype} {tuple(image.shape)}")
    H, W, _ = image.shape
    row_bytes = image.stride(0) if H > 1 else 3 * W
    if image.stride(2) != 1 or (W > 1 and image.stride(1) != 3) or row_bytes < 3 * W:
        raise ValueError(f"{what}: pixels must be interleaved, rows may only be padded at their ends")
    return H, W, row_bytes


def ema_scan(x: torch.Tensor, alpha: float, out: torch.Tensor = None) -> torch.Tensor:
    """The reference's ``update_ema`` loop (train/train.py:147-153) over every row of ``x`` in one launch (``tsod_ema_scan_f32``):
    ``out[r, 0] = x[r, 0]``, ``out[r, i] = a x[r, i] + b out[r, i-1]`` with a = f32(alpha), b = f32(1 - alpha), two products and
    one sum in f32, no FMA.  ``x``: f32 [n] or [rows, n] on the device, rows may be pitched.  No host read."""
    require_cuda(x, "ema_scan")
    if x.dim() not in (1, 2) or (x.shape[-1] > 1 and x.stride(-1) != 1):
        raise ValueError(f"ema_scan: x is f32 [n] or [rows, n] with unit stride along n, got {tuple(x.shape)} strides {x.stride()}")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    else:
        require_cuda(out, "ema_scan")
        if out.shape != x.shape or out.device != x.device or (out.shape[-1] > 1 and out.stride(-1) != 1):
            raise ValueError("ema_scan: out must have x's shape and device and unit stride along n")
    n = x.shape[-1]
    rows = 1 if x.dim() == 1 else x.shape[0]
    pitch = lambda t: n if t.dim() == 1 or rows == 1 else t.stride(0)
    a, b = float(alpha), 1.0 - float(alpha)                      # (the subtraction in double; ctypes rounds both to f32)
    check(lib().tsod_ema_scan_f32(ptr(x), rows, n, pitch(x), a, b, ptr(out), pitch(out), stream_ptr()), "ema_scan")
    return out


def plot_limits(series, out: torch.Tensor = None, device=None) -> torch.Tensor:
    """The axis limits (lo, hi) of a panel over the finite samples of up to ``_ffi.PLOT_MAX_SERIES`` f32 [n] device tensors
    (``tsod_plot_limits_f32``; the rule is in include/tsod.h), written into ``out`` (f32 [2] on the device).  No host read."""
    series = [s for s in series if s is not None]
    if len(series) > _ffi.PLOT_MAX_SERIES:
        raise ValueError(f"plot_limits: at most {_ffi.PLOT_MAX_SERIES} series, got {len(series)}")
    for s in series:
        require_cuda(s, "plot_limits")
        if s.dim() != 1 or not s.is_contiguous():
            raise ValueError(f"plot_limits: a series is a contiguous f32 [n] tensor, got {tuple(s.shape)}")
    dev = out.device if out is not None else (series[0].device if series else torch.device(device))
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=dev)
    require_cuda(out, "plot_limits")
    if out.numel() != 2 or not out.is_contiguous():
        raise ValueError("plot_limits: out is a contiguous f32 [2] tensor")
    ws = torch.empty(_ffi.PLOT_LIMITS_WORKSPACE_BYTES // 4, dtype=torch.float32, device=dev)
    k = max(len(series), 1)
    pointers, lengths = (ctypes.c_void_p * k)(*[ptr(s) for s in series]), (ctypes.c_int64 * k)(*[s.numel() for s in series])
    check(lib().tsod_plot_limits_f32(pointers, lengths, len(series), ptr(out), ptr(ws), _ffi.PLOT_LIMITS_WORKSPACE_BYTES,
                                     stream_ptr()), "plot_limits")
    return out


def plot_series(image: torch.Tensor, rect, series, x_range, limits: torch.Tensor) -> torch.Tensor:
    """Paint up to ``_ffi.PLOT_MAX_SERIES`` curves, in order, into the rectangle ``rect`` = (px0, py0, pw, ph) of ``image`` (u8
    [H,W,3] on the device) IN PLACE, one launch (``tsod_plot_series_u8``; the pixel rules are in include/tsod.h).

    ``series``: dicts with ``y`` (contiguous f32 [n] on the device) and optionally ``x_first`` (0), ``x_step`` (1), ``color``,
    ``alpha`` (255), ``width`` (1), ``marker`` (None | "o" | "s" | "^"), ``marker_size`` (1, odd).  ``x_range`` = (x_lo, x_hi)
    are the abscissae of the rectangle's first and last column, ``limits`` the f32 [2] device record (lo, hi) of its bottom
    and top row.  Returns ``image``."""
    H, W, row_bytes = _plot_image(image, "plot_series")
    require_cuda(limits, "plot_series")
    if limits.numel() != 2 or not limits.is_contiguous() or limits.device != image.device:
        raise ValueError("plot_series: limits is a contiguous f32 [2] tensor on the image's device")
    if len(series) > _ffi.PLOT_MAX_SERIES:
        raise ValueError(f"plot_series: at most {_ffi.PLOT_MAX_SERIES} series in one launch, got {len(series)}")
    arr = (_ffi.PlotSeries * max(len(series), 1))()
    for rec, s in zip(arr, series):
        y = s["y"]
        require_cuda(y, "plot_series")
        if y.dim() != 1 or not y.is_contiguous() or y.device != image.device:
            raise ValueError(f"plot_series: y is a contiguous f32 [n] tensor on the image's device, got {tuple(y.shape)}")
        marker = s.get("marker")
        if marker not in PLOT_MARKERS:
            raise ValueError(f"plot_series: marker is None, 'o', 's' or '^', got {marker!r}")
        rec.y, rec.n, rec.x_first, rec.x_step = ptr(y), y.numel(), int(s.get("x_first", 0)), int(s.get("x_step", 1))
        rec.color = _rgba("plot_series", s.get("color", (0, 0, 0)), s.get("alpha", 255))
        rec.width, rec.marker, rec.marker_size = int(s.get("width", 1)), PLOT_MARKERS[marker], int(s.get("marker_size", 1))
    px0, py0, pw, ph = (int(v) for v in rect)
    check(lib().tsod_plot_series_u8(ptr(image), H, W, row_bytes, px0, py0, pw, ph, arr, len(series), int(x_range[0]),
                                    int(x_range[1]), ptr(limits), stream_ptr()), "plot_series")
    return image


def pack_plot_items(items) -> torch.Tensor:
    """HOST: a list of item dicts as the records of ``tsod_plot_items_u8``, a u8 [n, sizeof(tsod_plot_item)] CPU tensor.
    ``kind`` "rect": ``x, y, w, h`` and optionally ``dash`` = (period, on); "text": ``x, y, text`` (str or bytes, at most 32
    bytes); "number": ``x, y, limits`` (f32 [2] device tensor, which must outlive the launch), ``tick``, ``ticks``.  All:
    ``color`` (black), ``alpha`` (255); the text kinds: ``scale`` (1), ``align`` ("left" | "right" | "center")."""
    size = ctypes.sizeof(_ffi.PlotItem)
    arr = (_ffi.PlotItem * max(len(items), 1))()
    for rec, it in zip(arr, items):
        kind = it["kind"]
        if kind not in PLOT_ITEM_KINDS:
            raise ValueError(f"plot_items: kind is 'rect', 'text' or 'number', got {kind!r}")
        rec.kind, rec.x, rec.y = PLOT_ITEM_KINDS[kind], int(it["x"]), int(it["y"])
        rec.color = _rgba("plot_items", it.get("color", (0, 0, 0)), it.get("alpha", 255))
        rec.scale, rec.align = int(it.get("scale", 1)), PLOT_ALIGN[it.get("align", "left")]
        if kind == "rect":
            rec.w, rec.h = int(it["w"]), int(it["h"])
            rec.dash_period, rec.dash_on = (int(v) for v in it.get("dash", (0, 0)))
        elif kind == "text":
            raw = it["text"].encode("utf-8") if isinstance(it["text"], str) else bytes(it["text"])
            if len(raw) > _ffi.PLOT_STRING_BYTES:
                raise ValueError(f"plot_items: {raw!r} is {len(raw)} bytes; a text item holds at most {_ffi.PLOT_STRING_BYTES}")
            rec.len = len(raw)
            rec.text = (ctypes.c_uint8 * _ffi.PLOT_STRING_BYTES)(*raw)
        else:
            limits = it["limits"]
            require_cuda(limits, "plot_items")
            if limits.numel() != 2 or not limits.is_contiguous():
                raise ValueError("plot_items: limits is a contiguous f32 [2] device tensor")
            rec.limits, rec.tick, rec.ticks = ptr(limits), int(it["tick"]), int(it["ticks"])
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).reshape(max(len(items), 1), size)
    return raw[:len(items)]


def plot_items(image: torch.Tensor, items) -> torch.Tensor:
    """Paint decorations - filled or dashed rectangles, strings in the overlay's 5x7 font, numbers formatted on the device from
    a limits record - in order onto ``image`` (u8 [H,W,3] on the device) IN PLACE, one launch (``tsod_plot_items_u8``).
    ``items``: a list of dicts (``pack_plot_items``; uploaded here through pinned memory, no host wait), or the packed records
    already on the device.  Returns ``image``."""
    H, W, row_bytes = _plot_image(image, "plot_items")
    if not isinstance(items, torch.Tensor):
        packed = pack_plot_items(items)
        items = packed.pin_memory().to(image.device, non_blocking=True) if len(packed) else packed
    size = ctypes.sizeof(_ffi.PlotItem)
    n = items.shape[0]
    if n and (not items.is_cuda or items.device != image.device or items.dtype != torch.uint8 or items.dim() != 2
              or items.shape[1] != size or not items.is_contiguous()):
        raise ValueError(f"plot_items: packed items are a contiguous u8 [n,{size}] tensor on the image's device")
    check(lib().tsod_plot_items_u8(ptr(image), H, W, row_bytes, ptr(items) if n else None, n, stream_ptr()), "plot_items")
    return image


# ----------------------------------------------------------------------------- JPEG decoding
def jpeg_bytes(data):
    """HOST: ``bytes`` / ``bytearray`` / ``memoryview`` / a u8 ndarray as a contiguous u8 ndarray, without a copy when the
    memory is already contiguous."""
    import numpy as np
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8:
            raise ValueError(f"a JPEG file in an ndarray is uint8, got {data.dtype}")
        return np.ascontiguousarray(data).reshape(-1)
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    raise TypeError(f"a JPEG file is bytes, bytearray, memoryview or a uint8 ndarray, not {type(data).__name__}")


def jpeg_parse(data):
    """HOST: ``(status, JpegInfo)`` of one file's markers (``tsod_jpeg_parse``); status 0, or the negative ``tsod_status`` of a
    file this build does not decode (-2) or that is damaged (-1).  No exception: the caller names the file."""
    raw = jpeg_bytes(data)
    info = _ffi.JpegInfo()
    return int(lib().tsod_jpeg_parse(raw.ctypes.data, raw.size, byref(info))), info


def jpeg_entropy_decode(data, coef) -> int:
    """HOST: the Huffman pass of one file into ``coef``, a writeable contiguous int16 ndarray of at least
    ``JpegInfo.coef_total`` elements (``tsod_jpeg_entropy_decode``).  Returns the status.  ctypes releases the GIL for the
    call and the library keeps no state, so any number of threads may decode at once."""
    import numpy as np
    raw = jpeg_bytes(data)
    if not (isinstance(coef, np.ndarray) and coef.dtype == np.int16 and coef.flags.c_contiguous and coef.flags.writeable):
        raise ValueError("jpeg_entropy_decode: coef is a writeable contiguous int16 ndarray")
    return int(lib().tsod_jpeg_entropy_decode(raw.ctypes.data, raw.size, coef.ctypes.data, coef.size))


def jpeg_plan(infos):
    """HOST: the launch plan of a batch from its ``JpegInfo`` records: a dict with ``table`` (a ctypes array of
    ``tsod_jpeg_image``), ``idct_work`` and ``rgb_work`` (int32 [n, 4] ndarrays, the work lists of the two kernels) and the
    buffer sizes ``coef_count`` / ``quant_count`` (elements), ``plane_bytes`` / ``out_bytes``.  Image i's coefficients start at
    ``table[i].coef_offset[0]`` and its pixels at ``table[i].out_offset``, a multiple of 256."""
    import numpy as np
    table = (_ffi.JpegImage * max(len(infos), 1))()
    coef = quant = out = 0
    idct_work, rgb_work = [], []
    for i, info in enumerate(infos):
        rec = table[i]
        rec.H, rec.W, rec.n_comp, rec.hs, rec.vs = info.H, info.W, info.n_comp, info.hmax, info.vmax
        rec.quant_offset, rec.out_offset = quant, out
        quant += 64 * info.n_comp
        out += (3 * info.H * info.W + 255) // 256 * 256
        for c in range(info.n_comp):
            rec.blocks_w[c], rec.blocks_h[c] = info.blocks_w[c], info.blocks_h[c]
            rec.coef_offset[c] = rec.plane_offset[c] = coef          # one sample per coefficient: the planes share the layout
            n_blocks = info.blocks_w[c] * info.blocks_h[c]
            coef += 64 * n_blocks
            first = np.arange(0, n_blocks, _ffi.JPEG_IDCT_BLOCKS, dtype=np.int32)
            idct_work.append(np.stack([np.full_like(first, i), np.full_like(first, c), first, np.zeros_like(first)], axis=1))
        ty, tx = np.meshgrid(np.arange(-(-info.H // _ffi.JPEG_RGB_TILE_H), dtype=np.int32),
                             np.arange(-(-info.W // _ffi.JPEG_RGB_TILE_W), dtype=np.int32), indexing="ij")
        rgb_work.append(np.stack([np.full(ty.size, i, dtype=np.int32), ty.reshape(-1), tx.reshape(-1),
                                  np.zeros(ty.size, dtype=np.int32)], axis=1))
    empty = np.zeros((0, 4), dtype=np.int32)
    return dict(table=table, n_images=len(infos), coef_count=coef, quant_count=quant, plane_bytes=coef, out_bytes=out,
                idct_work=np.ascontiguousarray(np.concatenate(idct_work or [empty])),
                rgb_work=np.ascontiguousarray(np.concatenate(rgb_work or [empty])))


def _jpeg_lists(table, table_dev, work, work_dev, what: str):
    import numpy as np
    n_images = len(table)
    if not (isinstance(work, np.ndarray) and work.dtype == np.int32 and work.ndim == 2 and work.shape[1] == 4
            and work.flags.c_contiguous):
        raise ValueError(f"{what}: the host work list is a contiguous int32 [n, 4] ndarray")
    for t, nbytes, name in ((table_dev, n_images * ctypes.sizeof(_ffi.JpegImage), "table"), (work_dev, work.nbytes, "work list")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= nbytes):
            raise TsodError(f"{what}: the device {name} must be a contiguous CUDA/ROCm tensor of at least {nbytes} bytes "
                            "(there is no CPU fallback)")
    return n_images, work.shape[0]


def _jpeg_buffer(t, dtype, device, what: str):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == dtype and t.dim() == 1
            and t.is_contiguous()):
        raise TsodError(f"{what} must be a contiguous 1-d {dtype} tensor on the table's CUDA/ROCm device (there is no CPU fallback)")
    return t


def jpeg_idct(table, table_dev, work, work_dev, coef, quant, planes) -> torch.Tensor:
    """Dequantise and inverse-transform every block of a batch into its u8 component planes: ONE launch on the current stream
    (``tsod_jpeg_idct_u8``).  ``table`` / ``work``: the host arrays of ``jpeg_plan``; ``table_dev`` / ``work_dev``: their copies in
    device memory (any dtype, 16-byte aligned).  ``coef``: int16 device tensor; ``quant``: int16 device tensor holding the uint16
    quantiser entries; ``planes``: u8 device tensor.  The library checks every record and work item against the sizes of
    these buffers before it launches.  Returns ``planes``."""
    n_images, n_work = _jpeg_lists(table, table_dev, work, work_dev, "jpeg_idct")
    dev = table_dev.device
    _jpeg_buffer(coef, torch.int16, dev, "jpeg_idct: coef")
    _jpeg_buffer(quant, torch.int16, dev, "jpeg_idct: quant")
    _jpeg_buffer(planes, torch.uint8, dev, "jpeg_idct: planes")
    check(lib().tsod_jpeg_idct_u8(table, ptr(table_dev), n_images, work.ctypes.data, ptr(work_dev), n_work, ptr(coef), coef.numel(),
                                  ptr(quant), quant.numel(), ptr(planes), planes.numel(), stream_ptr()), "jpeg_idct")
    return planes


def jpeg_to_rgb(table, table_dev, work, work_dev, planes, out) -> torch.Tensor:
    """Upsample the chroma planes, convert to RGB and crop, every image of a batch into its packed u8 [H,W,3] at
    ``out[table[i].out_offset:]``: ONE launch on the current stream (``tsod_jpeg_to_rgb_u8``).  Arguments as ``jpeg_idct``;
    ``out``: u8 device tensor.  Returns ``out``."""
    n_images, n_work = _jpeg_lists(table, table_dev, work, work_dev, "jpeg_to_rgb")
    dev = table_dev.device
    _jpeg_buffer(planes, torch.uint8, dev, "jpeg_to_rgb: planes")
    _jpeg_buffer(out, torch.uint8, dev, "jpeg_to_rgb: out")
    check(lib().tsod_jpeg_to_rgb_u8(table, ptr(table_dev), n_images, work.ctypes.data, ptr(work_dev), n_work, ptr(planes),
                                    planes.numel(), ptr(out), out.numel(), stream_ptr()), "jpeg_to_rgb")
    return out


def jpeg_segment_dtype():
    """The NumPy record dtype of ``tsod_jpeg_segment`` (``_ffi.JpegSegment``)."""
    import numpy as np
    return np.dtype([("stream_offset", "<i8"), ("bit_length", "<i8"), ("image", "<i4"), ("first_mcu", "<i4"), ("n_mcu", "<i4"),
                     ("flags", "<i4")])


JPEG_HUFF_BYTES = ctypes.sizeof(_ffi.JpegHuff) * _ffi.JPEG_HUFF_TABLES       # the six code tables of one image


def jpeg_scan_sizes(info, n: int):
    """HOST: ``(stream_bytes, n_segments)``, the capacities ``jpeg_scan_prepare`` needs at most for a file of ``n`` bytes
    whose markers gave ``info`` (``tsod_jpeg_scan_sizes``)."""
    nbytes, n_seg = ctypes.c_int64(0), ctypes.c_int32(0)
    check(lib().tsod_jpeg_scan_sizes(byref(info), int(n), byref(nbytes), byref(n_seg)), "jpeg_scan_sizes")
    return int(nbytes.value), int(n_seg.value)


def jpeg_scan_prepare(data, stream, segments, tables):
    """HOST: the byte-speed sweep that ``entropy="device"`` leaves on the host (``tsod_jpeg_scan_prepare``): the file's
    entropy-coded bytes, unstuffed and without restart markers, into ``stream`` (a writeable contiguous u8 ndarray), one record
    per restart interval into ``segments`` (a writeable contiguous ndarray of ``jpeg_segment_dtype()``) and the scan's six code
    tables into ``tables`` (a writeable contiguous u8 ndarray of ``JPEG_HUFF_BYTES``).  Returns ``(status, stream_bytes,
    n_segments)``; no exception for a damaged file: the caller names it.  ctypes releases the GIL for the call."""
    import numpy as np
    raw = jpeg_bytes(data)
    for a, dtype, what in ((stream, np.uint8, "stream"), (segments, jpeg_segment_dtype(), "segments"), (tables, np.uint8, "tables")):
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.ndim == 1 and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError(f"jpeg_scan_prepare: {what} is a writeable contiguous 1-d {dtype} ndarray")
    if tables.size < JPEG_HUFF_BYTES:
        raise ValueError(f"jpeg_scan_prepare: tables holds {JPEG_HUFF_BYTES} bytes")
    nbytes, n_seg = ctypes.c_int64(0), ctypes.c_int32(0)
    rc = int(lib().tsod_jpeg_scan_prepare(raw.ctypes.data, raw.size, stream.ctypes.data, stream.size, byref(nbytes),
                                          segments.ctypes.data, segments.size, byref(n_seg), tables.ctypes.data))
    return rc, int(nbytes.value), int(n_seg.value)


def _jpeg_huffman_args(what: str, table, table_dev, segments, segments_dev, work, work_dev, stream, huff, coef, status):
    """The argument checks ``jpeg_huffman`` and ``jpeg_huffman_split`` share, ``work`` being the work list of the one and the
    chunk list of the other: ``(n_images, n_work, device)``."""
    import numpy as np
    n_images, n_work = _jpeg_lists(table, table_dev, work, work_dev, what)
    if not (isinstance(segments, np.ndarray) and segments.dtype == jpeg_segment_dtype() and segments.ndim == 1
            and segments.flags.c_contiguous):
        raise ValueError(f"{what}: the host segment records are a contiguous 1-d ndarray of jpeg_segment_dtype()")
    if not (isinstance(segments_dev, torch.Tensor) and segments_dev.is_cuda and segments_dev.is_contiguous()
            and segments_dev.numel() * segments_dev.element_size() >= segments.nbytes):
        raise TsodError(f"{what}: the device segment records must be a contiguous CUDA/ROCm tensor of at least "
                        f"{segments.nbytes} bytes (there is no CPU fallback)")
    dev = table_dev.device
    _jpeg_buffer(stream, torch.uint8, dev, f"{what}: stream")
    _jpeg_buffer(huff, torch.uint8, dev, f"{what}: huff")
    _jpeg_buffer(coef, torch.int16, dev, f"{what}: coef")
    _jpeg_buffer(status, torch.int32, dev, f"{what}: status")
    if status.numel() < n_images:
        raise ValueError(f"{what}: status holds one word per image")
    return n_images, n_work, dev


def jpeg_huffman(table, table_dev, segments, segments_dev, work, work_dev, stream, huff, coef, status, subseq_words: int):
    """The Huffman pass of a whole batch on the device: a fill launch that clears ``coef`` and ``status``, then ONE launch, one
    workgroup per restart interval, on the current stream (``tsod_jpeg_huffman_i16``).  ``table`` / ``segments`` / ``work``: the
    host arrays (``jpeg_plan``'s table, a ``jpeg_segment_dtype()`` ndarray sorted by image, an int32 [n, 4] list of segment
    numbers); ``*_dev``: their copies in device memory.  ``stream``: u8 device tensor of the unstuffed bytes; ``huff``: u8
    device tensor, ``JPEG_HUFF_BYTES`` per image; ``coef``: int16 device tensor; ``status``: int32 device tensor, one word per
    image, nonzero afterwards where the image's entropy-coded data are damaged.  ``subseq_words``: 32-bit words per
    subsequence, 1 .. 64.  The library checks every record and work item before it launches.  Returns ``coef``."""
    n_images, n_work, _ = _jpeg_huffman_args("jpeg_huffman", table, table_dev, segments, segments_dev, work, work_dev, stream, huff, coef,
                                             status)
    check(lib().tsod_jpeg_huffman_i16(table, ptr(table_dev), n_images, segments.ctypes.data, ptr(segments_dev), segments.size,
                                      work.ctypes.data, ptr(work_dev), n_work, ptr(stream), stream.numel(), ptr(huff),
                                      huff.numel() // ctypes.sizeof(_ffi.JpegHuff), ptr(coef), coef.numel(), ptr(status),
                                      int(subseq_words), stream_ptr()), "jpeg_huffman")
    return coef


JPEG_SPLIT_MAX = 256                                                         # chunk_subseqs + overlap: one workgroup


def jpeg_split_chunks(segments, subseq_words: int, chunk_subseqs: int):
    """HOST: the chunk list ``jpeg_huffman_split`` takes for ``segments`` (a ``jpeg_segment_dtype()`` ndarray) and the number of
    subsequences in all.  A segment of ``bits`` bits has ``n = ceil(bits / (32 subseq_words))`` subsequences and ``max(1, ceil(n /
    chunk_subseqs))`` chunks; an item is (segment, chunk, list index of the segment's chunk 0, the segment's chunk count).
    Returns ``(int32 [n_chunks, 4] ndarray, n_subseqs)``."""
    import numpy as np
    if not 1 <= int(subseq_words) <= 64 or not 1 <= int(chunk_subseqs) <= JPEG_SPLIT_MAX:
        raise ValueError("jpeg_split_chunks: subseq_words is in [1, 64] and chunk_subseqs in [1, 256]")
    bits = np.asarray(segments["bit_length"], dtype=np.int64)
    subseqs = -(-bits // (32 * int(subseq_words)))
    counts = np.maximum(-(-subseqs // int(chunk_subseqs)), 1)
    first = np.cumsum(counts) - counts
    total = int(counts.sum())
    chunks = np.empty((total, 4), dtype=np.int32)
    chunks[:, 0] = np.repeat(np.arange(bits.size), counts)
    chunks[:, 2] = np.repeat(first, counts)
    chunks[:, 3] = np.repeat(counts, counts)
    chunks[:, 1] = np.arange(total) - chunks[:, 2]
    return chunks, int(subseqs.sum())


def jpeg_huffman_split_workspace_bytes(n_subseqs: int, n_chunks: int, n_segments: int) -> int:
    """Bytes of workspace ``jpeg_huffman_split`` needs (``tsod_jpeg_huffman_split_workspace_bytes``)."""
    return int(lib().tsod_jpeg_huffman_split_workspace_bytes(int(n_subseqs), int(n_chunks), int(n_segments)))


def jpeg_huffman_split(table, table_dev, segments, segments_dev, chunks, chunks_dev, stream, huff, coef, status, subseq_words: int,
                       chunk_subseqs: int, overlap: int, workspace, repaired=None):
    """``jpeg_huffman`` with every segment split over several workgroups (``tsod_jpeg_huffman_split_i16``): a fill launch, then
    three launches on the current stream - sync (one workgroup per chunk of ``chunk_subseqs`` subsequences, warmed up over the
    ``overlap`` subsequences before it), stitch (one workgroup per segment joins the chunks, repairing a chunk whose assumed entry
    was wrong) and write.  Arguments as ``jpeg_huffman``, with the work list replaced by ``chunks`` / ``chunks_dev``
    (``jpeg_split_chunks``); ``workspace``: u8 device tensor of ``jpeg_huffman_split_workspace_bytes`` bytes, never read before
    it is written; ``repaired``: optional int32 device tensor, one word per segment, that receives the number of chunks the
    stitch launch repaired.  The coefficients and ``status`` are ``jpeg_huffman``'s, bit for bit.  Returns ``coef``."""
    n_images, n_chunks, dev = _jpeg_huffman_args("jpeg_huffman_split", table, table_dev, segments, segments_dev, chunks, chunks_dev, stream,
                                                 huff, coef, status)
    _jpeg_buffer(workspace, torch.uint8, dev, "jpeg_huffman_split: workspace")
    if repaired is not None:
        _jpeg_buffer(repaired, torch.int32, dev, "jpeg_huffman_split: repaired")
        if repaired.numel() < segments.size:
            raise ValueError("jpeg_huffman_split: repaired holds one word per segment")
    check(lib().tsod_jpeg_huffman_split_i16(table, ptr(table_dev), n_images, segments.ctypes.data, ptr(segments_dev), segments.size,
                                            chunks.ctypes.data, ptr(chunks_dev), n_chunks, ptr(stream), stream.numel(), ptr(huff),
                                            huff.numel() // ctypes.sizeof(_ffi.JpegHuff), ptr(coef), coef.numel(), ptr(status),
                                            int(subseq_words), int(chunk_subseqs), int(overlap), ptr(workspace), workspace.numel(),
                                            None if repaired is None else ptr(repaired), stream_ptr()), "jpeg_huffman_split")
    return coef
