"""Float64 restatements of the streaming layer kernels (csrc/pool_layout.hip) in plain torch on the CPU, each with the error
scale T its f32 kernel is held to, and the depthwise kernel's patch-selection rule restated.

Layouts are the kernels' own: activations NHWC [N,H,W,C], depthwise weights [3,3,C], pair weights [G,2], grouped weights
[C,3,3,cpg].  Every restatement is a sum of shifted slices - no call into torch's convolution - so that
tests/test_layer_kernels_gpu.py can check it against F.conv2d (on a CPU-only machine) and the kernels against it.

The bars are derived, not measured.  With u = 2^-24 (f32 round to nearest) and every operation of an output rounded at
most once, whether or not the compiler contracts a multiply into the add behind it:

  depthwise     9 products, 8 sums, one scale multiply, one shift add; ReLU is 1-Lipschitz      |got - y| <= 12 u T
  pair          2 products, one sum, the bias                                                   |got - y| <=  4 u T
  grouped 3x3   K = 9 cpg fma steps, then scale, shift and a 1-Lipschitz activation (PReLU's
                slope multiply is one more rounding)                                            |got - y| <= (K + 3) u T

where T is the same expression on absolute values: T = |scale| conv(|x|, |w|) + |shift|.
"""
import torch

U = 2.0 ** -24
DW_BAR = 12 * U
PAIR_BAR = 4 * U
ACT_NONE, ACT_PRELU, ACT_RELU6, ACT_RELU = 0, 1, 2, 3


def gconv3x3_bar(cpg: int) -> float:
    return (9 * cpg + 3) * U


def _f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def _out_extent(n: int, stride: int) -> int:
    return (n - 1) // stride + 1


def _taps(x, stride):
    """The nine shifted (and strided) views of x [N,H,W,C] under pad 1, as (dh, dw, view [N,OH,OW,C])."""
    N, H, W, C = x.shape
    OH, OW = _out_extent(H, stride), _out_extent(W, stride)
    xp = torch.zeros((N, H + 2, W + 2, C), dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    for dh in range(3):
        for dw in range(3):
            yield dh, dw, xp[:, dh:dh + (OH - 1) * stride + 1:stride, dw:dw + (OW - 1) * stride + 1:stride]


def _affine(acc, acc_abs, scale, shift):
    s, b = _f64(scale), _f64(shift)
    y = acc if s is None else acc * s
    T = acc_abs if s is None else acc_abs * s.abs()
    if b is not None:
        y, T = y + b, T + b.abs()
    return y, T


def dwconv_ref(x, w, scale, shift, stride, relu):
    """Depthwise 3x3, pad 1: x [N,H,W,C], w [3,3,C], scale / shift [C] or None -> (y, T), both f64 [N,OH,OW,C]."""
    x, w = _f64(x), _f64(w)
    acc = acc_abs = None
    for (dh, dw, v), (_, _, va) in zip(_taps(x, stride), _taps(x.abs(), stride)):
        p, pa = v * w[dh, dw], va * w[dh, dw].abs()
        acc, acc_abs = (p, pa) if acc is None else (acc.add_(p), acc_abs.add_(pa))
    y, T = _affine(acc, acc_abs, scale, shift)
    return (y.clamp_min(0.0) if relu else y), T


def gconv_pair_ref(x, w, bias):
    """nn.Conv2d(2G, G, 1, groups=G): x [..., 2G], w [G,2], bias [G] or None -> (y, T), both f64 [..., G]."""
    x, w = _f64(x), _f64(w)
    G = w.shape[0]
    xe, xo = x[..., 0:2 * G:2], x[..., 1:2 * G:2]
    y = xe * w[:, 0] + xo * w[:, 1]
    T = xe.abs() * w[:, 0].abs() + xo.abs() * w[:, 1].abs()
    return _affine(y, T, None, bias)


def activation(v, act, slope=0.0):
    if act == ACT_NONE:
        return v
    if act == ACT_PRELU:
        return v.clamp_min(0.0) + slope * v.clamp_max(0.0)
    if act == ACT_RELU6:
        return v.clamp(0.0, 6.0)
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    raise ValueError(act)


def gconv3x3_ref(x, w, groups, scale, shift, stride, act=ACT_NONE, slope=0.0):
    """Grouped 3x3, pad 1, C -> C: x [N,H,W,C], w [C,3,3,cpg], scale / shift [C] or None -> (y, T), both f64 [N,OH,OW,C].
    |slope| <= 1 (the bar counts the activation as 1-Lipschitz)."""
    assert abs(slope) <= 1.0
    x, w = _f64(x), _f64(w)
    N, H, W, C = x.shape
    cpg = C // groups
    assert cpg * groups == C and tuple(w.shape) == (C, 3, 3, cpg)
    wg = w.view(groups, cpg, 3, 3, cpg)                                  # [g, o, kh, kw, c]
    acc = acc_abs = None
    for (dh, dw, v), (_, _, va) in zip(_taps(x, stride), _taps(x.abs(), stride)):
        k = wg[:, :, dh, dw, :]                                          # [g, o, c]
        shape = v.shape[:3]
        p = torch.einsum("ngc,goc->ngo", v.reshape(-1, groups, cpg), k).reshape(*shape, C)
        pa = torch.einsum("ngc,goc->ngo", va.reshape(-1, groups, cpg), k.abs()).reshape(*shape, C)
        acc, acc_abs = (p, pa) if acc is None else (acc.add_(p), acc_abs.add_(pa))
    y, T = _affine(acc, acc_abs, scale, shift)
    return activation(y, act, slope), T


# ---- the depthwise kernel's patch selection (tsod_dwconv3x3_amax_f32), restated: (R, OUTS) ladders per stride, tallest first;
# the first patch that still yields DW_WANT threads is taken, the last one otherwise.  Variants are (STRIDE, OUTS, R).
DW_WANT = 256 * 256 * 2
DW_LADDER = {1: ((8, 4), (4, 4), (2, 4), (2, 2)), 2: ((4, 2), (2, 2), (1, 2))}
DW_VARIANTS = frozenset((s, outs, r) for s, ladder in DW_LADDER.items() for r, outs in ladder)


def dw_threads(N, H, W, C, stride, r, outs):
    OH, OW = _out_extent(H, stride), _out_extent(W, stride)
    return N * ((OH + r - 1) // r) * ((OW + outs - 1) // outs) * (C // 4)


def dw_variant(N, H, W, C, stride):
    ladder = DW_LADDER[stride]
    for r, outs in ladder[:-1]:
        if dw_threads(N, H, W, C, stride, r, outs) >= DW_WANT:
            return (stride, outs, r)
    r, outs = ladder[-1]
    return (stride, outs, r)
