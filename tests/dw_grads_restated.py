"""float64 torch-autograd statements of the depthwise 3x3 / pair 1x1 backward and of the HarDNet tail (DESIGN.md section
4.17), with the error bar the tests assert: for every output element, T = the sum of the absolute values of the products
that make it up (autograd of the same graph on absolute values) and n = their number; any f32 summation order satisfies
|err| <= (n + 8) 2^-24 T.  Shared by tests/test_dw_grads_gpu.py and tests/test_tail_grads.py; plain CPU torch."""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24


def assert_within(got, ref, T, n, what):
    """|got - ref| <= (n + 8) 2^-24 T elementwise; prints the worst ratio first."""
    got, ref, T = got.detach().double().cpu(), ref.double(), T.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = (n + 8) * EPS * T
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()):.3e}  max err/bound {worst:.3f}  (n = {n})")
    assert bool((err <= bound).all()), (what, worst)


def pack33(w):
    """torch [C,1,3,3] -> the kernels' [3][3][C]."""
    C = w.shape[0]
    return w.reshape(C, 9).t().reshape(3, 3, C).contiguous()


def unpack33(d):
    """[3][3][C] -> [C,1,3,3]."""
    C = d.shape[2]
    return d.reshape(9, C).t().reshape(C, 1, 3, 3)


def dw_reference(x, w, scale, shift, stride, relu, dy, margin=1e-4):
    """y = relu?(scale * conv(x, w) + shift) in float64 from f32 NCHW inputs (w [C,1,3,3]; scale / shift [C] or None).
    -> dict of (gradient, T, n) for dx, dw, dscale, dshift, plus ``clear``: no pre-ReLU value within ``margin`` of zero."""
    C = x.shape[1]
    one = torch.ones(C, dtype=torch.float64)
    xs = x.double().requires_grad_()
    ws = w.double().requires_grad_()
    sc = (one.clone() if scale is None else scale.double()).requires_grad_()
    sh = (0 * one if shift is None else shift.double()).requires_grad_()
    conv = F.conv2d(xs, ws, None, stride, 1, groups=C)
    y = conv * sc.view(1, C, 1, 1) + sh.view(1, C, 1, 1)
    mask = (y > 0).double() if relu else torch.ones_like(y)
    clear = (not relu) or bool((y.detach().abs() > margin).all())
    grads = torch.autograd.grad(y * mask, [xs, ws, sc, sh], dy.double())
    xa, wa, sa = (v.detach().abs().requires_grad_() for v in (xs, ws, sc))
    sha = sh.detach().abs().requires_grad_()
    conva = F.conv2d(xa, wa, None, stride, 1, groups=C)
    ya = conva * sa.view(1, C, 1, 1) + sha.view(1, C, 1, 1)
    Ts = torch.autograd.grad(ya * mask, [xa, wa, sa, sha], dy.double().abs())
    pixels = y.shape[0] * y.shape[2] * y.shape[3]
    ns = (9, pixels, pixels, pixels)
    out = {k: (g, T, n) for k, g, T, n in zip(("dx", "dw", "dscale", "dshift"), grads, Ts, ns)}
    out["clear"], out["y"] = clear, y.detach()
    return out


def pair_reference(x, w, dy):
    """out[g] = w[g][0] x[2g] + w[g][1] x[2g+1] + bias[g] on rows: x [pixels, 2G], w [G,2], dy [pixels, G] (f32) ->
    dict of (gradient, T, n) for dx, dw, dbias."""
    P, G = dy.shape
    xs = x.double().view(P, G, 2).requires_grad_()
    ws = w.double().requires_grad_()
    b = torch.zeros(G, dtype=torch.float64, requires_grad=True)
    grads = torch.autograd.grad((xs * ws).sum(-1) + b, [xs, ws, b], dy.double())
    xa, wa = xs.detach().abs().requires_grad_(), ws.detach().abs().requires_grad_()
    ba = torch.zeros(G, dtype=torch.float64, requires_grad=True)
    Ts = torch.autograd.grad((xa * wa).sum(-1) + ba, [xa, wa, ba], dy.double().abs())
    return {"dx": (grads[0].reshape(P, 2 * G), Ts[0].reshape(P, 2 * G), 1), "dw": (grads[1], Ts[1], P), "dbias": (grads[2], Ts[2], P)}


def _tail(x0, p, mask):
    w1, b1, w2, b2, wp, bp = p
    C = x0.shape[1]
    y1 = F.conv2d(x0, w1, b1, 2, 1, groups=C)
    a = y1 * mask if mask is not None else y1
    b = F.conv2d(a, w2, b2, 2, 1, groups=C)
    return F.conv2d(b, wp, bp, groups=wp.shape[0]), y1


def tail_reference(x0, params, gy, mask_f32=None):
    """The four tail modules (dw3x3 s2 + bias, ReLU, dw3x3 s2 + bias, Conv2d(2G, G, 1, groups=G) + bias) in float64 on the
    tail's input ``x0`` [N,C,H,W] (f32), ``params`` the six torch-layout tensors, ``gy`` [N,G,h,w] the upstream gradient.
    -> [(gradient, T, n)] for the six.

    The ReLU's mask is the float64 one wherever it is decided: |y| > 11 * 2^-24 * (sum_taps |x||w| + |b|), the round-off an f32
    evaluation of y (nine products, a bias) can have.  Inside that band the sign of the f64 value says nothing about the f32
    forward that ran; there ``mask_f32`` (the f32 forward's own y > 0) is the derivative's mask, and outside it ``mask_f32``
    is asserted equal to the f64 mask.  Without ``mask_f32`` the band must be empty.
    n = the pixels summed over + 9: the upstream of the deeper layers is itself a short sum of products (<= 4 taps and a
    weight per stage), each of which adds its roundings to every term."""
    p64 = [t.detach().double().cpu() for t in params]
    x64, g64 = x0.detach().double().cpu(), gy.detach().double().cpu()
    with torch.no_grad():
        _, y1 = _tail(x64, p64, None)
        Ty = F.conv2d(x64.abs(), p64[0].abs(), p64[1].abs(), 2, 1, groups=x64.shape[1])
    band = y1.abs() <= 11 * EPS * Ty
    m64 = y1 > 0
    print(f"tail_reference: {int(band.sum())} of {band.numel()} pre-ReLU values inside the f32 round-off band")
    if mask_f32 is None:
        assert not bool(band.any())
        mask = m64
    else:
        mask_f32 = mask_f32.cpu().bool()
        assert bool((mask_f32 == m64)[~band].all()), "ReLU masks differ outside the round-off band"
        mask = torch.where(band, mask_f32, m64)
    mask = mask.double()
    ps = [t.clone().requires_grad_() for t in p64]
    out, _ = _tail(x64, ps, mask)
    grads = torch.autograd.grad(out, ps, g64)
    pa = [t.abs().requires_grad_() for t in p64]
    outa, _ = _tail(x64.abs(), pa, mask)
    Ts = torch.autograd.grad(outa, pa, g64.abs())
    N, _, H, W = x64.shape
    h1, w1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h2, w2 = (h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1
    n1, n2 = N * h1 * w1 + 9, N * h2 * w2 + 9
    return list(zip(grads, Ts, (n1, n1, n2, n2, n2, n2)))
