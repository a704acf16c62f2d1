"""float64 torch-autograd statements of the HarDNet stem's backward, with the error bar of
tests/dw_grads_restated.py: for every output element, T = the sum of the absolute values of the products that make it up
(autograd of the same graph on absolute values) and n = their number; |err| <= (n + 8) 2^-24 T.

As in tests/pw_grads_restated.py only the backward is under test: every layer's forward output is replaced, straight-through,
by the output the HIP run saved, and the ReLU6 mask is taken from that saved output (strict 0 < y < 6).  Shared by
tests/test_stem_grads_abi.py, tests/test_stem_grads_gpu.py and tests/test_full_grads.py; plain CPU torch."""
import torch
import torch.nn.functional as F

from pw_grads_restated import TAIL_N, _upstream_counts, assert_within  # noqa: F401  (assert_within re-exported)

STEM_NAMES = [f"base.0.{k}" for k in ("conv.weight", "norm.weight", "norm.bias")] + \
             [f"base.1.{k}" for k in ("conv.weight", "norm.weight", "norm.bias")] + \
             [f"base.2.{k}" for k in ("dwconv.weight", "norm.weight", "norm.bias")]


def conv3x3_layer_reference(x, w, scale, shift, y_hip, dy, stride):
    """The first layer alone: y = relu6(scale * conv3x3(x, w, stride, pad 1) + shift).  x [N,3,H,W], w [Cout,3,3,3], scale / shift
    [Cout], y_hip [N,Cout,OH,OW] the saved forward output, dy [N,Cout,OH,OW] (all f32) -> dict of (gradient, T, n) for dw,
    dscale, dshift.  There is no dx."""
    yh = y_hip.double()
    mask = ((yh > 0) & (yh < 6)).double()
    M = yh.shape[0] * yh.shape[2] * yh.shape[3]

    def run(absval):
        f = (lambda t: t.detach().double().abs()) if absval else (lambda t: t.detach().double())
        leaves = [f(t).requires_grad_() for t in (w, scale, shift)]
        w_, sc_, sh_ = leaves
        y = (F.conv2d(f(x), w_, None, stride, 1) * sc_.view(1, -1, 1, 1) + sh_.view(1, -1, 1, 1)) * mask
        y = y + (yh - y).detach()
        return torch.autograd.grad(y, leaves, f(dy))
    g, T = run(False), run(True)
    return {k: (gi, Ti, n) for k, gi, Ti, n in zip(("dw", "dscale", "dshift"), g, T, (M, M + 27, M))}


def stem_forward_plain(m0, m1, m2, x):
    """ConvLayer(3, c0, 3, stride 2) -> ConvLayer(c0, c1, 1) -> DWConvLayer(c1, stride 2) called as torch modules."""
    y0 = m0(x)
    y1 = m1(y0)
    return y0, y1, m2(y1)


def backbone_reference(stem, section, tail, gy, tail_mask=None):
    """The nine stem tensors' gradients when the stem feeds ``section`` (and ``tail``) of tests/pw_grads_restated.py's
    ``section_reference`` (same arguments; ``section`` may be empty and ``tail`` None: ``gy`` is then the gradient of the stem's
    output).  ``stem``: dict ``m0`` / ``m1`` / ``m2`` (the three modules, float64), ``x`` (the image [N,3,H,W]), ``y0`` / ``y1``
    (the saved outputs of base.0 / base.1) and ``out`` (base.2's saved output: slice 0 of the first block).
    -> {parameter name: (gradient, T, n)} for ``STEM_NAMES``; n is summed along the deepest path."""
    pixels = {}

    def run(absval):
        P = {}
        f = (lambda t: t.detach().double().abs()) if absval else (lambda t: t.detach().double())

        def leaf(name, t):
            P[name] = f(t).clone().requires_grad_()
            return P[name]

        def st(v, hip):
            return v + (f(hip) - v).detach()

        def bn(z, prefix, norm):
            inv = 1.0 / torch.sqrt(norm.running_var.detach().double() + norm.eps)
            mu = norm.running_mean.detach().double()
            scale = leaf(prefix + ".weight", norm.weight) * inv
            b = leaf(prefix + ".bias", norm.bias)
            shift = b + mu.abs() * scale if absval else b - mu * scale
            return z * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)

        def conv_layer(x, prefix, m, y_hip):
            z = bn(F.conv2d(x, leaf(prefix + ".conv.weight", m.conv.weight), None, m.conv.stride, m.conv.padding),
                   prefix + ".norm", m.norm)
            yh = y_hip.detach().double()
            pixels[prefix] = z.shape[0] * z.shape[2] * z.shape[3]
            return st(z * ((yh > 0) & (yh < 6)).double(), y_hip)

        def dw_layer(x, prefix, m, hip):
            C = x.shape[1]
            z = F.conv2d(x, leaf(prefix + ".dwconv.weight", m.dwconv.weight), None, m.dwconv.stride, 1, groups=C)
            pixels[prefix] = z.shape[0] * z.shape[2] * z.shape[3]
            return st(bn(z, prefix + ".norm", m.norm), hip)

        x = conv_layer(f(stem["x"]), "base.0", stem["m0"], stem["y0"])
        x = conv_layer(x, "base.1", stem["m1"], stem["y1"])
        x = dw_layer(x, "base.2", stem["m2"], stem["out"])
        for b in section:
            if b.get("down") is not None:
                x = dw_layer(x, f"base.{b['down_index']}", b["down"], b["slices"][0])
            blk, layers_ = b["block"], [x]
            for li, comb in enumerate(blk.layers, start=1):
                tin = torch.cat([layers_[k] for k in blk.links[li - 1]], 1)
                prefix = f"base.{b['index']}.layers.{li - 1}"
                y = conv_layer(tin, prefix + ".layer1", comb.layer1, b["ys"][li - 1])
                layers_.append(dw_layer(y, prefix + ".layer2", comb.layer2, b["slices"][li]))
            x = conv_layer(torch.cat([layers_[k] for k in blk.output_slices()], 1), f"base.{b['tr_index']}", b["transition"], b["tr_y"])
        if tail is not None:
            i1, c1, i2, c2, ip, pair = tail
            C = x.shape[1]
            y1 = F.conv2d(x, f(c1.weight), f(c1.bias), 2, 1, groups=C)
            bb = F.conv2d(y1 * tail_mask.double(), f(c2.weight), f(c2.bias), 2, 1, groups=C)
            x = F.conv2d(bb, f(pair.weight), f(pair.bias), groups=pair.out_channels)
        return torch.autograd.grad(x, [P[k] for k in STEM_NAMES], f(gy))

    grads, Ts = run(False), run(True)
    # products behind an element of the gradient that arrives at the stem's output (the first block's slice 0)
    up = TAIL_N if tail is not None else 0
    for b in reversed(section):
        up_slice, _ = _upstream_counts(b["block"], up, b["transition"].conv.out_channels)
        up = up_slice[0] + (9 if b.get("down") is not None else 0)
    c0, c1 = stem["m1"].conv.in_channels, stem["m1"].conv.out_channels
    n = {"base.2.dwconv.weight": up + pixels["base.2"], "base.2.norm.bias": up + pixels["base.2"],
         "base.2.norm.weight": up + pixels["base.2"] + 9}
    up += 9                                                    # base.2's dx gather
    n.update({"base.1.conv.weight": up + pixels["base.1"], "base.1.norm.bias": up + pixels["base.1"],
              "base.1.norm.weight": up + pixels["base.1"] + c0})
    up += c1                                                   # base.1's dx
    n.update({"base.0.conv.weight": up + pixels["base.0"], "base.0.norm.bias": up + pixels["base.0"],
              "base.0.norm.weight": up + pixels["base.0"] + 27})
    return {k: (g, T, n[k]) for k, g, T in zip(STEM_NAMES, grads, Ts)}
