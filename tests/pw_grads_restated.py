"""float64 torch-autograd statements of the 1x1 ConvLayer backward and of a HarDBlock section, with the
error bar of tests/dw_grads_restated.py: for every output element, T = the sum of the absolute values of the products that make
it up (autograd of the same graph on absolute values) and n = their number; |err| <= (n + 8) 2^-24 T.

Only the backward is under test: every layer's forward output is replaced, straight-through, by the output the HIP run saved
(y = y64 + (y_hip - y64).detach()), and the ReLU6 mask is taken from that saved output (strict 0 < y < 6: where the forward
clamped, torch's hardtanh backward gives nothing).  Shared by tests/test_pw_grads_abi.py, tests/test_pw_grads_gpu.py and
tests/test_block_grads.py; plain CPU torch."""
import torch
import torch.nn.functional as F

from dw_grads_restated import EPS, assert_within  # noqa: F401  (re-exported)

TAIL_N = 9 + 9 + 2          # products behind an element of the gradient the tail hands the last transition layer


def conv_layer_reference(xg, w, scale, shift, y_hip, dy):
    """One ConvLayer on rows: y = relu6(scale * (xg @ w.T) + shift), i.e. F.conv2d(1x1) + eval F.batch_norm + F.hardtanh(0, 6)
    with BN folded.  xg [M,K] the gathered real input, w [Cout,K], scale / shift [Cout], y_hip [M,Cout] the saved forward
    output, dy [M,Cout] (all f32) -> dict of (gradient, T, n) for dx [M,K], dw, dscale, dshift."""
    M, K = xg.shape
    yh = y_hip.double()
    mask = ((yh > 0) & (yh < 6)).double()

    def run(absval):
        f = (lambda t: t.detach().double().abs()) if absval else (lambda t: t.detach().double())
        leaves = [f(t).requires_grad_() for t in (xg, w, scale, shift)]
        x_, w_, sc_, sh_ = leaves
        y = ((x_ @ w_.t()) * sc_ + sh_) * mask
        y = y + (yh - y).detach()
        return torch.autograd.grad(y, leaves, f(dy))
    g, T = run(False), run(True)
    ns = (w.shape[0], M, M + K, M)
    return {k: (gi, Ti, n) for k, gi, Ti, n in zip(("dx", "dw", "dscale", "dshift"), g, T, ns)}


def block_forward_plain(blk, transition, x):
    """The reference's HarDBlock.forward + transition ConvLayer with the repo's modules called as torch modules (any dtype):
    -> (out, slices [block input, layer outputs...], 1x1 outputs per layer)."""
    layers_, ys = [x], []
    for li, comb in enumerate(blk.layers, start=1):
        tin = torch.cat([layers_[k] for k in blk.links[li - 1]], 1)
        y = comb.layer1(tin)
        ys.append(y)
        layers_.append(comb.layer2(y))
    out = transition(torch.cat([layers_[k] for k in blk.output_slices()], 1))
    return out, layers_, ys


def _upstream_counts(blk, up_transition, tr_cout):
    """n of the gradient arriving at every slice of a block (deepest path): (per slice, per layer's masked gradient)."""
    L = len(blk.layers)
    outs = blk.output_slices()
    up_slice, up_g = {}, {}
    for s in range(L, -1, -1):
        cons = [(up_g[j] + blk.layer_out[j - 1]) for j in range(s + 1, L + 1) if s in blk.links[j - 1]]
        if s in outs:
            cons.append(up_transition + tr_cout)
        up_slice[s] = max(cons) + len(cons)
        if s >= 1:
            up_g[s] = up_slice[s] + 9
    return up_slice, up_g


def section_reference(section, tail, x_in, gy, tail_mask=None):
    """The section in float64.  ``section``: per HarDBlock in forward order a dict ``index`` (of the block in ``base``), ``block``,
    ``tr_index``, ``transition`` (ConvLayer), ``down_index`` / ``down`` (the DWConvLayer in FRONT of the block, None for the
    first), ``slices`` (the HIP run's block buffer as NCHW real-channel tensors: slice 0 = input), ``ys`` (the saved 1x1 outputs)
    and ``tr_y`` (the saved transition output).  ``tail``: None (``gy`` is then the gradient of the last transition output) or
    (i1, conv1, i2, conv2, ip, pair) with ``tail_mask`` the f32 forward's ReLU mask.  ``x_in`` the section's input.
    -> {parameter name: (gradient, T, n)} with the names of ``named_parameters()`` under ``base``."""
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
            z = bn(F.conv2d(x, leaf(prefix + ".conv.weight", m.conv.weight)), prefix + ".norm", m.norm)
            yh = y_hip.detach().double()
            pixels[prefix] = z.shape[0] * z.shape[2] * z.shape[3]
            return st(z * ((yh > 0) & (yh < 6)).double(), y_hip)

        def dw_layer(x, prefix, m, hip):
            C = x.shape[1]
            z = F.conv2d(x, leaf(prefix + ".dwconv.weight", m.dwconv.weight), None, m.dwconv.stride, 1, groups=C)
            pixels[prefix] = z.shape[0] * z.shape[2] * z.shape[3]
            return st(bn(z, prefix + ".norm", m.norm), hip)

        x = f(x_in)
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
            y1 = F.conv2d(x, leaf(f"base.{i1}.weight", c1.weight), leaf(f"base.{i1}.bias", c1.bias), 2, 1, groups=C)
            bb = F.conv2d(y1 * tail_mask.double(), leaf(f"base.{i2}.weight", c2.weight), leaf(f"base.{i2}.bias", c2.bias), 2, 1, groups=C)
            x = F.conv2d(bb, leaf(f"base.{ip}.weight", pair.weight), leaf(f"base.{ip}.bias", pair.bias), groups=pair.out_channels)
        names = list(P)
        return names, torch.autograd.grad(x, [P[k] for k in names], f(gy))

    names, grads = run(False)
    _, Ts = run(True)
    # term counts along the deepest path, from the last block down
    n = {}
    up = TAIL_N if tail is not None else 0
    for b in reversed(section):
        blk = b["block"]
        up_slice, up_g = _upstream_counts(blk, up, b["transition"].conv.out_channels)
        tr = f"base.{b['tr_index']}"
        K_tr = b["transition"].conv.in_channels
        n[tr + ".conv.weight"] = n[tr + ".norm.bias"] = up + pixels[tr]
        n[tr + ".norm.weight"] = up + pixels[tr] + K_tr
        for li, comb in enumerate(blk.layers, start=1):
            p1, p2 = f"base.{b['index']}.layers.{li - 1}.layer1", f"base.{b['index']}.layers.{li - 1}.layer2"
            n[p2 + ".dwconv.weight"] = n[p2 + ".norm.bias"] = up_slice[li] + pixels[p2]
            n[p2 + ".norm.weight"] = up_slice[li] + pixels[p2] + 9
            n[p1 + ".conv.weight"] = n[p1 + ".norm.bias"] = up_g[li] + pixels[p1]
            n[p1 + ".norm.weight"] = up_g[li] + pixels[p1] + comb.layer1.conv.in_channels
        up = up_slice[0]
        if b.get("down") is not None:
            d = f"base.{b['down_index']}"
            n[d + ".dwconv.weight"] = n[d + ".norm.bias"] = up + pixels[d]
            n[d + ".norm.weight"] = up + pixels[d] + 9
            up += 9
    if tail is not None:
        big = max(pixels.values())
        for k in names:
            n.setdefault(k, big + 9)                      # (the six tail tensors: dw_grads_restated.tail_reference's count)
    return {k: (g, T, n[k]) for k, g, T in zip(names, grads, Ts)}
