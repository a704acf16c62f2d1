"""The backward of one trainable HarDBlock with active dropout in float64: the graph of
tests/bn_train_restated.py's ``bn_section_reference`` for a single block - every conv output replaced, straight-through, by the
saved raw z and every layer output by the saved output, F.batch_norm(training=True) on the saved z, the ReLU6 mask from the saved
output, T from the same graph on absolute values - in which the concatenated input of the transition layer is multiplied by the
dropout mask (its scale where kept, 0 where dropped; it is its own absolute value).  The counts n are bn_section_reference's:
the multiply is exact in float64 and adds no term of its own."""
import torch
import torch.nn.functional as F

from bn_train_restated import _AbsBatchNorm
from pw_grads_restated import TAIL_N, _upstream_counts


def section_reference(b, tail, gy, tail_mask, mask):
    """``b``: one block as bn_section_reference takes it (``index``, ``block``, ``tr_index``, ``transition``, ``slices``, ``ys``,
    ``zs``, ``dw_zs``, ``tr_y``, ``tr_z``; no ``down``: slice 0 is the section's input).  ``tail``: None (``gy`` is then the
    gradient of the transition's output) or (i1, conv1, i2, conv2, ip, pair) with ``tail_mask``.  ``mask`` [N, C, h, w].
    -> {parameter name: (gradient, T, n)}."""
    pixels, order = {}, []
    blk, transition, slices = b["block"], b["transition"], b["slices"]

    def run(absval):
        P = {}
        f = (lambda t: t.detach().double().abs()) if absval else (lambda t: t.detach().double())

        def leaf(name, t):
            P[name] = f(t).clone().requires_grad_()
            return P[name]

        def st(v, hip):
            return v + (f(hip) - v).detach()

        def bn(z, prefix, norm, z_hip):
            z = st(z, z_hip)
            gamma, beta = leaf(prefix + ".weight", norm.weight), leaf(prefix + ".bias", norm.bias)
            if not absval:
                return F.batch_norm(z, None, None, gamma, beta, True, 0.0, norm.eps)
            zh = z_hip.detach().double()
            d = (0, 2, 3)
            inv = 1.0 / torch.sqrt(zh.var(d, unbiased=False, keepdim=True) + norm.eps)
            xhat = ((zh - zh.mean(d, keepdim=True)) * inv).abs()
            return _AbsBatchNorm.apply(z, gamma, beta, xhat, norm.weight.detach().double().abs() * inv.reshape(-1))

        def conv_layer(x, prefix, m, y_hip, z_hip):
            z = F.conv2d(x, leaf(prefix + ".conv.weight", m.conv.weight), None, m.conv.stride, m.conv.padding)
            yh = y_hip.detach().double()
            pixels[prefix] = z.shape[0] * z.shape[2] * z.shape[3]
            if not absval:
                order.append(prefix)
            return st(bn(z, prefix + ".norm", m.norm, z_hip) * ((yh > 0) & (yh < 6)).double(), y_hip)

        def dw_layer(x, prefix, m, hip, z_hip):
            z = F.conv2d(x, leaf(prefix + ".dwconv.weight", m.dwconv.weight), None, m.dwconv.stride, 1, groups=x.shape[1])
            pixels[prefix] = z.shape[0] * z.shape[2] * z.shape[3]
            if not absval:
                order.append(prefix)
            return st(bn(z, prefix + ".norm", m.norm, z_hip), hip)

        layers_ = [f(slices[0])]
        for li, comb in enumerate(blk.layers, start=1):
            tin = torch.cat([layers_[k] for k in blk.links[li - 1]], 1)
            prefix = f"base.{b['index']}.layers.{li - 1}"
            y = conv_layer(tin, prefix + ".layer1", comb.layer1, b["ys"][li - 1], b["zs"][li - 1])
            layers_.append(dw_layer(y, prefix + ".layer2", comb.layer2, slices[li], b["dw_zs"][li - 1]))
        dropped = torch.cat([layers_[k] for k in blk.output_slices()], 1) * mask.detach().double()
        x = conv_layer(dropped, f"base.{b['tr_index']}", transition, b["tr_y"], b["tr_z"])
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
    n, up = {}, TAIL_N if tail is not None else 0
    up_slice, up_g = _upstream_counts(blk, up, transition.conv.out_channels)
    tr = f"base.{b['tr_index']}"
    n[tr + ".conv.weight"] = n[tr + ".norm.bias"] = up + pixels[tr]
    n[tr + ".norm.weight"] = up + pixels[tr] + transition.conv.in_channels
    for li, comb in enumerate(blk.layers, start=1):
        p1, p2 = f"base.{b['index']}.layers.{li - 1}.layer1", f"base.{b['index']}.layers.{li - 1}.layer2"
        n[p2 + ".dwconv.weight"] = n[p2 + ".norm.bias"] = up_slice[li] + pixels[p2]
        n[p2 + ".norm.weight"] = up_slice[li] + pixels[p2] + 9
        n[p1 + ".conv.weight"] = n[p1 + ".norm.bias"] = up_g[li] + pixels[p1]
        n[p1 + ".norm.weight"] = up_g[li] + pixels[p1] + comb.layer1.conv.in_channels
    if tail is not None:
        big = max(pixels.values())
        for k in names:
            n.setdefault(k, big + 9)
    after, extra = 0, {}
    for prefix in reversed(order):                                        # the BatchNorms between a layer and the output
        after += pixels[prefix] + 3
        extra[prefix] = after
    for k in names:
        n[k] += extra.get(k.rsplit(".", 2)[0], 0)
    return {k: (g, T, n[k]) for k, g, T in zip(names, grads, Ts)}
