"""float64 restatement of a ResNet identity Bottleneck's backward, with the error bar of
tests/dw_grads_restated.py: for every output element, T = the sum of the absolute values of the products that make it up and
n = their number along the deepest path; |err| <= (n + 8) 2^-24 T.

Only the backward is under test: the block input x and the three stage outputs y1, y2, y3 are the ones the HIP run saved, and
the PReLU masks m(y) = (y > 0 ? 1 : a) are taken from those saved outputs.  Per stage (conv + folded BN + PReLU, stage 3 with
the residual add in front of the PReLU), from the gradient d of its output:

    g = d m(y)                        s = sum d y [y < 0]
    z = scale (*) conv(u, w) + shift, scale = gamma inv, shift = beta - mean scale   ->  d w, d gamma, d beta, d u from g
    dx of the block = g3 + (stage 1's d u);     d a = (s3 + s2 + s1) / a

The linear part (z as a function of u, w, gamma, beta) is differentiated by torch autograd in float64, once on the values and
once on absolute values (T).  Shared by tests/test_resnet_grads_abi.py, tests/test_resnet_grads_gpu.py and
tests/test_resnet_block_grads.py; plain CPU torch."""
import torch
import torch.nn.functional as F

from dw_grads_restated import EPS, assert_within  # noqa: F401  (re-exported)


def prelu_reference(y, dy, a):
    """y, dy (any shape, f32 or f64), slope a -> {"g": (g, T, 1), "dslope_num": (sum dy y [y < 0], sum |dy y| [y < 0], terms + 1)}."""
    y, dy = y.double(), dy.double()
    g = dy * torch.where(y > 0, 1.0, float(a))
    neg = (y < 0).double()
    return {"g": (g, g.abs(), 1), "dslope_num": ((dy * y * neg).sum(), (dy * y * neg).abs().sum(), int(neg.sum()) + 1)}


def conv_stage_reference(u, w, scale, g, pad, gT=None):
    """z = scale[o] * conv2d(u, w, stride 1, pad) (+ shift) in float64: u [N,C,H,W], w [Cout,C,k,k] (torch layout), scale [Cout],
    g [N,Cout,H,W] the masked gradient of z (``gT``: its T, default |g|) -> dict of (gradient, T, n) for du, dw, dscale, dshift;
    n counts the products of THIS stage only (the caller adds what is behind g)."""
    def run(absval):
        f = (lambda t: t.detach().double().abs()) if absval else (lambda t: t.detach().double())
        leaves = [f(t).requires_grad_() for t in (u, w, scale)]
        sh = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
        z = F.conv2d(leaves[0], leaves[1], None, 1, pad) * leaves[2].view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        up = (gT.double() if gT is not None else g.double().abs()) if absval else g.double()
        return torch.autograd.grad(z, leaves + [sh], up)
    grads, Ts = run(False), run(True)
    M = u.shape[0] * u.shape[2] * u.shape[3]
    K = w.shape[1] * w.shape[2] * w.shape[3]
    taps = w.shape[2] * w.shape[3]
    ns = (taps * w.shape[0] + 1, M + 1, M + K, M)
    return {k: (gi, Ti, n) for k, gi, Ti, n in zip(("du", "dw", "dscale", "dshift"), grads, Ts, ns)}


def block_reference(blk, saved, d3, d3T=None, up=0):
    """One identity Bottleneck.  ``blk``: the module in float64 on the CPU (conv{1,2,3}, bn{1,2,3}, relu); ``saved``: dict of
    the saved x, y1, y2, y3 as NCHW tensors; d3 = d loss / d y3 [N,4 width,h,w] with T ``d3T`` (default |d3|) and ``up`` products
    behind it.  -> ({parameter name: (gradient, T, n)}, (dx, dxT, n of dx))."""
    a = float(blk.relu.weight.detach())
    d, dT = d3.double(), (d3.double().abs() if d3T is None else d3T.double())
    out, s_sum, s_T, s_terms = {}, 0.0, 0.0, 0
    g3 = g3T = None
    inputs = {3: saved["y2"], 2: saved["y1"], 1: saved["x"]}
    for i in (3, 2, 1):
        conv, bn = getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}")
        y = saved[f"y{i}"].double()
        m = torch.where(y > 0, 1.0, a)
        g, gT = d * m, dT * m
        up += 1
        neg = (y < 0).double()
        s_sum = s_sum + (d * y * neg).sum()
        s_T = s_T + (d * y * neg).abs().sum()
        s_terms += int(neg.sum())
        if i == 3:
            g3, g3T = g, gT
        inv = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        mean = bn.running_mean.detach().double()
        gamma = bn.weight.detach().double()
        st = conv_stage_reference(inputs[i].double(), conv.weight.detach().double(), gamma * inv, g, conv.padding[0], gT)
        # the fold rule: scale = gamma inv, shift = beta - mean scale
        (dsc, dscT, n_sc), (dsh, dshT, n_sh) = st["dscale"], st["dshift"]
        out[f"conv{i}.weight"] = (st["dw"][0], st["dw"][1], up + st["dw"][2])
        out[f"bn{i}.weight"] = ((dsc - mean * dsh) * inv, (dscT + mean.abs() * dshT) * inv, up + n_sc + 2)
        out[f"bn{i}.bias"] = (dsh, dshT, up + n_sh)
        d, dT = st["du"][0], st["du"][1]
        up += st["du"][2]
    out["relu.weight"] = ((s_sum / a).reshape(1), (s_T / a).reshape(1), s_terms + 1)
    return out, (g3 + d, g3T + dT, up + 1)


def section_reference(blocks, gy):
    """``blocks``: [(prefix, module in float64, saved dict)] in forward order; ``gy`` the gradient of the last block's output
    (NCHW).  -> {prefix + "." + parameter name: (gradient, T, n)}."""
    ref = {}
    d, dT, up = gy.double(), None, 0
    for prefix, blk, saved in reversed(blocks):
        out, (d, dT, up) = block_reference(blk, saved, d, dT, up)
        ref.update({f"{prefix}.{k}": v for k, v in out.items()})
    return ref


def bottleneck_forward_plain(blk, x):
    """The reference's Bottleneck.forward for an identity block, with torch functionals (any dtype) -> (x, y1, y2, y3)."""
    ys, cur = [], x
    for i in (1, 2, 3):
        conv, bn = getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}")
        z = F.batch_norm(F.conv2d(cur, conv.weight, None, conv.stride, conv.padding), bn.running_mean, bn.running_var, bn.weight,
                         bn.bias, False, 0.0, bn.eps)
        if i == 3:
            z = z + x
        cur = F.prelu(z, blk.relu.weight)
        ys.append(cur)
    return ys
