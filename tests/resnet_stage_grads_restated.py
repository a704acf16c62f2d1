"""float64 restatement of a ResNet projection Bottleneck's backward and of a section that mixes both
block kinds, with the error bar of tests/resnet_grads_restated.py: |err| <= (n + 8) 2^-24 T.

Notation of section 4.21.  s is the block's stride (on conv2 and on the shortcut), x [N,Cin,H,W], y1 [N,width,H,W], y2 and y3
over the output grid OH = (H - 1) / s + 1.  From d3 = d loss / d y3:

    g3 = d3 m(y3)      conv3 (1x1, input y2) and the shortcut (1x1 at stride s, input x) both from g3
    g2 = d2 m(y2)      conv2 (3x3 at stride s, pad 1, input y1)
    g1 = d1 m(y1)      conv1 (1x1, input x);  dx = conv1's d x + the shortcut's d x;  d a = (s3 + s2 + s1) / a

The linear part of every stage is differentiated by torch autograd in float64, once on the values and once on absolute values
(T).  Shared by tests/test_resnet_stage_grads_abi.py, tests/test_resnet_stage_grads_gpu.py and
tests/test_resnet_stage_block_grads.py; plain CPU torch."""
import torch
import torch.nn.functional as F

from resnet_grads_restated import assert_within, block_reference  # noqa: F401  (assert_within: re-exported)


def strided_stage_reference(u, w, scale, g, stride, pad, gT=None):
    """resnet_grads_restated.conv_stage_reference with a stride: z = scale[o] * conv2d(u, w, stride, pad) (+ shift) in float64,
    g [N,Cout,OH,OW] the masked gradient of z -> dict of (gradient, T, n) for du, dw, dscale, dshift.  n counts the products of
    this stage only: an element of du is reached by at most ceil(k / stride)^2 taps, the parameter sums run over the OUTPUT
    pixels."""
    def run(absval):
        f = (lambda t: t.detach().double().abs()) if absval else (lambda t: t.detach().double())
        leaves = [f(t).requires_grad_() for t in (u, w, scale)]
        sh = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
        z = F.conv2d(leaves[0], leaves[1], None, stride, pad) * leaves[2].view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        up = (gT.double() if gT is not None else g.double().abs()) if absval else g.double()
        return torch.autograd.grad(z, leaves + [sh], up)
    grads, Ts = run(False), run(True)
    M = g.shape[0] * g.shape[2] * g.shape[3]
    K = w.shape[1] * w.shape[2] * w.shape[3]
    taps = (-(-w.shape[2] // stride)) * (-(-w.shape[3] // stride))
    ns = (taps * w.shape[0] + 1, M + 1, M + K, M)
    return {k: (gi, Ti, n) for k, gi, Ti, n in zip(("du", "dw", "dscale", "dshift"), grads, Ts, ns)}


def projection_block_reference(blk, saved, d3, d3T=None, up=0):
    """One projection Bottleneck.  Arguments and results as resnet_grads_restated.block_reference; the thirteen names."""
    a = float(blk.relu.weight.detach())
    s = blk.conv2.stride[0]
    d, dT = d3.double(), (d3.double().abs() if d3T is None else d3T.double())
    out, s_sum, s_T, s_terms = {}, 0.0, 0.0, 0
    dxs = dxsT = None
    inputs = {3: saved["y2"], 2: saved["y1"], 1: saved["x"]}

    def fold(prefix_conv, prefix_bn, conv, bn, st, up):
        inv = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        mean = bn.running_mean.detach().double()
        (dsc, dscT, n_sc), (dsh, dshT, n_sh) = st["dscale"], st["dshift"]
        out[f"{prefix_conv}.weight"] = (st["dw"][0], st["dw"][1], up + st["dw"][2])
        out[f"{prefix_bn}.weight"] = ((dsc - mean * dsh) * inv, (dscT + mean.abs() * dshT) * inv, up + n_sc + 2)
        out[f"{prefix_bn}.bias"] = (dsh, dshT, up + n_sh)

    def stage(conv, bn, u, g, gT):
        inv = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        return strided_stage_reference(u.double(), conv.weight.detach().double(), bn.weight.detach().double() * inv, g,
                                       conv.stride[0], conv.padding[0], gT)

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
        if i == 3:                                                # the shortcut hangs on g3 too
            ds_conv, ds_bn = blk.downsample[0], blk.downsample[1]
            assert ds_conv.stride[0] == s
            sd = stage(ds_conv, ds_bn, saved["x"], g, gT)
            fold("downsample.0", "downsample.1", ds_conv, ds_bn, sd, up)
            dxs, dxsT = sd["du"][0], sd["du"][1]
        st = stage(conv, bn, inputs[i], g, gT)
        fold(f"conv{i}", f"bn{i}", conv, bn, st, up)
        d, dT = st["du"][0], st["du"][1]
        up += st["du"][2]
    out["relu.weight"] = ((s_sum / a).reshape(1), (s_T / a).reshape(1), s_terms + 1)
    return out, (d + dxs, dT + dxsT, up + 1)


def section_reference(blocks, gy):
    """``blocks``: [(prefix, module in float64, saved dict)] in forward order, identity and projection Bottlenecks mixed; ``gy``
    the gradient of the last block's output (NCHW).  -> {prefix + "." + parameter name: (gradient, T, n)}."""
    ref = {}
    d, dT, up = gy.double(), None, 0
    for prefix, blk, saved in reversed(blocks):
        one = block_reference if blk.downsample is None else projection_block_reference
        out, (d, dT, up) = one(blk, saved, d, dT, up)
        ref.update({f"{prefix}.{k}": v for k, v in out.items()})
    return ref


def projection_forward_plain(blk, x):
    """The reference's Bottleneck.forward for a projection block, with torch functionals (any dtype) -> [y1, y2, y3]."""
    def bn_of(bn, z):
        return F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    ds_conv, ds_bn = blk.downsample[0], blk.downsample[1]
    identity = bn_of(ds_bn, F.conv2d(x, ds_conv.weight, None, ds_conv.stride, ds_conv.padding))
    ys, cur = [], x
    for i in (1, 2, 3):
        conv, bn = getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}")
        z = bn_of(bn, F.conv2d(cur, conv.weight, None, conv.stride, conv.padding))
        if i == 3:
            z = z + identity
        cur = F.prelu(z, blk.relu.weight)
        ys.append(cur)
    return ys
