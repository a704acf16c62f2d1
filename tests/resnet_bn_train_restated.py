"""float64 restatement of the backward of ResNet's trainable section with batch-statistics BatchNorm,
in the style of tests/resnet_stem_grads_restated.py's section and tests/bn_train_restated.py's ``bn_section_reference``, with the
bar of sections 4.21 - 4.23: |err| <= (n + 8) 2^-24 T.

Only the backward is under test: every BatchNorm's raw input z, every stage output y, the block inputs and the image are the
ones the HIP run saved (``f.grad_fn.saved``); masks and pool winners come from the saved outputs.  Per stage, from the
gradient d of its output:

    g = d m(y),  m(y) = (y > 0 ? 1 : a)              s = sum d y [y < 0]
    xhat = (z - mean z) / sqrt(var z + eps),  k = gamma / sqrt(var z + eps)      (biased variance, over N, H, W)
    d gamma = sum g xhat     d beta = sum g     dz = k (g - mean g - xhat mean(g xhat))
    d w, d u from dz through the conv alone (unit scale)

A block's stage 3 hands g3 to the residual branch too: the identity (dx = g3 + stage 1's d u) or downsample.1's BatchNorm on its
own saved z and then downsample.0.  d a = (s3 + s2 + s1) / a.  T takes every BatchNorm term absolutely (|k| (gT + mean gT +
|xhat| mean(gT |xhat|)), sum gT |xhat|, sum gT); n grows by pixels + 3 per BatchNorm on the way (the two means over the pixels
that enter every dz).  Plain CPU torch."""
import torch
import torch.nn.functional as F

from resnet_stem_grads_restated import assert_within, prelu_pool_reference, strided_stage_reference  # noqa: F401


def bn_stage_reference(z, gamma, eps, g, gT):
    """A batch-statistics BatchNorm's backward from its saved input z [N,C,H,W] (float64 on entry or not), the gradient g of its
    output and g's T -> dict of (value, T, n of THIS step) for dz, dgamma, dbeta."""
    z, g, gT, gamma = z.double(), g.double(), gT.double(), gamma.detach().double()
    d = (0, 2, 3)
    inv = 1.0 / torch.sqrt(z.var(d, unbiased=False, keepdim=True) + eps)
    xhat = (z - z.mean(d, keepdim=True)) * inv
    k = gamma.view(1, -1, 1, 1) * inv
    pixels = z.shape[0] * z.shape[2] * z.shape[3]
    dz = k * (g - g.mean(d, keepdim=True) - xhat * (g * xhat).mean(d, keepdim=True))
    dzT = k.abs() * (gT + gT.mean(d, keepdim=True) + xhat.abs() * (gT * xhat.abs()).mean(d, keepdim=True))
    return dict(dz=(dz, dzT, pixels + 3), dgamma=((g * xhat).sum(d), (gT * xhat.abs()).sum(d), pixels + 1),
                dbeta=(g.sum(d), gT.sum(d), pixels))


def _conv(conv, u, dz, dzT):
    one = torch.ones(conv.out_channels, dtype=torch.float64)
    return strided_stage_reference(u.double(), conv.weight.detach().double(), one, dz, conv.stride[0], conv.padding[0], dzT)


def block_reference(blk, saved, d3, d3T=None, up=0):
    """One Bottleneck, identity or projection.  ``saved``: x, y1, y2, y3, z1, z2, z3 and (projection) zd as NCHW tensors.
    Arguments and results as resnet_grads_restated.block_reference."""
    a = float(blk.relu.weight.detach())
    d, dT = d3.double(), (d3.double().abs() if d3T is None else d3T.double())
    out, s_sum, s_T, s_terms = {}, 0.0, 0.0, 0
    side = sideT = None
    inputs = {3: saved["y2"], 2: saved["y1"], 1: saved["x"]}
    for i in (3, 2, 1):
        conv, bn = getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}")
        y = saved[f"y{i}"].double()
        m = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, a))      # (float64: two Python scalars would give float32)
        g, gT = d * m, dT * m
        up += 1
        neg = (y < 0).double()
        s_sum = s_sum + (d * y * neg).sum()
        s_T = s_T + (d * y * neg).abs().sum()
        s_terms += int(neg.sum())
        if i == 3:
            if blk.downsample is None:
                side, sideT = g, gT
            else:
                ds_conv, ds_bn = blk.downsample[0], blk.downsample[1]
                bd = bn_stage_reference(saved["zd"], ds_bn.weight, ds_bn.eps, g, gT)
                out["downsample.1.weight"] = bd["dgamma"][:2] + (up + bd["dgamma"][2],)
                out["downsample.1.bias"] = bd["dbeta"][:2] + (up + bd["dbeta"][2],)
                sd = _conv(ds_conv, saved["x"], bd["dz"][0], bd["dz"][1])
                out["downsample.0.weight"] = (sd["dw"][0], sd["dw"][1], up + bd["dz"][2] + sd["dw"][2])
                side, sideT = sd["du"][0], sd["du"][1]
        b = bn_stage_reference(saved[f"z{i}"], bn.weight, bn.eps, g, gT)
        out[f"bn{i}.weight"] = b["dgamma"][:2] + (up + b["dgamma"][2],)
        out[f"bn{i}.bias"] = b["dbeta"][:2] + (up + b["dbeta"][2],)
        up += b["dz"][2]
        st = _conv(conv, inputs[i], b["dz"][0], b["dz"][1])
        out[f"conv{i}.weight"] = (st["dw"][0], st["dw"][1], up + st["dw"][2])
        d, dT = st["du"][0], st["du"][1]
        up += st["du"][2]
    out["relu.weight"] = ((s_sum / a).reshape(1), (s_T / a).reshape(1), s_terms + 1)
    return out, (d + side, dT + sideT, up + 1)


def stem_reference(owner, saved, dp, dpT=None, up=0):
    """The stem: ``saved`` x (the image), y (conv1's output after BN and PReLU) and z (conv1's raw output), NCHW."""
    a = float(owner.relu.weight.detach())
    pr = prelu_pool_reference(saved["y"], dp, a, dpT, up)
    g, gT, up = pr["g"]
    b = bn_stage_reference(saved["z"], owner.bn1.weight, owner.bn1.eps, g, gT)
    st = _conv(owner.conv1, saved["x"], b["dz"][0], b["dz"][1])
    s, sT, n_s = pr["dslope_num"]
    return {"conv1.weight": (st["dw"][0], st["dw"][1], up + b["dz"][2] + st["dw"][2]),
            "bn1.weight": b["dgamma"][:2] + (up + b["dgamma"][2],), "bn1.bias": b["dbeta"][:2] + (up + b["dbeta"][2],),
            "relu.weight": ((s / a).reshape(1), (sT / a).reshape(1), n_s)}


def section_reference(stem, blocks, gy):
    """``blocks``: [(prefix, module in float64, saved dict)] in forward order; ``stem``: None or (module with conv1 / bn1 / relu in
    float64, saved dict); ``gy`` the gradient of the last block's output (NCHW).  -> {parameter name: (gradient, T, n)}."""
    ref = {}
    d, dT, up = gy.double(), None, 0
    for prefix, blk, saved in reversed(blocks):
        out, (d, dT, up) = block_reference(blk, saved, d, dT, up)
        ref.update({f"{prefix}.{k}": v for k, v in out.items()})
    if stem is not None:
        ref.update(stem_reference(stem[0], stem[1], d, dT, up))
    return ref


def block_forward_plain(blk, x, seen=None):
    """The reference's Bottleneck.forward under .train() with torch functionals (any dtype; running statistics untouched)
    -> dict x, y1, y2, y3, z1, z2, z3 (and zd)."""
    def bn_of(bn, z):
        return F.batch_norm(z, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)
    out = dict(x=x)
    identity = x
    if blk.downsample is not None:
        out["zd"] = F.conv2d(x, blk.downsample[0].weight, None, blk.downsample[0].stride)
        identity = bn_of(blk.downsample[1], out["zd"])
    cur = x
    for i in (1, 2, 3):
        conv, bn = getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}")
        out[f"z{i}"] = F.conv2d(cur, conv.weight, None, conv.stride, conv.padding)
        z = bn_of(bn, out[f"z{i}"])
        if i == 3:
            z = z + identity
        cur = out[f"y{i}"] = F.prelu(z, blk.relu.weight)
    return out
