"""The training side of ``ResNet`` (DESIGN.md sections 4.21 and 4.22): the ONE autograd node of its feature map over the
trained Bottlenecks (``train_blocks``: the identity blocks at the end of ``layer4``; ``train_from``: every block from the first
of a stage on, projection blocks included), the copies the node keeps of what ``build_plan`` recorded, and what happens to the
packed weights after an optimizer step.

``build_plan`` records every trained block as a dict: ``name`` ("layer4.2"), ``x`` (the block's input [N,h,w,4 width]), ``ys``
(the three stage outputs y1, y2 [N,h,w,width] and y3 [N,h,w,4 width], each after BN and PReLU, y3 after the residual add too),
``pcs`` (the three ``PackedConv``), ``rot`` (conv2's rotated, scaled image: the 3x3 dgrad's weights), ``slope`` (the PReLU
slope the launches carry by value) and ``bn`` (the three BatchNorms' running mean and 1 / sqrt(var + eps)).  A projection block
(``downsample``; its forward runs conv3 and the shortcut as one stacked GEMM on folded weights) carries ``pcs[2]`` as a plain
pack of conv3 made for the backward, and ``pcd`` (the same of ``downsample.0``), ``stride``, ``s2d`` (conv2's 2x2 phase pack where the
stride is 2; ``rot`` is None then) and ``bn_d``.

The "stem" mode (section 4.23) also records the stem, ``plan.stem_record``: ``x4`` (the staged image [N,H,W,4]), ``y`` (conv1's
output after BN and PReLU [N,OH,OW,64]), ``pc`` (conv1's ``PackedConv``), ``slope`` and ``bn``; the pooled map is the first block's
``x``.

The batch-statistics plan (section 4.24; ``block_record_batch_stats``) records per block ``bnt`` in place of ``bn`` - per stage
what the BatchNorm's backward reads: the raw conv output ``z``, ``mean``, ``invstd``, ``gamma`` (the module's parameter) and ``C`` -
``one`` (the unit scales the conv backward takes), ``rot`` / ``s2d`` made from the unscaled weights, and for a projection block
``pcd``, ``stride`` and ``bnt_d``; the stem record carries ``bnt`` too."""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
from torch.autograd.function import once_differentiable

from .. import _ffi, hip_ops
from .._ffi import TsodError
from ..engine import PackedConv
from .hardnet_grads import _bn_grads, _bn_stats, bnt_copy


def eligible(blk) -> bool:
    """A block ``train_blocks`` can reach: an identity Bottleneck with a dense 3x3 at stride 1."""
    return (len(blk._stage_names) == 3 and blk.conv2.groups == 1 and blk.conv2.stride == (1, 1) and blk.downsample is None)


def eligible_stage(blk) -> bool:
    """A block ``train_from`` can reach: a Bottleneck with a dense 3x3 at stride 1 or 2 whose shortcut is the identity or
    Sequential(1x1 conv with groups 1 and conv2's stride, BatchNorm2d)."""
    if len(blk._stage_names) != 3 or blk.conv2.groups != 1 or blk.conv2.stride not in ((1, 1), (2, 2)):
        return False
    ds = blk.downsample
    if ds is None:
        return blk.conv2.stride == (1, 1)
    return (isinstance(ds, torch.nn.Sequential) and len(ds) == 2 and isinstance(ds[0], torch.nn.Conv2d)
            and isinstance(ds[1], torch.nn.BatchNorm2d) and ds[0].kernel_size == (1, 1) and ds[0].groups == 1
            and ds[0].stride == blk.conv2.stride and ds[0].bias is None)


def block_record(plan, blk, name, x, ys, pcs):
    """What the node needs of one trained block of the plan being built (``_ResidualBlock._emit``)."""
    slope = pcs[0].slope
    if not (math.isfinite(slope) and slope > 0.0):
        raise TsodError(f"{name}: the PReLU slope is {slope}; a trained block needs a finite slope > 0 (its backward takes the "
                        "mask from the saved outputs, and sign(prelu(z)) = sign(z) only then)")
    pc2, pcs = pcs[1], list(pcs)
    ds, rec = blk.downsample, {}
    if ds is not None:
        # the forward's stacked GEMM holds conv3 and the shortcut folded and side by side: the backward reads plain packs and
        # folded scales of its own, made once per (block, device) under the block's name (refresh_packs drops them with the rest)
        if len(pcs) == 2:
            pcs.append(plan.packed(f"{name}.conv3.grad", lambda: PackedConv(blk.conv3.weight, plan.device, bn=blk.bn3)))
        pcd = plan.packed(f"{name}.downsample.grad", lambda: PackedConv(ds[0].weight, plan.device, bn=ds[1]))
        rec = dict(pcd=pcd, stride=pc2.stride, bn_d=_bn_stats(ds[1], pcd.cout, plan.device),
                   s2d=plan.packed(f"{name}.conv2.s2d", lambda: hip_ops.s2d_conv3x3_weight(pc2.w, pc2.scale)) if pc2.stride == 2
                   else None)
    rot = None if pc2.stride == 2 else plan.packed(f"{name}.conv2.rot", lambda: hip_ops.rotate_conv3x3_weight(pc2.w, pc2.scale))
    bn = [_bn_stats(getattr(blk, b), pc.cout, plan.device) for (_, b), pc in zip(blk._stage_names, pcs)]
    return dict(name=name, x=x, ys=list(ys), pcs=pcs, rot=rot, slope=slope, bn=bn, **rec)


def _check_slope(name, slope):
    if not (math.isfinite(slope) and slope > 0.0):
        raise TsodError(f"{name}: the PReLU slope is {slope}; a trained block needs a finite slope > 0 (its backward takes the "
                        "mask from the saved outputs, and sign(prelu(z)) = sign(z) only then)")


def block_record_batch_stats(plan, blk, name, x, ys, pcs, bnts, pcd, bnt_d):
    """``block_record`` for a block of the batch-statistics plan (``_ResidualBlock._emit_batch_stats``): the BatchNorms are not
    folded, so the conv backward runs with unit scale and conv2's dx images are made from the unscaled weight, under cache
    names of their own (dropped with the block's packs by ``refresh_packs``)."""
    slope = pcs[0].slope
    _check_slope(name, slope)
    pc2 = pcs[1]
    one = [plan.packed(f"{name}.one.{pc.cout}", lambda pc=pc: torch.ones(pc.cout, dtype=torch.float32, device=plan.device))
           for pc in pcs]
    rot = s2d = None
    if pc2.stride == 2:
        s2d = plan.packed(f"{name}.conv2.s2d.raw", lambda: hip_ops.s2d_conv3x3_weight(pc2.w, one[1]))
    else:
        rot = plan.packed(f"{name}.conv2.rot.raw", lambda: hip_ops.rotate_conv3x3_weight(pc2.w, one[1]))
    rec = dict(name=name, x=x, ys=list(ys), pcs=list(pcs), rot=rot, s2d=s2d, slope=slope, stride=pc2.stride, bnt=list(bnts),
               one=one)
    if pcd is not None:
        rec.update(pcd=pcd, bnt_d=bnt_d)
    return rec


def block_copy_batch_stats(rec, x=None):
    """``block_copy`` for a record of the batch-statistics plan: every BatchNorm's z, mean, invstd and gamma are copied too (the
    next forward overwrites the first three, an optimizer step the last)."""
    y1, y2, y3 = (t.clone() for t in rec["ys"])
    out = dict(name=rec["name"], x=rec["x"].clone() if x is None else x, y1=y1, y2=y2, y3=y3, w=[pc.w for pc in rec["pcs"]],
               scale=rec["one"], rot=rec["rot"], s2d=rec["s2d"], slope=rec["slope"], stride=rec["stride"],
               bnt=[bnt_copy(b) for b in rec["bnt"]])
    if "pcd" in rec:
        out.update(wd=rec["pcd"].w, bnt_d=bnt_copy(rec["bnt_d"]))
    return out


def stem_record(plan, owner, x4, y, pc, bnt=None):
    """What the node needs of the stem of the plan being built (``ResNet.build_plan`` in the "stem" mode); ``bnt``: the stem's
    BatchNorm ran on batch statistics (section 4.24) - what its backward reads, in place of ``bn``."""
    slope = pc.slope
    if not (math.isfinite(slope) and slope > 0.0):
        raise TsodError(f"relu: the stem's PReLU slope is {slope}; a trained stem needs a finite slope > 0 (its backward takes the "
                        "mask from the saved output, and sign(prelu(z)) = sign(z) only then)")
    if bnt is not None:
        return dict(x4=x4, y=y, pc=pc, slope=slope, bnt=bnt)
    return dict(x4=x4, y=y, pc=pc, slope=slope, bn=_bn_stats(owner.bn1, pc.cout, plan.device))


def stem_copy(rec):
    """The node's own view of the stem record: the activations copied, the pack and scale by reference (``block_copy``)."""
    if "bnt" in rec:
        return dict(x4=rec["x4"].clone(), y=rec["y"].clone(), w=rec["pc"].w, scale=torch.ones_like(rec["pc"].scale),
                    slope=rec["slope"], bnt=bnt_copy(rec["bnt"]))
    return dict(x4=rec["x4"].clone(), y=rec["y"].clone(), w=rec["pc"].w, scale=rec["pc"].scale, slope=rec["slope"], bn=rec["bn"])


STEM_NAMES = ("conv1.weight", "bn1.weight", "bn1.bias", "relu.weight")
STEM_MODULES = ("conv1", "bn1", "relu")                          # what ``refresh_packs`` watches of the stem
STEM_PACK_KEYS = ("conv1", "conv1.fused")                        # ... and the ``_packed_cache`` names their change drops


def block_copy(rec, x=None):
    """The node's own view of a block record: forwards and backwards may interleave in any order.  The activations are copied
    (the plan's buffers are written by the next forward); ``x``: the copy that already exists of the block's input (the previous
    trained block's y3 is the same buffer: one copy serves both, the backward writes into neither).  The packs, scales and the
    rotated image are held by reference: nothing writes them in place - a changed block's packs are dropped and made anew
    (``refresh_packs``), so the objects the forward saw stay as they were for as long as the node holds them."""
    y1, y2, y3 = (t.clone() for t in rec["ys"])
    out = dict(name=rec["name"], x=rec["x"].clone() if x is None else x, y1=y1, y2=y2, y3=y3, w=[pc.w for pc in rec["pcs"]],
               scale=[pc.scale for pc in rec["pcs"]], rot=rec["rot"], slope=rec["slope"], bn=rec["bn"])
    if "pcd" in rec:                                              # a projection block
        out.update(wd=rec["pcd"].w, scaled=rec["pcd"].scale, stride=rec["stride"], s2d=rec["s2d"], bn_d=rec["bn_d"])
    return out


class _ResNetGrads(torch.autograd.Function):
    """The feature map of a training-mode forward as an autograd node over ``trainable_parameters()``.  forward(saved, *params)
    hands out the map the plan computed; backward runs, on the node's OWN copies (``ctx.saved``), per trained block from the
    last one down: tsod_prelu_grad_f32 on y3, conv3's tsod_pw_wgrad_f32 / tsod_pw_dgrad_f32, the mask on y2, conv2's
    tsod_conv3x3_dense_wgrad_f32 and its dx through the forward conv library on the rotated image, the mask on y1, conv1's wgrad,
    and dx = g3 + conv1's dgrad (skipped for the earliest block).  A projection block: the shortcut's
    tsod_pw_wgrad_f32 / tsod_pw_dgrad_f32 from g3 on the rows tsod_pixel_subsample_f32 takes of x; conv2 through
    tsod_conv3x3_strided_wgrad_f32; at stride 2 its dx is the forward conv library on the 2x2 phase pack, read by
    tsod_prelu_grad_d2s_f32; dx = conv1's dgrad, then the shortcut's added by tsod_pixel_upsample_add_f32.  The stem (section
    4.23, where one of its four tensors needs a gradient): the earliest block's dx is the gradient of the pooled map, read by
    tsod_prelu_grad_pool_f32 on the stem's y, then tsod_conv7x7s2_wgrad_f32 on the staged image.  It returns the gradients in
    torch's parameter layouts."""

    @staticmethod
    def forward(ctx, saved, *params):
        ctx.saved = saved
        return saved.pop("out")

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        sv = ctx.saved
        need = dict(zip(sv["names"], ctx.needs_input_grad[1:]))
        out = {}
        d3 = hip_ops.nchw_to_nhwc(gy) if sv["nchw"] else gy.contiguous()
        if sv.get("batch_stats"):
            _backward_batch_stats(sv, need, out, d3)
            return (None,) + tuple(out.get(k) if n else None for k, n in need.items())

        def params_of(prefix, i, d_w, d_sc, d_sh, stats, to_torch):
            if d_w is not None:
                out[f"{prefix}.conv{i}.weight"] = to_torch(d_w)
            if d_sc is not None:                                  # (wanted with dshift: the fold rule needs both)
                out[f"{prefix}.bn{i}.weight"], out[f"{prefix}.bn{i}.bias"] = _bn_grads(d_sc, d_sh, stats, d_sh.numel())
            elif d_sh is not None:
                out[f"{prefix}.bn{i}.bias"] = d_sh

        def wants(prefix, i):
            w, g, b = need[f"{prefix}.conv{i}.weight"], need[f"{prefix}.bn{i}.weight"], need[f"{prefix}.bn{i}.bias"]
            return dict(want_dw=w, want_dscale=g, want_dshift=g or b)

        def pointwise(prefix, i, x, b, g, dx, accumulate, want_dx):
            w = b["w"][i - 1]
            K = w.shape[3]
            dx, d_w, d_sc, d_sh = hip_ops.conv1x1_bn_relu6_grad(x, [(0, K)], w, b["scale"][i - 1], None, g, dx=dx, accumulate=accumulate,
                                                                want_dx=want_dx, **wants(prefix, i))
            params_of(prefix, i, d_w, d_sc, d_sh, b["bn"][i - 1], lambda d: d.view(d.shape[0], d.shape[1], 1, 1))
            return dx

        def shortcut(prefix, b, g3, want_dx):
            """downsample.0 / downsample.1 from g3 -> the shortcut's dx over the subsampled grid (None unless wanted)."""
            w, g, bb = (need[f"{prefix}.downsample.{k}"] for k in ("0.weight", "1.weight", "1.bias"))
            if not (w or g or bb or want_dx):
                return None
            wd = b["wd"]
            xs = b["x"] if b["stride"] == 1 else hip_ops.pixel_subsample(b["x"], b["stride"])
            dxs, d_w, d_sc, d_sh = hip_ops.conv1x1_bn_relu6_grad(xs, [(0, wd.shape[3])], wd, b["scaled"], None, g3,
                                                                 dx=torch.empty_like(xs) if want_dx else None, want_dx=want_dx,
                                                                 want_dw=w, want_dscale=g, want_dshift=g or bb)
            if d_w is not None:
                out[f"{prefix}.downsample.0.weight"] = d_w.view(d_w.shape[0], d_w.shape[1], 1, 1)
            if d_sc is not None:
                out[f"{prefix}.downsample.1.weight"], out[f"{prefix}.downsample.1.bias"] = _bn_grads(d_sc, d_sh, b["bn_d"], d_sh.numel())
            elif d_sh is not None:
                out[f"{prefix}.downsample.1.bias"] = d_sh
            return dxs

        blocks = sv["blocks"]
        stem = sv.get("stem")
        want_stem = stem is not None and any(need[k] for k in STEM_NAMES)
        for bi in range(len(blocks) - 1, -1, -1):
            b = blocks[bi]
            prefix, a = b["name"], b["slope"]
            want_a = need[prefix + ".relu.weight"]
            first = bi == 0 and not want_stem                     # the earliest trained block: nobody wants its dx
            proj = "wd" in b
            g3, s3 = hip_ops.prelu_grad(b["y3"], d3, a, want_dslope=want_a)
            d2 = pointwise(prefix, 3, b["y2"], b, g3, torch.empty_like(b["y2"]), False, True)
            dxs = shortcut(prefix, b, g3, not first) if proj else None
            g2, s2 = hip_ops.prelu_grad(b["y2"], d2, a, want_dslope=want_a)
            w2 = wants(prefix, 2)
            if any(w2.values()):
                if proj:
                    d_w, d_sc, d_sh = hip_ops.conv3x3_strided_wgrad(g2, b["y1"], b["w"][1], b["scale"][1], stride=b["stride"], **w2)
                else:
                    d_w, d_sc, d_sh = hip_ops.conv3x3_dense_wgrad(g2, b["y1"], b["w"][1], b["scale"][1], **w2)
                params_of(prefix, 2, d_w, d_sc, d_sh, b["bn"][1], lambda d: d.permute(0, 3, 1, 2).contiguous())
            if b["rot"] is None:                                  # stride 2: the phase-stacked image, read through the mask pass
                p = hip_ops.conv2d_nhwc(g2, b["s2d"], pad=1, precision=_ffi.PREC_F32)
                g1, s1 = hip_ops.prelu_grad_d2s(b["y1"], p, a, want_dslope=want_a)
            else:
                d1 = hip_ops.conv2d_nhwc(g2, b["rot"], pad=1, precision=_ffi.PREC_F32)
                g1, s1 = hip_ops.prelu_grad(b["y1"], d1, a, want_dslope=want_a)
            if not proj:
                d3 = pointwise(prefix, 1, b["x"], b, g1, None if first else g3.clone(), True, not first)
            else:
                d3 = pointwise(prefix, 1, b["x"], b, g1, None if first else torch.empty_like(b["x"]), False, not first)
                if not first:
                    hip_ops.pixel_upsample_add(d3, dxs, b["stride"])
            if want_a:
                out[prefix + ".relu.weight"] = ((s3 + s2) + s1) / a
        if want_stem:                                             # d3: layer1.0's dx, the gradient of the pooled map
            a, want_a = stem["slope"], need["relu.weight"]
            g, s = hip_ops.prelu_grad_pool(stem["y"], d3, a, want_dslope=want_a)
            w, gm, bt = need["conv1.weight"], need["bn1.weight"], need["bn1.bias"]
            if w or gm or bt:
                d_w, d_sc, d_sh = hip_ops.conv7x7s2_wgrad(g, stem["x4"], stem["w"], stem["scale"], want_dw=w, want_dscale=gm,
                                                          want_dshift=gm or bt)
                if d_w is not None:
                    out["conv1.weight"] = d_w
                if d_sc is not None:
                    out["bn1.weight"], out["bn1.bias"] = _bn_grads(d_sc, d_sh, stem["bn"], d_sh.numel())
                elif d_sh is not None:
                    out["bn1.bias"] = d_sh
            if want_a:
                out["relu.weight"] = s / a
        return (None,) + tuple(out.get(k) if n else None for k, n in need.items())


def _backward_batch_stats(sv, need, out, d3):
    """The backward of the batch-statistics plan into ``out``: today's order per block, with every
    mask + BatchNorm pair as one tsod_bn_prelu_train_grad_f32 where the stage's output gradient exists as a tensor (behind a
    stride-2 3x3 and behind the stem the gathering mask kernel, then tsod_bn_train_grad_f32, which also serves downsample.1 on
    g3), and the conv backward from dz with unit scale."""
    def bn_params(prefix, dgamma, dbeta, C):
        out[prefix + ".weight"], out[prefix + ".bias"] = dgamma[:C], dbeta[:C]

    def stage(prefix, i, b, y, d, want_a, want_g=False):
        """mask and BatchNorm of stage i from (y, d, z) -> (dz, the slope's sum, g or None)"""
        t = b["bnt"][i - 1]
        dz, dgamma, dbeta, s, g = hip_ops.batch_norm_prelu_train_grad(y, d, t["z"], t["mean"], t["invstd"], t["gamma"], b["slope"],
                                                                      C_real=t["C"], want_dslope=want_a, want_g=want_g)
        bn_params(f"{prefix}.bn{i}", dgamma, dbeta, t["C"])
        return dz, s, g

    def plain_bn(prefix, t, g):
        dz, dgamma, dbeta = hip_ops.batch_norm_train_grad(g, t["z"], t["mean"], t["invstd"], t["gamma"], C_real=t["C"])
        bn_params(prefix, dgamma, dbeta, t["C"])
        return dz

    def pointwise(name, x, w, one, dz, dx, accumulate, want_dx):
        dx, d_w, _, _ = hip_ops.conv1x1_bn_relu6_grad(x, [(0, w.shape[3])], w, one, None, dz, dx=dx, accumulate=accumulate,
                                                      want_dx=want_dx, want_dw=need[name], want_dscale=False, want_dshift=False)
        if d_w is not None:
            out[name] = d_w.view(d_w.shape[0], d_w.shape[1], 1, 1)
        return dx

    blocks = sv["blocks"]
    stem = sv.get("stem")
    want_stem = stem is not None and any(need[k] for k in STEM_NAMES)
    for bi in range(len(blocks) - 1, -1, -1):
        b = blocks[bi]
        prefix, a = b["name"], b["slope"]
        want_a = need[prefix + ".relu.weight"]
        first = bi == 0 and not want_stem                         # the earliest trained block: nobody wants its dx
        proj = "wd" in b
        dz3, s3, g3 = stage(prefix, 3, b, b["y3"], d3, want_a, want_g=True)
        dxs = None
        if proj:                                                  # downsample.1 has no activation: the plain grad on g3
            dzd = plain_bn(f"{prefix}.downsample.1", b["bnt_d"], g3)
            xs = b["x"] if b["stride"] == 1 else hip_ops.pixel_subsample(b["x"], b["stride"])
            dxs = pointwise(f"{prefix}.downsample.0.weight", xs, b["wd"], b["scale"][2], dzd,
                            None if first else torch.empty_like(xs), False, not first)
        d2 = pointwise(f"{prefix}.conv3.weight", b["y2"], b["w"][2], b["scale"][2], dz3, torch.empty_like(b["y2"]), False, True)
        dz2, s2, _ = stage(prefix, 2, b, b["y2"], d2, want_a)
        if need[f"{prefix}.conv2.weight"]:
            d_w, _, _ = hip_ops.conv3x3_strided_wgrad(dz2, b["y1"], b["w"][1], b["scale"][1], stride=b["stride"], want_dw=True,
                                                      want_dscale=False, want_dshift=False)
            out[f"{prefix}.conv2.weight"] = d_w.permute(0, 3, 1, 2).contiguous()
        if b["rot"] is None:                                      # stride 2: the phase-stacked image, read through the mask pass
            p = hip_ops.conv2d_nhwc(dz2, b["s2d"], pad=1, precision=_ffi.PREC_F32)
            g1, s1 = hip_ops.prelu_grad_d2s(b["y1"], p, a, want_dslope=want_a)
            dz1 = plain_bn(f"{prefix}.bn1", b["bnt"][0], g1)
        else:
            d1 = hip_ops.conv2d_nhwc(dz2, b["rot"], pad=1, precision=_ffi.PREC_F32)
            dz1, s1, _ = stage(prefix, 1, b, b["y1"], d1, want_a)
        if not proj:
            d3 = pointwise(f"{prefix}.conv1.weight", b["x"], b["w"][0], b["scale"][0], dz1, None if first else g3, True, not first)
        else:
            d3 = pointwise(f"{prefix}.conv1.weight", b["x"], b["w"][0], b["scale"][0], dz1,
                           None if first else torch.empty_like(b["x"]), False, not first)
            if not first:
                hip_ops.pixel_upsample_add(d3, dxs, b["stride"])
        if want_a:
            out[prefix + ".relu.weight"] = ((s3 + s2) + s1) / a
    if want_stem:                                                 # d3: layer1.0's dx, the gradient of the pooled map
        a, want_a = stem["slope"], need["relu.weight"]
        g, s = hip_ops.prelu_grad_pool(stem["y"], d3, a, want_dslope=want_a)
        dz = plain_bn("bn1", stem["bnt"], g)
        if need["conv1.weight"]:
            out["conv1.weight"] = hip_ops.conv7x7s2_wgrad(dz, stem["x4"], stem["w"], stem["scale"], want_dw=True, want_dscale=False,
                                                          want_dshift=False)[0]
        if want_a:
            out["relu.weight"] = s / a


def feature_map_with_grads(plan, nchw, named):
    """The output of the training-mode ``plan`` that just ran, carrying the node over ``named`` (``_trainable_named()``)."""
    out = plan.output_nhwc
    blocks, prev = [], None
    for rec in plan.block_records:
        shared = prev is not None and prev["ys"][2] is rec["x"]
        copy = block_copy_batch_stats if "bnt" in rec else block_copy
        blocks.append(copy(rec, blocks[-1]["y3"] if shared else None))
        prev = rec
    saved = dict(out=hip_ops.nhwc_to_nchw(out) if nchw else out.clone(), nchw=nchw, names=[k for k, _ in named], blocks=blocks)
    if plan.bn_steps:
        saved["batch_stats"] = True
    if getattr(plan, "stem_record", None) is not None:
        saved["stem"] = stem_copy(plan.stem_record)
    return _ResNetGrads.apply(saved, *(p for _, p in named))


# -- packed weights after an optimizer step ---------------------------------------------------------
def versions_of(module) -> tuple:
    return tuple(t._version for t in list(module.parameters()) + list(module.buffers()))


def refresh_packs(owner):
    """Drop what was packed from every watched block (``owner._watched``: the blocks of the widest mode ever set, and in the
    "stem" mode ``conv1`` / ``bn1`` / ``relu``, whose packs are "conv1" and "conv1.fused") whose
    parameters or BatchNorm buffers changed (``_version``) since they were last known to match: the block's entries of
    ``_packed_cache`` (its three packs with their bf16x3 / fp16x2 images, the rotated image), every plan of the owner (a launch
    descriptor carries the slope by value, so no plan survives a step), and ``weights_version`` moves so that a captured graph
    goes stale.  The next forward packs the changed blocks again and assembles its plan from the frozen blocks' packs as they
    are.  It runs at the start of every forward of the owner and in ``ResNet.refresh_packs()``; until one of the two has run
    after a step, ``weights_version`` has not moved and a captured graph replays the old weights.  Nothing while no mode was
    ever set: today's contract for in-place edits (``invalidate_packed``)."""
    watched = owner.__dict__.get("_watched")
    if not watched:
        return
    prefixes, names = [], set()
    for name, seen in watched.items():
        v = versions_of(owner.get_submodule(name))
        if v != seen:
            watched[name] = v
            if name in STEM_MODULES:                              # conv1 / bn1 / relu share the stem's two packs, kept under
                names.update(STEM_PACK_KEYS)                      # names of their own: no "<block>." prefix matches them
            else:
                prefixes.append(name + ".")
    if prefixes or names:
        for key in [k for k in owner._packed_cache if isinstance(k[0], str) and (k[0] in names or k[0].startswith(tuple(prefixes)))]:
            del owner._packed_cache[key]
        owner.__dict__["_plans"] = OrderedDict()
        owner._bump_version()
