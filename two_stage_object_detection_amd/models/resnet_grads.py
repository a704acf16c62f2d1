"""The training side of ``ResNet``: the ONE autograd node of its feature map over the identity
Bottlenecks at the end of ``layer4``, the copies the node keeps of what ``build_plan`` recorded, and what happens to the packed
weights after an optimizer step.

``build_plan`` records every trained block as a dict: ``name`` ("layer4.2"), ``x`` (the block's input [N,h,w,4 width]), ``ys``
(the three stage outputs y1, y2 [N,h,w,width] and y3 [N,h,w,4 width], each after BN and PReLU, y3 after the residual add too),
``pcs`` (the three ``PackedConv``), ``rot`` (conv2's rotated, scaled image: the 3x3 dgrad's weights), ``slope`` (the PReLU
slope the launches carry by value) and ``bn`` (the three BatchNorms' running mean and 1 / sqrt(var + eps))."""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
from torch.autograd.function import once_differentiable

from .. import _ffi, hip_ops
from .._ffi import TsodError
from .hardnet_grads import _bn_grads, _bn_stats


def eligible(blk) -> bool:
    """A block ``train_blocks`` can reach: an identity Bottleneck with a dense 3x3 at stride 1."""
    return (len(blk._stage_names) == 3 and blk.conv2.groups == 1 and blk.conv2.stride == (1, 1) and blk.downsample is None)


def block_record(plan, blk, name, x, ys, pcs):
    """What the node needs of one trained block of the plan being built (``_ResidualBlock._emit``)."""
    slope = pcs[0].slope
    if not (math.isfinite(slope) and slope > 0.0):
        raise TsodError(f"{name}: the PReLU slope is {slope}; a trained block needs a finite slope > 0 (its backward takes the "
                        "mask from the saved outputs, and sign(prelu(z)) = sign(z) only then)")
    pc2 = pcs[1]
    rot = plan.packed(f"{name}.conv2.rot", lambda: hip_ops.rotate_conv3x3_weight(pc2.w, pc2.scale))
    bn = [_bn_stats(getattr(blk, b), pc.cout, plan.device) for (_, b), pc in zip(blk._stage_names, pcs)]
    return dict(name=name, x=x, ys=list(ys), pcs=list(pcs), rot=rot, slope=slope, bn=bn)


def block_copy(rec):
    """The node's own view of a block record: forwards and backwards may interleave in any order.  The activations are copied
    (the plan's buffers are written by the next forward).  The packs, scales and the rotated image are held by reference:
    nothing writes them in place - a changed block's packs are dropped and made anew (``refresh_packs``), so the objects the
    forward saw stay as they were for as long as the node holds them."""
    y1, y2, y3 = (t.clone() for t in rec["ys"])
    return dict(name=rec["name"], x=rec["x"].clone(), y1=y1, y2=y2, y3=y3, w=[pc.w for pc in rec["pcs"]],
                scale=[pc.scale for pc in rec["pcs"]], rot=rec["rot"], slope=rec["slope"], bn=rec["bn"])


class _ResNetGrads(torch.autograd.Function):
    """The feature map of a training-mode forward as an autograd node over ``trainable_parameters()``.  forward(saved, *params)
    hands out the map the plan computed; backward runs, on the node's OWN copies (``ctx.saved``), per trained block from the
    last one down: tsod_prelu_grad_f32 on y3, conv3's tsod_pw_wgrad_f32 / tsod_pw_dgrad_f32, the mask on y2, conv2's
    tsod_conv3x3_dense_wgrad_f32 and its dx through the forward conv library on the rotated image, the mask on y1, conv1's wgrad,
    and dx = g3 + conv1's dgrad (skipped for the earliest block).  It returns the gradients in torch's parameter layouts."""

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

        blocks = sv["blocks"]
        for bi in range(len(blocks) - 1, -1, -1):
            b = blocks[bi]
            prefix, a = b["name"], b["slope"]
            want_a = need[prefix + ".relu.weight"]
            g3, s3 = hip_ops.prelu_grad(b["y3"], d3, a, want_dslope=want_a)
            d2 = pointwise(prefix, 3, b["y2"], b, g3, torch.empty_like(b["y2"]), False, True)
            g2, s2 = hip_ops.prelu_grad(b["y2"], d2, a, want_dslope=want_a)
            w2 = wants(prefix, 2)
            if any(w2.values()):
                d_w, d_sc, d_sh = hip_ops.conv3x3_dense_wgrad(g2, b["y1"], b["w"][1], b["scale"][1], **w2)
                params_of(prefix, 2, d_w, d_sc, d_sh, b["bn"][1], lambda d: d.permute(0, 3, 1, 2).contiguous())
            d1 = hip_ops.conv2d_nhwc(g2, b["rot"], pad=1, precision=_ffi.PREC_F32)
            g1, s1 = hip_ops.prelu_grad(b["y1"], d1, a, want_dslope=want_a)
            first = bi == 0                                       # the earliest trained block: nobody wants its dx
            d3 = pointwise(prefix, 1, b["x"], b, g1, None if first else g3.clone(), True, not first)
            if want_a:
                out[prefix + ".relu.weight"] = ((s3 + s2) + s1) / a
        return (None,) + tuple(out.get(k) if n else None for k, n in need.items())


def feature_map_with_grads(plan, nchw, named):
    """The output of the training-mode ``plan`` that just ran, carrying the node over ``named`` (``_trainable_named()``)."""
    out = plan.output_nhwc
    saved = dict(out=hip_ops.nhwc_to_nchw(out) if nchw else out.clone(), nchw=nchw, names=[k for k, _ in named],
                 blocks=[block_copy(r) for r in plan.block_records])
    return _ResNetGrads.apply(saved, *(p for _, p in named))


# -- packed weights after an optimizer step ---------------------------------------------------------
def versions_of(module) -> tuple:
    return tuple(t._version for t in list(module.parameters()) + list(module.buffers()))


def refresh_packs(owner):
    """Drop what was packed from every watched block (``owner._watched``: the blocks of the widest ``train_blocks`` ever set) whose
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
    stale = []
    for name, seen in watched.items():
        v = versions_of(owner.get_submodule(name))
        if v != seen:
            watched[name] = v
            stale.append(name + ".")
    if stale:
        for key in [k for k in owner._packed_cache if isinstance(k[0], str) and k[0].startswith(tuple(stale))]:
            del owner._packed_cache[key]
        owner.__dict__["_plans"] = OrderedDict()
        owner._bump_version()
