"""The training side of ``ResNet`` (DESIGN.md sections 4.21 - 4.24): the ONE autograd node of its feature map over the trained
Bottlenecks (``train_blocks``: the identity blocks at the end of ``layer4``; ``train_from``: every block from the first of a stage
on, projection blocks included), the copies the node keeps of what ``build_plan`` recorded, and what happens to the packed
weights after an optimizer step.  There is one record, one copy and one backward walk for both plans - BatchNorm folded, and
BatchNorm on batch statistics (section 4.24, "One walk").

``build_plan`` records every trained block as a dict (``block_record``): ``name`` ("layer4.2"), ``x`` (the block's input
[N,h,w,4 width]), ``ys`` (the three stage outputs y1, y2 [N,h,w,width] and y3 [N,h,w,4 width], each after BN and PReLU, y3 after
the residual add too), ``pcs`` (the three ``PackedConv``), ``scale`` (the three scales the conv backward takes), ``rot`` (conv2's
rotated image: the 3x3 dgrad's weights) or, where conv2's stride is 2, ``s2d`` (its 2x2 phase pack), ``stride``, ``slope`` (the
PReLU slope the launches carry by value) and ``pcd`` (``downsample.0``'s pack; None for an identity block).
  * Folded: ``scale`` is the packs' folded scales (``rot`` / ``s2d`` carry conv2's), ``bn`` the three BatchNorms' running mean and
    1 / sqrt(var + eps), ``bn_d`` the same of ``downsample.1``.  A projection block's forward runs conv3 and the shortcut as one
    stacked GEMM on folded weights, so ``pcs[2]`` and ``pcd`` are plain packs made for the backward.
  * Batch statistics: ``scale`` is ones (``rot`` / ``s2d`` hold the unscaled weight, under cache names of their own), ``bnt`` is per
    stage what the BatchNorm's backward reads - the raw conv output ``z``, ``mean``, ``invstd``, ``gamma`` (the module's parameter)
    and ``C`` - and ``bnt_d`` the same of ``downsample.1``.

The "stem" mode (section 4.23) also records the stem, ``plan.stem_record``: ``x4`` (the staged image [N,H,W,4]), ``y`` (conv1's
output after BN and PReLU [N,OH,OW,64]), ``pc`` (conv1's ``PackedConv``), ``slope`` and ``bn`` or ``bnt``; the pooled map is the first
block's ``x``."""
from __future__ import annotations

import math
from collections import OrderedDict
from types import SimpleNamespace

import torch
from torch.autograd.function import once_differentiable

from .. import _ffi, hip_ops
from .._ffi import TsodError
from ..engine import PackedConv, bn_fold_grads, bn_fold_stats, bnt_copy


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


def _check_slope(slope, whose, what, saved):
    if not (math.isfinite(slope) and slope > 0.0):
        raise TsodError(f"{whose} PReLU slope is {slope}; a trained {what} needs a finite slope > 0 (its backward takes the "
                        f"mask from the saved {saved}, and sign(prelu(z)) = sign(z) only then)")


def block_record(plan, blk, name, x, ys, pcs, bnts=None, pcd=None, bnt_d=None):
    """What the node needs of one trained block of the plan being built (``_ResidualBlock._emit``); ``bnts``: the block ran on
    batch statistics (``_emit_batch_stats``) - what its three BatchNorms' backwards read, with ``pcd`` / ``bnt_d`` of a projection
    block's shortcut.  What is made here is cached under the block's name: ``refresh_packs`` drops it with the block's packs."""
    pcs, ds = list(pcs), blk.downsample
    pc2, slope = pcs[1], pcs[0].slope
    _check_slope(slope, f"{name}: the", "block", "outputs")
    tag = "" if bnts is None else ".raw"
    if bnts is not None:                       # not folded: the conv backward runs with unit scale, conv2's dx on the unscaled weight
        scale = [plan.packed(f"{name}.one.{pc.cout}", lambda pc=pc: torch.ones(pc.cout, dtype=torch.float32, device=plan.device))
                 for pc in pcs]
        bn = dict(bnt=list(bnts), bnt_d=bnt_d)
    else:
        if ds is not None:
            # the forward's stacked GEMM holds conv3 and the shortcut folded and side by side: the backward reads plain packs and
            # folded scales of its own, made once per (block, device)
            if len(pcs) == 2:
                pcs.append(plan.packed(f"{name}.conv3.grad", lambda: PackedConv(blk.conv3.weight, plan.device, bn=blk.bn3)))
            pcd = plan.packed(f"{name}.downsample.grad", lambda: PackedConv(ds[0].weight, plan.device, bn=ds[1]))
        scale = [pc.scale for pc in pcs]
        bn = dict(bn=[bn_fold_stats(getattr(blk, b), pc.cout, plan.device) for (_, b), pc in zip(blk._stage_names, pcs)],
                  bn_d=None if ds is None else bn_fold_stats(ds[1], pcd.cout, plan.device))
    rot = s2d = None
    if pc2.stride == 2:
        s2d = plan.packed(f"{name}.conv2.s2d{tag}", lambda: hip_ops.s2d_conv3x3_weight(pc2.w, scale[1]))
    else:
        rot = plan.packed(f"{name}.conv2.rot{tag}", lambda: hip_ops.rotate_conv3x3_weight(pc2.w, scale[1]))
    return dict(name=name, x=x, ys=list(ys), pcs=pcs, scale=scale, rot=rot, s2d=s2d, slope=slope, stride=pc2.stride, pcd=pcd, **bn)


def block_copy(rec, x=None):
    """The node's own view of a block record: forwards and backwards may interleave in any order.  The activations are copied
    (the plan's buffers are written by the next forward), and so are a batch-statistics BatchNorm's z, mean, invstd (the next
    forward overwrites them) and gamma (an optimizer step does); ``x``: the copy that already exists of the block's input (the
    previous trained block's y3 is the same buffer: one copy serves both, the backward writes into neither).  The packs, scales
    and the rotated image are held by reference: nothing writes them in place - a changed block's packs are dropped and made
    anew (``refresh_packs``), so the objects the forward saw stay as they were for as long as the node holds them.  The keys are
    the documented ones of either plan (``ResNet.set_train_mode``)."""
    y1, y2, y3 = (t.clone() for t in rec["ys"])
    out = dict(name=rec["name"], x=rec["x"].clone() if x is None else x, y1=y1, y2=y2, y3=y3, w=[pc.w for pc in rec["pcs"]],
               scale=rec["scale"], rot=rec["rot"], slope=rec["slope"])
    pcd, geometry = rec["pcd"], dict(stride=rec["stride"], s2d=rec["s2d"])
    if "bnt" in rec:
        out.update(geometry, bnt=[bnt_copy(b) for b in rec["bnt"]])
        return out if pcd is None else dict(out, wd=pcd.w, bnt_d=bnt_copy(rec["bnt_d"]))
    out["bn"] = rec["bn"]                                         # (stride and s2d: with a projection block's keys only)
    return out if pcd is None else dict(out, **geometry, wd=pcd.w, scaled=pcd.scale, bn_d=rec["bn_d"])


def stem_record(plan, owner, x4, y, pc, bnt=None):
    """What the node needs of the stem of the plan being built (``ResNet.build_plan`` in the "stem" mode); ``bnt``: the stem's
    BatchNorm ran on batch statistics (section 4.24) - what its backward reads, in place of ``bn``."""
    _check_slope(pc.slope, "relu: the stem's", "stem", "output")
    bn = dict(bn=bn_fold_stats(owner.bn1, pc.cout, plan.device)) if bnt is None else dict(bnt=bnt)
    return dict(x4=x4, y=y, pc=pc, slope=pc.slope, **bn)


def stem_copy(rec):
    """The node's own view of the stem record: the activations copied, the pack and scale by reference (``block_copy``)."""
    pc = rec["pc"]
    bn = dict(scale=pc.scale, bn=rec["bn"]) if "bn" in rec else dict(scale=torch.ones_like(pc.scale), bnt=bnt_copy(rec["bnt"]))
    return dict(x4=rec["x4"].clone(), y=rec["y"].clone(), w=pc.w, slope=rec["slope"], **bn)


STEM_NAMES = ("conv1.weight", "bn1.weight", "bn1.bias", "relu.weight")
STEM_MODULES = ("conv1", "bn1", "relu")                          # what ``refresh_packs`` watches of the stem
STEM_PACK_KEYS = ("conv1", "conv1.fused")                        # ... and the ``_packed_cache`` names their change drops
_NO_BN = (None, None, None)


def _folded(need, out):
    """The walk's two variant pieces where BatchNorm is folded into the convs: the mask alone stands between a stage's (y, d) and
    its conv backward, which is asked for dscale / dshift too - ``bn*.weight`` / ``.bias`` follow by the fold rule (``params_of``)."""
    def stage(bn, t, y, d, a, want_a, want_g=False):
        g, s = hip_ops.prelu_grad(y, d, a, want_dslope=want_a)
        return g, s, g

    def wants(conv, bn):
        w, g, b = need[conv + ".weight"], need[bn + ".weight"], need[bn + ".bias"]
        return dict(want_dw=w, want_dscale=g, want_dshift=g or b)
    # this plan's own launch order: an identity block's conv2 takes the dense wgrad, the shortcut runs after conv3's dgrad and only
    # where something of it is wanted, and conv1's dgrad is added into a copy of g3
    return SimpleNamespace(stage=stage, behind_mask=lambda bn, t, g: g, wants=wants, dense_wgrad=True, shortcut_first=False,
                           shortcut_always=False, own_g3=False)


def _batch_stats(need, out):
    """... where BatchNorm ran on batch statistics: every mask + BatchNorm pair is one
    tsod_bn_prelu_train_grad_f32 where the stage's output gradient exists as a tensor (behind a gathering mask - a stride-2 3x3,
    the stem's pool - and for downsample.1 on g3, tsod_bn_train_grad_f32), ``bn*.weight`` / ``.bias`` are its dgamma / dbeta, and
    the conv backward is asked for dW only, from dz with unit scale."""
    def stage(bn, t, y, d, a, want_a, want_g=False):
        dz, dgamma, dbeta, s, g = hip_ops.batch_norm_prelu_train_grad(y, d, t["z"], t["mean"], t["invstd"], t["gamma"], a,
                                                                      C_real=t["C"], want_dslope=want_a, want_g=want_g)
        out[bn + ".weight"], out[bn + ".bias"] = dgamma[:t["C"]], dbeta[:t["C"]]
        return dz, s, g

    def behind_mask(bn, t, g):
        dz, dgamma, dbeta = hip_ops.batch_norm_train_grad(g, t["z"], t["mean"], t["invstd"], t["gamma"], C_real=t["C"])
        out[bn + ".weight"], out[bn + ".bias"] = dgamma[:t["C"]], dbeta[:t["C"]]
        return dz

    def wants(conv, bn):
        return dict(want_dw=need[conv + ".weight"], want_dscale=False, want_dshift=False)
    # this plan's own launch order: every conv2 takes the strided wgrad, the shortcut runs before conv3's dgrad and always (its
    # BatchNorm's backward does), and conv1's dgrad is added into g3 itself, a fresh g_out nobody reads afterwards
    return SimpleNamespace(stage=stage, behind_mask=behind_mask, wants=wants, dense_wgrad=False, shortcut_first=True,
                           shortcut_always=True, own_g3=True)


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
    tsod_prelu_grad_pool_f32 on the stem's y, then tsod_conv7x7s2_wgrad_f32 on the staged image.  That is the folded plan's walk
    (``_folded``); the batch-statistics plan's (``_batch_stats``) is the same loop with its own two pieces.  It returns the
    gradients in torch's parameter layouts."""

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
        v = (_batch_stats if sv.get("batch_stats") else _folded)(need, out)
        stage, behind_mask, wants = v.stage, v.behind_mask, v.wants

        def params_of(conv, bn, d_w, d_sc, d_sh, stats):
            if d_w is not None:
                out[conv + ".weight"] = d_w
            if d_sc is not None:                                  # (wanted with dshift: the fold rule needs both)
                out[bn + ".weight"], out[bn + ".bias"] = bn_fold_grads(d_sc, d_sh, stats, d_sh.numel())
            elif d_sh is not None:
                out[bn + ".bias"] = d_sh

        def pointwise(conv, bn, x, w, scale, stats, g, dx, accumulate, want_dx, want):
            dx, d_w, d_sc, d_sh = hip_ops.conv1x1_bn_relu6_grad(x, [(0, w.shape[3])], w, scale, None, g, dx=dx, accumulate=accumulate,
                                                                want_dx=want_dx, **want)
            params_of(conv, bn, None if d_w is None else d_w.view(d_w.shape[0], d_w.shape[1], 1, 1), d_sc, d_sh, stats)
            return dx

        def shortcut(prefix, b, g3, want_dx):
            """downsample.0 / downsample.1 from g3 -> the shortcut's dx over the subsampled grid (None unless wanted)."""
            conv, bn = prefix + ".downsample.0", prefix + ".downsample.1"
            want = wants(conv, bn)
            if not (v.shortcut_always or want_dx or any(want.values())):
                return None
            g = behind_mask(bn, b.get("bnt_d"), g3)               # (downsample.1 has no activation)
            xs = b["x"] if b["stride"] == 1 else hip_ops.pixel_subsample(b["x"], b["stride"])
            return pointwise(conv, bn, xs, b["wd"], b["scaled"] if "scaled" in b else b["scale"][2], b.get("bn_d"), g,   # (or conv3's ones)
                             torch.empty_like(xs) if want_dx else None, False, want_dx, want)

        blocks, stem = sv["blocks"], sv.get("stem")
        want_stem = stem is not None and any(need[k] for k in STEM_NAMES)
        for bi in range(len(blocks) - 1, -1, -1):
            b = blocks[bi]
            prefix, a, w, scale = b["name"], b["slope"], b["w"], b["scale"]
            bnt, bn = b.get("bnt", _NO_BN), b.get("bn", _NO_BN)
            conv1, conv2, conv3, bn1, bn2, bn3 = (f"{prefix}.{k}" for k in ("conv1", "conv2", "conv3", "bn1", "bn2", "bn3"))
            want_a = need[prefix + ".relu.weight"]
            first = bi == 0 and not want_stem                     # the earliest trained block: nobody wants its dx
            proj = "wd" in b
            dz3, s3, g3 = stage(bn3, bnt[2], b["y3"], d3, a, want_a, True)
            dxs = shortcut(prefix, b, g3, not first) if proj and v.shortcut_first else None
            d2 = pointwise(conv3, bn3, b["y2"], w[2], scale[2], bn[2], dz3, torch.empty_like(b["y2"]), False, True, wants(conv3, bn3))
            if proj and not v.shortcut_first:
                dxs = shortcut(prefix, b, g3, not first)
            dz2, s2, _ = stage(bn2, bnt[1], b["y2"], d2, a, want_a)
            w2 = wants(conv2, bn2)
            if any(w2.values()):
                if v.dense_wgrad and not proj:
                    d_w, d_sc, d_sh = hip_ops.conv3x3_dense_wgrad(dz2, b["y1"], w[1], scale[1], **w2)
                else:
                    d_w, d_sc, d_sh = hip_ops.conv3x3_strided_wgrad(dz2, b["y1"], w[1], scale[1], stride=b["stride"], **w2)
                params_of(conv2, bn2, None if d_w is None else d_w.permute(0, 3, 1, 2).contiguous(), d_sc, d_sh, bn[1])
            if b["rot"] is None:                                  # stride 2: the phase-stacked image, read through the mask pass
                p = hip_ops.conv2d_nhwc(dz2, b["s2d"], pad=1, precision=_ffi.PREC_F32)
                g1, s1 = hip_ops.prelu_grad_d2s(b["y1"], p, a, want_dslope=want_a)
                dz1 = behind_mask(bn1, bnt[0], g1)
            else:
                d1 = hip_ops.conv2d_nhwc(dz2, b["rot"], pad=1, precision=_ffi.PREC_F32)
                dz1, s1, _ = stage(bn1, bnt[0], b["y1"], d1, a, want_a)
            # dx = conv1's dgrad added into g3 (an identity block), or written and the shortcut's dx added over its grid
            dx = None if first else torch.empty_like(b["x"]) if proj else g3 if v.own_g3 else g3.clone()
            d3 = pointwise(conv1, bn1, b["x"], w[0], scale[0], bn[0], dz1, dx, not proj, not first, wants(conv1, bn1))
            if proj and not first:
                hip_ops.pixel_upsample_add(d3, dxs, b["stride"])
            if want_a:
                out[prefix + ".relu.weight"] = ((s3 + s2) + s1) / a
        if want_stem:                                             # d3: layer1.0's dx, the gradient of the pooled map
            a, want_a = stem["slope"], need["relu.weight"]
            g, s = hip_ops.prelu_grad_pool(stem["y"], d3, a, want_dslope=want_a)
            dz = behind_mask("bn1", stem.get("bnt"), g)
            want = wants("conv1", "bn1")
            if any(want.values()):
                params_of("conv1", "bn1", *hip_ops.conv7x7s2_wgrad(dz, stem["x4"], stem["w"], stem["scale"], **want), stem.get("bn"))
            if want_a:
                out["relu.weight"] = s / a
        return (None,) + tuple(out.get(k) if n else None for k, n in need.items())


def feature_map_with_grads(plan, nchw, named):
    """The output of the training-mode ``plan`` that just ran, carrying the node over ``named`` (``_trainable_named()``)."""
    out = plan.output_nhwc
    blocks, prev = [], None
    for rec in plan.block_records:
        shared = prev is not None and prev["ys"][2] is rec["x"]
        blocks.append(block_copy(rec, blocks[-1]["y3"] if shared else None))
        prev = rec
    saved = dict(out=hip_ops.nhwc_to_nchw(out) if nchw else out.clone(), nchw=nchw, names=[k for k, _ in named], blocks=blocks)
    if plan.batch_stats:
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
