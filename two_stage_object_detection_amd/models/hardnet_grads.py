"""The training side of ``HarDNetFeatureExtraction`` (DESIGN.md sections 4.17 - 4.19): the ONE autograd node of its feature map,
the copies the node keeps of what ``build_plan`` recorded, and the refresh of the packed weights after an optimizer step.

``build_plan`` records trainable layers in two shapes (``pw_copy`` / ``dw_copy`` make the node's own copies of them):
  * a 1x1 ConvLayer (a HarDBlock layer's ``layer1``, a transition layer, ``base.1``): ``index`` in ``base``, ``rc`` (its pack),
    ``slices`` / ``segs`` / ``seg_real`` (what it gathers from its input buffer), ``cout``, ``y`` / ``y_off`` (its output; None
    where the consumer's record holds it), ``off`` (its slice of the block buffer), ``bn`` (BN statistics);
  * a depthwise layer (``layer2``, the DWConvLayer between blocks, ``base.2``, the tail's two convs - and the tail's pair conv,
    which needs the same facts): ``index``, ``dw`` (its pack), ``stride``, ``C``, ``dw_bn`` (BN statistics or None) and ``x``
    = (input, channel offset) where no 1x1 record holds that input as its ``y`` (the tail), else None.
Where the layer's BatchNorm ran on batch statistics the record carries ``bnt`` (1x1) / ``dw_bnt``
(depthwise) = ``z`` (the conv's raw output [N,h,w,C_pad]), ``mean``, ``invstd``, ``gamma`` (the module's ``weight``), ``C``; its
pack then has unit scale and ``bn`` / ``dw_bn`` are None.  A block whose transition read a dropped copy of its output slices
(active dropout) carries ``dropout``: ``p``, ``ordinal``, ``segs`` [(channel offset, real width, first
logical channel)], ``C`` and ``key`` (the plan's two key words; the node clones them)."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _ffi, hip_ops
from ..engine import bn_fold_grads, bnt_copy


def _conv33_weight(d, C):                                     # [3][3][C_pad] -> torch's [C,1,3,3]
    return d[:, :, :C].reshape(9, C).t().reshape(C, 1, 3, 3)


def pw_copy(rec):
    rc, y = rec["rc"], rec["y"]
    return dict(index=rec["index"], off=rec["off"], cout=rec["cout"], segs=rec["segs"], seg_real=rec["seg_real"],
                slices=rec["slices"], w=rc.w.view(rc.cout, -1).clone(), scale=rc.scale.clone(), bn=rec["bn"],
                y=None if y is None else y[..., rec["y_off"]:rec["y_off"] + rc.cout].clone(), bnt=bnt_copy(rec.get("bnt")))


def dw_copy(rec):
    return dict(rec, dw=tuple(t.clone() if isinstance(t, torch.Tensor) else t for t in rec["dw"]),
                x=None if rec["x"] is None else (rec["x"][0].clone(), rec["x"][1]), dw_bnt=bnt_copy(rec.get("dw_bnt")))


def _bn_train_back(out, prefix, bnt, g, g_off=0):
    """A batch-statistics BatchNorm's backward from the (masked) gradient of its output: its ``weight`` / ``bias`` gradients go
    to ``out`` straight from dgamma / dbeta, dz (the conv's output gradient) is returned."""
    dz, dgamma, dbeta = hip_ops.batch_norm_train_grad(g, bnt["z"], bnt["mean"], bnt["invstd"], bnt["gamma"], g_off=g_off,
                                                      C_real=bnt["C"])
    out[prefix + ".weight"], out[prefix + ".bias"] = dgamma[:bnt["C"]], dbeta[:bnt["C"]]
    return dz


class _BackboneGrads(torch.autograd.Function):
    """The feature map of a training-mode forward as an autograd node over ``trainable_parameters()``.  forward(saved, *params)
    hands out the map the plan computed; backward runs, on the node's OWN copies (``ctx.saved``), the tail (section 4.17:
    tsod_gconv1x1_pair_grad_f32, tsod_dwconv3x3_grad_f32 twice - in "tail" mode the first conv gives no dx, otherwise the masked
    gradient of the last transition layer, tsod_dwconv3x3_grad_act_f32), then per HarDBlock from the last one down (section 4.18):
    the transition's tsod_pw_wgrad_f32 / tsod_pw_dgrad_f32 into a zeroed block-shaped gradient buffer, the layers in descending
    order (depthwise backward with the fused ReLU6 mask, then the 1x1's wgrad and dgrad into the slices it gathered from, added
    in that order) and the ``DWConvLayer`` in front of the block, then the stem (section 4.19).  It returns the gradients in
    torch's parameter layouts (autograd adds them into ``.grad``)."""

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

        def wants(prefix):
            return need[prefix + ".weight"], need[prefix + ".bias"]

        def dw_layer(prefix, x, rec, dy, dy_off):
            """backward of a DWConvLayer whose input x is a ReLU6 output -> that layer's masked gradient"""
            w33, sc, sh = rec["dw"][:3]
            bnt = rec.get("dw_bnt")
            if bnt is not None:                                   # batch statistics: dz first, then the conv with unit scale
                dy, dy_off = _bn_train_back(out, prefix + ".norm", bnt, dy, dy_off), 0
                want = need[prefix + ".dwconv.weight"]
            else:
                want = need[prefix + ".dwconv.weight"] or any(wants(prefix + ".norm"))
            g, d_w, d_sc, d_sh = hip_ops.dwconv3x3_grad(x, w33, sc, sh, rec["stride"], False, dy, want_params=want, dy_off=dy_off,
                                                        act_dx=True)
            if want:
                out[prefix + ".dwconv.weight"] = _conv33_weight(d_w, rec["C"])
                if bnt is None:
                    out[prefix + ".norm.weight"], out[prefix + ".norm.bias"] = bn_fold_grads(d_sc, d_sh, rec["dw_bn"], rec["C"])
            return g

        def pw_layer(prefix, buf, lay, g, dbuf, want_seg):
            """backward of a 1x1 ConvLayer from its masked gradient g: parameter gradients, and dx added into dbuf"""
            want_w, (want_g, want_b) = need[prefix + ".conv.weight"], wants(prefix + ".norm")
            if lay.get("bnt") is not None:                        # batch statistics: dz first, then the conv with unit scale
                g, want_g, want_b = _bn_train_back(out, prefix + ".norm", lay["bnt"], g), False, False
            _, d_w, d_sc, d_sh = hip_ops.conv1x1_bn_relu6_grad(
                buf, lay["segs"], lay["w"], lay["scale"], None, g, seg_real=lay["seg_real"], seg_want=want_seg, cout=lay["cout"],
                dx=dbuf, accumulate=True, want_dx=any(want_seg), want_dw=want_w, want_dscale=want_g, want_dshift=want_g or want_b)
            if want_w:
                out[prefix + ".conv.weight"] = d_w.view(d_w.shape[0], d_w.shape[1], 1, 1)
            if want_g or want_b:
                zero = d_sh if d_sc is None else d_sc
                out[prefix + ".norm.weight"], out[prefix + ".norm.bias"] = bn_fold_grads(zero, d_sh, lay["bn"], lay["cout"])

        # ---- the tail (section 4.17); with trainable blocks the last transition's mask is fused into its first layer's dx gather
        blocks, stem = sv["blocks"], sv.get("stem")
        g0 = hip_ops.nchw_to_nhwc(gy) if sv["nchw"] else gy.contiguous()
        (x0, off0), (a, _), (b, _) = sv["inputs"]
        (w1, _, sh1, _), (w2, _, sh2, _), (wg, bias) = sv["packs"]
        i1, i2, ip = sv["tail_indices"]
        d_b, d_wg, d_bias = hip_ops.gconv1x1_pair_grad(b, wg, g0, want_dw=need[f"base.{ip}.weight"], want_dbias=need[f"base.{ip}.bias"])
        d_a, d_w2, _, d_sh2 = hip_ops.dwconv3x3_grad(a, w2, None, sh2, 2, False, d_b)
        g, d_w1, _, d_sh1 = hip_ops.dwconv3x3_grad(x0, w1, None, sh1, 2, True, d_a, want_dx=bool(blocks), in_off=off0,
                                                   act_dx=bool(blocks))
        C = sv["C"]
        out.update({f"base.{i1}.weight": _conv33_weight(d_w1, C), f"base.{i1}.bias": d_sh1[:C],
                    f"base.{i2}.weight": _conv33_weight(d_w2, C), f"base.{i2}.bias": d_sh2[:C],
                    f"base.{ip}.weight": None if d_wg is None else d_wg.view(-1, 2, 1, 1), f"base.{ip}.bias": d_bias})

        # ---- the blocks, last first; g = the masked gradient of the block's transition layer
        for bi in range(len(blocks) - 1, -1, -1):
            blk = blocks[bi]
            first, buf = bi == 0, blk["buf"]
            dbuf = torch.zeros_like(buf)
            tr = blk["transition"]
            skip0 = first and stem is None                        # the first block's input slice: wanted by the stem only
            drop = blk.get("dropout")
            if drop is None:
                pw_layer(f"base.{tr['index']}", buf, tr, g, dbuf, [not (skip0 and k == 0) for k in tr["slices"]])
            else:
                # active dropout (section 4.26): the transition read a dropped copy of its slices - made again here from the
                # node's key - and its input gradient, the first thing written into dbuf, passes the same mask in place
                mask = dict(segs=drop["segs"], C=drop["C"], ordinal=drop["ordinal"])
                xd = hip_ops.dropout(buf, drop["p"], drop["key"], out=torch.empty_like(buf), **mask)
                pw_layer(f"base.{tr['index']}", xd, tr, g, dbuf, [not (skip0 and k == 0) for k in tr["slices"]])
                del xd
                hip_ops.dropout(dbuf, drop["p"], drop["key"], out=dbuf, **mask)
            for li in range(len(blk["layers"]), 0, -1):
                lay = blk["layers"][li - 1]
                prefix = f"base.{blk['index']}.layers.{li - 1}"
                g = dw_layer(prefix + ".layer2", lay["y"], lay, dbuf, lay["off"])
                pw_layer(prefix + ".layer1", buf, lay, g, dbuf, [not (skip0 and k == 0) for k in lay["slices"]])
            if first:
                break
            prev = blocks[bi - 1]["transition"]
            down = blk["down"]
            if down is not None:                                  # the DWConvLayer between the blocks
                g = dw_layer(f"base.{down['index']}", prev["y"], down, dbuf, 0)
            else:                                                 # the transition wrote slice 0 itself
                g = hip_ops.relu6_grad_mask(prev["y"], dbuf, 0)
        # ---- the stem (section 4.19): base.2 reads slice 0 of the first block's gradient, base.1 is a one-segment 1x1 layer,
        # base.0 has parameter gradients only (tsod_conv3x3_wgrad_f32 takes its mask from the saved output)
        if stem is not None:
            lay1 = stem["base1"]
            g = dw_layer("base.2", lay1["y"], stem, dbuf, 0)
            d0 = torch.zeros_like(stem["y0"])
            pw_layer("base.1", stem["y0"], lay1, g, d0, [True])
            want_w, (want_g, want_b) = need["base.0.conv.weight"], wants("base.0.norm")
            if stem.get("bnt0") is not None:                      # batch statistics: the mask pass, dz, then the conv's dW with
                y0 = stem["y0"]                                   # unit scale and a mask that is open everywhere
                dz = _bn_train_back(out, "base.0.norm", stem["bnt0"], hip_ops.relu6_grad_mask(y0, d0))
                if want_w:
                    out["base.0.conv.weight"] = hip_ops.conv3x3_bn_relu6_grad(
                        stem["x4"], stem["w0"], stem["scale0"], torch.ones_like(y0), dz, stride=2, cout=stem["bnt0"]["C"],
                        want_dscale=False, want_dshift=False)[0]
            elif want_w or want_g or want_b:
                c0 = stem["y0"].shape[3]
                d_w, d_sc, d_sh = hip_ops.conv3x3_bn_relu6_grad(stem["x4"], stem["w0"], stem["scale0"], stem["y0"], d0, stride=2,
                                                                want_dw=want_w, want_dscale=want_g, want_dshift=True)
                out["base.0.conv.weight"] = d_w
                out["base.0.norm.weight"], out["base.0.norm.bias"] = bn_fold_grads(d_sh if d_sc is None else d_sc, d_sh,
                                                                                   stem["bn0"], c0)
        return (None,) + tuple(out.get(k) if n else None for k, n in need.items())


def feature_map_with_grads(plan, nchw, named):
    """The output of the training-mode ``plan`` that just ran, carrying the node over ``named`` (``_trainable_named()``)."""
    out = plan.output_nhwc
    tail = [dw_copy(r) for r in plan.tail]
    saved = dict(out=hip_ops.nhwc_to_nchw(out) if nchw else out.clone(), nchw=nchw, names=[k for k, _ in named],
                 inputs=[t["x"] for t in tail], packs=[t["dw"] for t in tail], tail_indices=tuple(t["index"] for t in tail),
                 C=tail[0]["C"],
                 blocks=[dict(index=b["index"], buf=b["buf"].clone(), layers=[{**dw_copy(d), **pw_copy(p)} for p, d in b["layers"]],
                              transition=pw_copy(b["transition"]), down=None if b["down"] is None else dw_copy(b["down"]),
                              dropout=None if b.get("dropout") is None else dict(b["dropout"], key=b["dropout"]["key"].clone()))
                         for b in plan.block_records])
    if plan.stem_record is not None:
        sr = plan.stem_record
        pc0 = sr["pc0"]
        saved["stem"] = dict(dw_copy(sr["base2"]), x4=plan.input_nhwc.clone(), y0=sr["y0"].clone(), w0=pc0.w.clone(),
                             scale0=pc0.scale.clone(), bn0=sr["bn0"], bnt0=bnt_copy(sr.get("bnt0")), base1=pw_copy(sr["base1"]))
    return _BackboneGrads.apply(saved, *(p for _, p in named))


# -- packed weights after an optimizer step ---------------------------------------------------------
def rewrite_raw_conv(owner, old, new):
    """``new``'s images into ``old``'s storage (a ``PackedConv`` / ``_RawConv``).  The fp16x2 exponent is part of every launch
    descriptor that reads the image: it is kept while the new weights fit it (graphs stay valid); otherwise the descriptors of
    every plan follow and captured graphs of those plans are dropped (they hold the old exponent by value)."""
    old.w.copy_(new.w)
    old.scale.copy_(new.scale)
    old.shift.copy_(new.shift)
    if getattr(old, "w3", None) is not None:
        old.w3.copy_(hip_ops.pack_conv_weight_bf16x3(old.w))
    if getattr(old, "w2", None) is not None:
        img, e = old.w2
        top = float(old.w.abs().max()) * 2.0 ** e
        if not (2.0 ** 12 <= top < 2.0 ** 15):             # (packed for just below 2^14; fp16 ends at 65504)
            e = hip_ops.fp16x2_weight_scale_exp(old.w)
            for plan in owner._plans.values():
                for st in plan.conv_steps:
                    # (a batch-statistics plan holds the pack behind engine._IdentityEpilogue)
                    if getattr(st.pc, "pack", st.pc) is old and int(st.desc.precision) == _ffi.PREC_FP16X2:
                        st.desc.w_scale_exp = int(e)
                        plan.graph = None
            owner._bump_version()
        img.copy_(hip_ops.pack_conv_weight_fp16x2(old.w, e))
        old.w2 = (img, e)


def copy_pack(owner, old, new):
    """A depthwise / pair pack (a tuple of tensors, None and sizes) tensor-wise into ``old``'s storage."""
    for o, t in zip(old, new):
        if isinstance(o, torch.Tensor):
            o.copy_(t)


def refresh_packs(owner):
    """Rewrite in place the packed images of every unit (``owner._units()``), from the first unit of the widest training mode
    ever set on, whose parameters or BatchNorm buffers (the running statistics move under ``batch_stats``) changed (``_version``)
    since they were last known to match: plans and graphs keep their
    pointers; an autograd node of an earlier forward holds copies.  Nothing while no mode was ever set: today's contract for
    in-place edits (``invalidate_packed``)."""
    start = owner.__dict__.get("_watch_from")
    if start is None:
        return
    seen = owner.__dict__.setdefault("_pack_versions", {})
    stale = {}
    for u in owner._units():
        if u.index >= start:
            v = tuple(t._version for t in list(u.module.parameters()) + list(u.module.buffers()))
            if seen.get(u.name) != v:
                seen[u.name] = v
                stale[u.name] = u
    if stale:
        with torch.inference_mode():                          # (the packs may have been made under inference mode)
            for (name, device), old in list(owner._packed_cache.items()):
                if name in stale:
                    stale[name].write(owner, old, stale[name].make(device))
