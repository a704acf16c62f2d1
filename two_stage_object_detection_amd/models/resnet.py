"""ResNet backbones with the reference's module surface (models/resnet.py of the reference) and a
HIP execution path.

Same class names, constructor signatures, sub-module names and parameter shapes as the reference
(``conv1/bn1/relu/maxpool/layer{1..4}[/avgpool/fc]``, blocks ``conv{1,2,3}/bn{1,2,3}/relu/downsample``),
so its checkpoints load with ``strict=True`` and ``torch.manual_seed(s)`` reproduces the same
initial weights (sub-modules are created, and the Kaiming fan_out pass applied, in the same order:
reference models/resnet.py:94-109).

The nn.Conv2d / nn.BatchNorm2d / nn.PReLU children are parameter containers only.  ``forward``
compiles a launch plan of fused conv+BN+PReLU(+residual) implicit-GEMM kernels (engine.Plan) for the
input geometry and runs it on the GPU; there is no eager / CPU path.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import hip_ops
from .._ffi import ACT_NONE, ACT_PRELU, TsodError, lib, ptr, require_cuda, stem_out_hw
from ..engine import (FusedBottleneckWeights, FusedShortcutConv, FusedStemWeights, PackedConv, Plan, PlanOwner, _IdentityEpilogue,
                      prelu_slope)
from . import resnet_grads


def _bn_stats_step(plan: Plan, bn, name: str, z: torch.Tensor):
    """``plan.bn_stats`` of the raw conv output z [N,h,w,C] for the BatchNorm ``name``."""
    C = z.shape[3]
    out = plan.bn_stats(bn, z, C, name)
    if C != bn.num_features or C % 4:
        raise TsodError(f"batch_stats: {name} has {bn.num_features} channels, its conv output {C}; a multiple of 4 is needed")
    return out


def _bn_apply_prelu_step(plan: Plan, z, scale, shift, slope, dst, residual=None, second=None):
    """tsod_bn_apply_prelu_f32: dst = prelu(scale * z + shift + R, slope) with R nothing, ``residual`` or ``second`` = (z2, scale2,
    shift2), and dst's range words."""
    C = z.shape[3]
    z2, scale2, shift2 = second if second is not None else (None, None, None)
    plan.call(lib().tsod_bn_apply_prelu_f32, ptr(z), z.numel() // C, C, C, C, 0, ptr(scale), ptr(shift), ptr(residual),
              0 if residual is None else residual.shape[3], 0, ptr(z2), 0 if z2 is None else z2.shape[3], 0, ptr(scale2),
              ptr(shift2), float(slope), ptr(dst), dst.shape[3], 0, plan.amax_ptr(dst) or None, keep=(z, dst, residual, z2))


def _conv(cin, cout, k, stride=1, pad=0, groups=1):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, groups=groups, bias=False)


class _ResidualBlock(nn.Module):
    """Shared machinery of the two block types: a list of (conv, bn) stages, one shared PReLU."""
    expansion = 1
    _stage_names: tuple = ()

    def _emit(self, plan: Plan, x: torch.Tensor, name: str, record: bool = False) -> torch.Tensor:
        """``record`` (a trained block, ``resnet_grads.eligible`` / ``eligible_stage``): the same launches, but the stage
        outputs stay out of the buffer pool and go, with the packs, to ``plan.block_records`` for the autograd node."""
        dev = plan.device
        slope = prelu_slope(self.relu)
        identity = x
        # the whole block as ONE launch (tsod_bottleneck_fp16x2): 64 mid channels, stride 1 - layer1, the HBM-bound stage of the trunk
        # (the 64-channel intermediates stay in LDS): the identity blocks layer1.1 / layer1.2 and (round 5) the block in front of
        # them, whose shortcut is a 1x1 projection at stride 1 (layer1.0): conv3 + shortcut as one stacked-K GEMM inside the launch
        if getattr(plan, "fuse_bottleneck", False) and len(self._stage_names) == 3 and not record:
            ident = self.downsample is None and self.conv1.in_channels == self.conv3.out_channels
            proj = (getattr(plan, "fuse_projection", False) and self.downsample is not None and len(self.downsample) == 2 and isinstance(self.downsample[0], nn.Conv2d)
                    and self.downsample[0].kernel_size == (1, 1) and self.downsample[0].stride == (1, 1) and self.downsample[0].groups == 1)
            if ((ident or proj) and self.conv1.out_channels == 64 and self.conv2.groups == 1 and self.conv2.stride == (1, 1)
                    and self.conv1.in_channels % 64 == 0 and self.conv3.out_channels % 64 == 0):
                fb = plan.packed(f"{name}.fused", lambda: FusedBottleneckWeights(self, dev))
                out = plan.pool.alloc((x.shape[0], x.shape[1], x.shape[2], fb.cout))
                return plan.bottleneck(fb, x, out, name=f"{name}.fused")
        # projection shortcut + last 1x1 conv as ONE stacked-K GEMM (engine.FusedShortcutConv): one launch, no shortcut tensor
        # written and re-read as residual.  Needs a 1x1 last conv (Bottleneck) and channel counts the K-steps divide.
        last_name, last_bn = self._stage_names[-1]
        last_conv = getattr(self, last_name)
        fuse = (self.downsample is not None and getattr(plan, "fuse_shortcut", True) and last_conv.kernel_size == (1, 1)
                and last_conv.groups == 1 and last_conv.in_channels % 32 == 0 and self.downsample[0].in_channels % 32 == 0
                and self.downsample[0].kernel_size == (1, 1))
        if self.downsample is not None and not fuse:
            ds_conv, ds_bn = self.downsample[0], self.downsample[1]
            pc = plan.packed(f"{name}.downsample", lambda: PackedConv(ds_conv.weight, dev, bn=ds_bn, stride=ds_conv.stride[0],
                                                                      act=ACT_NONE))
            oh, ow = pc.out_hw(x.shape[1], x.shape[2])
            identity = plan.conv(pc, x, plan.pool.alloc((x.shape[0], oh, ow, pc.cout)), name=f"{name}.downsample")
        cur = x
        last = len(self._stage_names) - 1
        ys, pcs = [], []
        for i, (cname, bname) in enumerate(self._stage_names):
            conv, bn = getattr(self, cname), getattr(self, bname)
            if conv.groups != 1:                      # ResNeXt's grouped 3x3 (models/resnet.py:46-47): direct kernel, no MFMA
                cur = self._emit_grouped(plan, conv, bn, cur, x, slope, f"{name}.{cname}")
                continue
            if i == last and fuse:
                ds_conv, ds_bn = self.downsample[0], self.downsample[1]
                pc = plan.packed(f"{name}.{cname}+downsample", lambda conv=conv, bn=bn: FusedShortcutConv(
                    conv.weight, bn, ds_conv.weight, ds_bn, ds_conv.stride[0], dev, ACT_PRELU, slope))
                out = plan.pool.alloc((cur.shape[0], cur.shape[1], cur.shape[2], pc.cout))
                plan.conv(pc, cur, out, segs=[(0, pc.cin)], name=f"{name}.{cname}+downsample", x2=x, stride2=pc.stride2)
                ys.append(out)                        # (no pack joins pcs: a trained block's record makes plain ones)
                if cur is not x and not record:
                    plan.pool.release(cur)
                cur = out
                continue
            pc = plan.packed(f"{name}.{cname}", lambda conv=conv, bn=bn: PackedConv(
                conv.weight, dev, bn=bn, stride=conv.stride[0], pad=conv.padding[0], act=ACT_PRELU, slope=slope))
            oh, ow = pc.out_hw(cur.shape[1], cur.shape[2])
            out = plan.pool.alloc((cur.shape[0], oh, ow, pc.cout))
            plan.conv(pc, cur, out, residual=identity if i == last else None, name=f"{name}.{cname}")
            ys.append(out)
            pcs.append(pc)
            if cur is not x and not record:
                plan.pool.release(cur)
            cur = out
        if identity is not x:
            plan.pool.release(identity)
        if record:
            plan.block_records.append(resnet_grads.block_record(plan, self, name, x, ys, pcs))
        return cur

    def _emit_batch_stats(self, plan: Plan, x: torch.Tensor, name: str) -> torch.Tensor:
        """A trained Bottleneck of the batch-statistics plan: per BatchNorm the conv with an identity
        epilogue into a raw z outside the pool (one pack per conv, shared with the folded plans), tsod_bn_stats_f32 on the
        module's own tensors, tsod_bn_apply_prelu_f32; conv3's apply adds x or the shortcut's BatchNorm as its second operand,
        so a projection block runs conv3 and downsample.0 as two convs.  Everything goes to ``plan.block_records``."""
        dev = plan.device
        slope = prelu_slope(self.relu)
        N = x.shape[0]

        def raw_conv(key, conv, bn, act, src):
            pc = plan.packed(key, lambda: PackedConv(conv.weight, dev, bn=bn, stride=conv.stride[0], pad=conv.padding[0], act=act,
                                                     slope=slope if act == ACT_PRELU else 0.0))
            oh, ow = pc.out_hw(src.shape[1], src.shape[2])
            z = torch.empty((N, oh, ow, pc.cout), dtype=torch.float32, device=dev)
            plan.conv(_IdentityEpilogue(pc, dev), src, z, name=key)
            return pc, z

        cur, ys, pcs, bnts = x, [], [], []
        pcd = bnt_d = None
        for i, (cname, bname) in enumerate(self._stage_names):
            conv, bn = getattr(self, cname), getattr(self, bname)
            pc, z = raw_conv(f"{name}.{cname}", conv, bn, ACT_PRELU, cur)
            bnt, scale, shift = _bn_stats_step(plan, bn, f"{name}.{bname}", z)
            out = plan.pool.alloc(tuple(z.shape))
            if i < 2:
                _bn_apply_prelu_step(plan, z, scale, shift, slope, out)
            elif self.downsample is None:
                _bn_apply_prelu_step(plan, z, scale, shift, slope, out, residual=x)
            else:
                pcd, zd = raw_conv(f"{name}.downsample", self.downsample[0], self.downsample[1], ACT_NONE, x)
                bnt_d, scale_d, shift_d = _bn_stats_step(plan, self.downsample[1], f"{name}.downsample.1", zd)
                _bn_apply_prelu_step(plan, z, scale, shift, slope, out, second=(zd, scale_d, shift_d))
            ys.append(out)
            pcs.append(pc)
            bnts.append(bnt)
            cur = out
        plan.block_records.append(resnet_grads.block_record(plan, self, name, x, ys, pcs, bnts, pcd, bnt_d))
        return cur

    def _emit_grouped(self, plan: Plan, conv, bn, cur, x, slope, name):
        from ..engine import fold_bn
        C, groups, stride = conv.out_channels, conv.groups, conv.stride[0]
        if conv.kernel_size != (3, 3) or conv.in_channels != C or (C // groups) % 4:
            raise TsodError(f"{name}: only 3x3 grouped convs with as many output as input channels and a multiple of 4 "
                            "channels per group have a HIP kernel (what resnext50_32x4d uses)")

        def make():
            w = conv.weight.detach().float().permute(0, 2, 3, 1).contiguous().to(plan.device)     # [C][3][3][C/groups]
            sc, sh = fold_bn(bn)
            return w, sc.to(plan.device), sh.to(plan.device)
        w, sc, sh = plan.packed(name, make)
        N, H, W, _ = cur.shape
        out = plan.pool.alloc((N, (H - 1) // stride + 1, (W - 1) // stride + 1, C))
        plan.call(lib().tsod_gconv3x3_amax_f32, ptr(cur), N, H, W, C, cur.shape[3], groups, ptr(w), ptr(sc), ptr(sh), stride,
                  ACT_PRELU, float(slope), ptr(out), C, plan.amax_ptr(out) or None, keep=(cur, out, w, sc, sh))
        if cur is not x:
            plan.pool.release(cur)
        return out


class BasicBlock(_ResidualBlock):
    expansion = 1
    _stage_names = (("conv1", "bn1"), ("conv2", "bn2"))

    def __init__(self, in_channel, out_channel, stride=1, downsample=None, **kwargs):
        super().__init__()
        self.conv1 = _conv(in_channel, out_channel, 3, stride, 1)
        self.bn1 = nn.BatchNorm2d(out_channel)
        self.relu = nn.PReLU()
        self.conv2 = _conv(out_channel, out_channel, 3, 1, 1)
        self.bn2 = nn.BatchNorm2d(out_channel)
        self.downsample = downsample


class Bottleneck(_ResidualBlock):
    expansion = 4
    _stage_names = (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"))

    def __init__(self, in_channel, out_channel, stride=1, downsample=None, groups=1, width_per_group=64):
        super().__init__()
        width = int(out_channel * (width_per_group / 64.)) * groups
        self.conv1 = _conv(in_channel, width, 1)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = _conv(width, width, 3, stride, 1, groups)      # stride on the 3x3 (v1.5)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = _conv(width, out_channel * self.expansion, 1)
        self.bn3 = nn.BatchNorm2d(out_channel * self.expansion)
        self.relu = nn.PReLU()
        self.downsample = downsample


_STAGES = ("layer4", "layer3", "layer2")       # what ``train_from`` may be given, narrowest section first
_STEM = "stem"                                 # ... and the widest: conv1 / bn1 / relu and every block


class ResNet(PlanOwner, nn.Module):
    _train_mode = None           # set_train_mode(): a plain instance attribute once set - pickled and deep-copied, never in
                                 # the state_dict
    _batch_stats = False         # set_train_mode(batch_stats=): likewise
    _grads = resnet_grads        # (PlanOwner._forward_train: its refresh_packs and feature_map_with_grads)

    def __init__(self, block, blocks_num, num_classes=25, include_top=True, groups=1, width_per_group=64):
        super().__init__()
        self.include_top = include_top
        self.in_channel = 64
        self.groups = groups
        self.width_per_group = width_per_group
        self.conv1 = _conv(3, 64, 7, 2, 3)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.PReLU()
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        for i, (ch, n, stride) in enumerate(zip((64, 128, 256, 512), blocks_num, (1, 2, 2, 2)), start=1):
            setattr(self, f"layer{i}", self._make_layer(block, ch, n, stride))
        if include_top:
            self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
            self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self._init_plan_owner()
        self.out_channels = 512 * block.expansion

    def _make_layer(self, block, channel, block_num, stride=1):
        out_ch = channel * block.expansion
        downsample = None
        if stride != 1 or self.in_channel != out_ch:
            downsample = nn.Sequential(_conv(self.in_channel, out_ch, 1, stride), nn.BatchNorm2d(out_ch))
        blocks = [block(self.in_channel, channel, downsample=downsample, stride=stride, groups=self.groups,
                        width_per_group=self.width_per_group)]
        self.in_channel = out_ch
        blocks += [block(out_ch, channel, groups=self.groups, width_per_group=self.width_per_group)
                   for _ in range(1, block_num)]
        return nn.Sequential(*blocks)

    # -- training mode -------------------------------------------------
    @property
    def n_blocks(self) -> int:
        """The largest ``n`` of ``train_blocks(n)``: the length of the run of eligible blocks at the end of ``layer4`` (identity
        Bottlenecks with a dense 3x3 at stride 1: 2 for resnet50 / resnet101, 0 for resnet34 and resnext50_32x4d)."""
        n = 0
        for blk in reversed(list(self.layer4)):
            if not resnet_grads.eligible(blk):
                break
            n += 1
        return n

    @property
    def trainable_stages(self) -> tuple:
        """The stage names ``train_from`` accepts, widest last: a stage is offered when every block from its first to the end of
        ``layer4`` is ``resnet_grads.eligible_stage`` (resnet50 / resnet101: ("layer4", "layer3", "layer2"); resnet34 and
        resnext50_32x4d: ()).  ``layer1`` is never offered: its blocks run as one launch each and keep no stage outputs."""
        stages = []
        for stage in _STAGES:
            if not all(resnet_grads.eligible_stage(blk) for blk in getattr(self, stage)):
                break
            stages.append(stage)
        return tuple(stages)

    @property
    def trainable_sections(self) -> tuple:
        """Everything ``train_from`` accepts, widest last: ``trainable_stages``, then "stem" (the whole backbone: ``conv1``,
        ``bn1``, ``relu`` and every block of ``layer1`` ... ``layer4``) where all three stages are offered, every block of
        ``layer1`` is ``resnet_grads.eligible_stage``, ``conv1`` is Conv2d(3, 64, 7, 2, 3, bias=False) and ``maxpool`` is
        MaxPool2d(3, 2, 1) (resnet50 / resnet101; resnet34 and resnext50_32x4d: ())."""
        stages = self.trainable_stages
        c, mp = self.conv1, self.maxpool
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        stem_ok = (isinstance(c, nn.Conv2d) and (c.in_channels, c.out_channels) == (3, 64) and c.kernel_size == (7, 7)
                   and c.stride == (2, 2) and c.padding == (3, 3) and c.dilation == (1, 1) and c.groups == 1 and c.bias is None
                   and isinstance(mp, nn.MaxPool2d) and pair(mp.kernel_size) == (3, 3) and pair(mp.stride) == (2, 2)
                   and pair(mp.padding) == (1, 1) and pair(mp.dilation) == (1, 1) and not mp.ceil_mode)
        if stages == _STAGES and stem_ok and all(resnet_grads.eligible_stage(blk) for blk in self.layer1):
            return stages + (_STEM,)
        return stages

    @property
    def train_mode(self):
        """None | n (int >= 1) | a name of ``trainable_sections``: what ``set_train_mode`` was given last."""
        return self._train_mode

    def set_train_mode(self, mode, batch_stats=False):
        """How much of the backbone is differentiable: None (nothing, the default) or ``n`` in 1..``n_blocks`` (the last ``n``
        blocks of ``layer4``, ten tensors each: ``conv{1,2,3}.weight``, ``bn{1,2,3}.weight`` / ``.bias``, ``relu.weight``;
        ValueError outside that range).  Returns self.

        The contract is ``HarDNetFeatureExtraction.set_train_mode``'s: eval() only; BatchNorm stays folded - its ``weight`` /
        ``bias`` get gradients through the folded scale / shift, its running statistics are constants.  While a mode is on, grad
        mode enabled and a parameter of the section requires grad, the map that ``forward`` / ``forward_nhwc`` return carries ONE
        autograd node (``resnet_grads._ResNetGrads``; HIP kernels of csrc/conv_grads.hip and pw_grads.hip, the 3x3's dx through
        the forward conv library) that gives the gradients of ``trainable_parameters()`` and nothing for the image.  The forward
        runs the same launches on a plan of its own (another plan-cache key) and returns the same bits; that plan keeps, per
        trained block, the block input and the three stage outputs out of its buffer pool, and the node copies them.  The
        PReLU slope of every trained block must be finite and > 0 (TsodError otherwise): the masks are taken from the saved
        outputs.  With no mode ever set nothing of the inference path changes.

        In-place updates of the parameters (an optimizer step) are noticed through their ``_version`` before the next forward of
        ANY kind for the blocks of the widest mode ever set: a changed block's packs are dropped and packed again, every plan
        of the module is dropped and ``weights_version`` moves (``refresh_packs()``).  The comparison runs in a forward of this
        module, not in ``optimizer.step()``: a graph captured around the module (``FasterRCNN.make_graphed``) that is replayed
        right after a step, with no eager forward in between, still passes its ``weights_version`` check and runs the old
        weights - call ``refresh_packs()`` after ``step()`` where graphs are replayed.

        ``f.grad_fn.saved`` is the dict the backward reads: ``names`` (the parameter names in ``trainable_parameters()`` order),
        ``nchw``, and ``blocks``: per trained block in forward order ``name``, ``x``, ``y1``, ``y2``, ``y3`` (NHWC copies), ``w`` / ``scale``
        (the three f32 packs [Cout,KH,KW,Cin] and folded scales), ``rot`` (the 3x3 dgrad's image [C,3,3,Cout]), ``slope``, ``bn``
        (per stage: running mean, 1 / sqrt(var + eps)).  One record (``resnet_grads.block_record``), one copy (``block_copy``) and
        one backward walk serve this layout and ``batch_stats``' below; the variant alone decides which keys an entry carries.

        ``mode`` a stage name of ``trainable_stages`` ("layer4", "layer3", "layer2"; ValueError for
        anything else): every block from the first block of that stage to the end of ``layer4`` under the same contract, on the
        plan key ("train_from", stage).  An identity block has the ten tensors above, a projection block thirteen: the ten, then
        ``downsample.0.weight``, ``downsample.1.weight``, ``downsample.1.bias``.  Its entry of ``blocks`` also carries ``wd`` /
        ``scaled`` (the shortcut's f32 pack and folded scale; ``w[2]`` / ``scale[2]`` are conv3's, made for the backward: the forward
        runs both as one folded GEMM), ``stride``, ``s2d`` (conv2's 2x2 phase pack [4 C,2,2,Cout] where the stride is 2, and ``rot``
        is None then) and ``bn_d``.

        ``mode`` "stem" (where ``trainable_sections`` offers it; ``train_full()``): the whole backbone,
        on the plan key ("train_from", "stem").  ``trainable_parameters()`` is then every parameter of an ``include_top=False``
        module in module order: ``conv1.weight``, ``bn1.weight``, ``bn1.bias``, ``relu.weight``, then the blocks of ``layer1`` ...
        ``layer4`` as above.  The contract is the same but for the launches: this plan always runs the stem and ``layer1`` as
        per-layer launches (conv1 as a ``PackedConv``, tsod_maxpool3x3s2_f32, three convs per block), whatever ``fuse_stem``,
        ``fuse_bottleneck`` and ``fuse_projection`` say - the one-launch kernels keep nothing for a backward - so its map has the
        bits of the inference forward with those three switches off (the default); inference keeps its one-launch kernels.
        The stem's slope must be finite and > 0 too.  ``saved`` gains ``stem``: ``x4`` (the staged image [N,H,W,4]), ``y``
        (conv1's output after BN and PReLU), ``w`` / ``scale`` (conv1's f32 pack [64,7,8,4] and folded scale), ``slope``, ``bn``;
        the pooled map is ``blocks[0]["x"]``.  With the four stem tensors frozen (``requires_grad_(False)``) no stem launch runs
        in the backward and ``layer1.0`` is the earliest block: "from layer1 on".

        ``batch_stats=True`` (every mode) adds the reference's contract, ``.train()``: under ``.eval()``
        nothing changes (same plan-cache key, same bits); under ``.train()`` with grad mode on the forward takes a plan of its
        own variant (the key gains "batch_stats") in which every BatchNorm from the mode's first module on normalises with the
        statistics of the current batch (over N, H, W), backpropagates through them and updates its ``running_mean``,
        ``running_var`` (momentum, unbiased variance) and ``num_batches_tracked`` in the module's own storage - current when
        ``forward`` returns; the blocks below stay folded on their running statistics (frozen BN) and their buffers do not change
        by a bit.  Per such BatchNorm the conv runs with an identity epilogue into a raw buffer z, then tsod_bn_stats_f32 and
        tsod_bn_apply_prelu_f32 (conv3's adds the block input, or ``downsample.1`` on its own z as a second operand: a projection
        block then runs conv3 and ``downsample.0`` as two convs); the stem is conv1, statistics, apply, tsod_maxpool3x3s2_f32.
        The backward runs tsod_bn_prelu_train_grad_f32 on (y, d, z) per stage - behind a stride-2 3x3 and behind the stem the
        gathering mask kernels followed by tsod_bn_train_grad_f32, which also serves ``downsample.1`` - and feeds dz to the
        conv backward with unit scale; ``bn*.weight`` / ``.bias`` gradients are dgamma / dbeta.  ``saved`` then carries
        ``batch_stats`` = True and, per block, ``bnt`` (per stage: ``z``, ``mean``, ``invstd``, ``gamma``, ``C`` - the node's own
        copies) in place of ``bn``, ``scale`` as ones, ``rot`` / ``s2d`` made from the unscaled weight, and for a projection block
        ``bnt_d`` in place of ``bn_d``; ``stem`` carries ``bnt`` likewise.  The slopes must still be finite and > 0.  Under
        ``.train()`` with grad mode off, without ``batch_stats`` or with nothing of the section requiring grad, the forward raises
        ``call .eval() first`` as before.  A BatchNorm of the section with ``momentum=None``, ``track_running_stats=False`` or
        ``affine=False``: NotImplementedError here; BatchNorm tensors off the forward's device: TsodError, and fewer than two
        pixels per channel in any BatchNorm of the section: ValueError, both in the forward.  Memory on top of the mode's: the raw
        z of every BatchNorm of the section, twice (plan and node)."""
        if isinstance(mode, str):
            if mode == "layer1":
                raise ValueError("train_from: layer1 cannot be trained: each of its blocks runs as one launch and keeps no stage "
                                 f"outputs for a backward; trainable_stages = {self.trainable_stages}.  Where trainable_sections "
                                 'offers "stem", train_from("stem") with conv1 / bn1 / relu frozen by requires_grad_(False) '
                                 "trains from layer1 on: that plan runs layer1 as per-layer launches")
            if mode not in self.trainable_sections:
                raise ValueError(f"train_from: stage must be one of trainable_stages = {self.trainable_stages} (trainable_sections "
                                 f"= {self.trainable_sections}), got {mode!r}")
        elif mode is not None:
            mode = int(mode)
            if mode < 1 or mode > self.n_blocks:
                raise ValueError(f"train_blocks: n must be 1..n_blocks = {self.n_blocks} (the identity Bottlenecks at the end of "
                                 f"layer4 of this backbone), got {mode}")
        batch_stats = bool(batch_stats) and mode is not None
        if batch_stats:
            for name, bn in self._section_norms(mode):
                if bn.momentum is None or not bn.track_running_stats or not bn.affine:
                    raise NotImplementedError(f"batch_stats: {name} has momentum=None, track_running_stats=False or affine=False; "
                                              "only the reference's BatchNorm2d (momentum, running statistics, affine) is built")
        self._batch_stats = batch_stats
        if mode is not None:
            watched = self.__dict__.setdefault("_watched", {})
            for name, blk in self._stem_modules(mode) + self._section(mode):     # the widest mode ever set: what the refresh watches
                watched.setdefault(name, resnet_grads.versions_of(blk))
        self._train_mode = mode
        return self

    def refresh_packs(self):
        """Notice in-place changes of the watched blocks now (``resnet_grads.refresh_packs``: packs and plans dropped,
        ``weights_version`` moved) instead of at the next forward: the call a training loop makes after ``optimizer.step()``
        when it replays captured graphs of this module, which go stale through ``weights_version`` only.  Returns self."""
        resnet_grads.refresh_packs(self)
        return self

    def train_blocks(self, n: int, batch_stats=False):
        """``set_train_mode(n)``.  Memory: per trained block N x h x w x 10 width floats (x, y1, y2, y3), twice (plan and node),
        and one rotated 3x3 image per trained block and device."""
        return self.set_train_mode(int(n), batch_stats)

    def train_from(self, stage: str, batch_stats=False):
        """``set_train_mode(stage)``: every block from the first of ``stage`` (one of ``trainable_stages``) to the end of
        ``layer4``.  Memory: what ``train_blocks`` keeps, per trained block, and per trained stride-2 3x3 and device the 2x2 phase
        pack, 16 / 9 of the weight, in place of the rotated image."""
        return self.set_train_mode(str(stage), batch_stats)

    def train_full(self, batch_stats=False):
        """``set_train_mode("stem")``: every parameter of the backbone (named after HarDNet's).  Memory: what ``train_from``
        keeps for every block, and the stem's output N x OH x OW x 64 floats and the staged image N x H x W x 4, each twice."""
        return self.set_train_mode(_STEM, batch_stats)

    def _stem_modules(self, mode):
        return [(k, getattr(self, k)) for k in resnet_grads.STEM_MODULES] if mode == _STEM else []

    def _section(self, n):
        if n == _STEM:
            return [(f"layer{li}.{i}", blk) for li in range(1, 5) for i, blk in enumerate(getattr(self, f"layer{li}"))]
        if isinstance(n, str):
            return [(f"{stage}.{i}", blk) for stage in reversed(_STAGES[:_STAGES.index(n) + 1])
                    for i, blk in enumerate(getattr(self, stage))]
        blocks = list(self.layer4)
        return [(f"layer4.{i}", blocks[i]) for i in range(len(blocks) - n, len(blocks))]

    def _section_norms(self, mode):
        """(name, BatchNorm2d) of every BatchNorm of the mode's section, in module order."""
        norms = [("bn1", self.bn1)] if mode == _STEM else []
        for name, blk in self._section(mode):
            norms += [(f"{name}.{b}", getattr(blk, b)) for _, b in blk._stage_names]
            if blk.downsample is not None:
                norms.append((f"{name}.downsample.1", blk.downsample[1]))
        return norms

    def _trainable_named(self):
        mode = self._train_mode or 0
        return [(f"{name}.{k}", p) for name, blk in self._stem_modules(mode) + self._section(mode) for k, p in blk.named_parameters()]

    def trainable_parameters(self):
        """The parameters the feature map's autograd node reaches, in module order; empty with no mode on."""
        return [p for _, p in self._trainable_named()]

    def _active_mode(self):
        if self._train_mode is None or self.include_top or not torch.is_grad_enabled():      # (include_top: forward raises)
            return None
        return self._train_mode if any(p.requires_grad for p in self.trainable_parameters()) else None

    def _trains_in_plan(self) -> bool:
        """The batch-statistics variant is on: ``batch_stats`` set, ``.train()``, grad mode on, a parameter requiring grad."""
        return self._batch_stats and self.training and self._active_mode() is not None

    def _plan_variant(self):
        mode = self._active_mode()
        if mode is None:
            return ()
        key = ("train_from" if isinstance(mode, str) else "train_blocks", mode)
        return key + ("batch_stats",) if self._trains_in_plan() else key

    def _mode_norms(self):
        return self._section_norms(self._train_mode)

    def forward_nhwc(self, x, slot: int = 0):
        if self._active_mode() is not None:
            return self._forward_train(x, slot, nchw=False)
        resnet_grads.refresh_packs(self)
        return super().forward_nhwc(x, slot)

    # -- plan (cache, invalidation, lookup: engine.PlanOwner) -----------------------------------
    def build_plan(self, N, H, W, device, slot=0) -> Plan:
        """Launch plan for a [N,3,H,W] input: NCHW->NHWC4, 7x7 stem as a 7x8x4 implicit GEMM with
        BN+PReLU, 3x3/s2 max pool, then the residual stages."""
        plan = self._new_plan(device, slot)
        plan.fuse_shortcut = bool(self.fuse_shortcut)
        plan.fuse_bottleneck = bool(self.fuse_bottleneck)
        plan.fuse_projection = bool(self.fuse_projection)
        x4 = plan.pool.alloc((N, H, W, 4))
        plan.input_nhwc = x4
        oh, ow, ph, pw = stem_out_hw(H, W)
        mode = self._active_mode()
        plan.stem_record = None
        # the batch-statistics variant (section 4.24): the statistics launches share one workspace
        batch_stats = plan.batch_stats = self._trains_in_plan()
        if mode != _STEM and self.fuse_stem and tuple(self.conv1.weight.shape) == (64, 3, 7, 7):
            # conv1 + bn1 + PReLU + max pool as ONE launch that reads the images where stage_input finds them (NCHW or NHWC4):
            # no layout pass, the 64-channel conv output never leaves the CU (tsod_stem_fp16x2)
            fs = plan.packed("conv1.fused", lambda: FusedStemWeights(self.conv1, self.bn1, self.relu, device))
            cur = plan.stem(fs, N, H, W, plan.pool.alloc((N, ph, pw, 64)), name="conv1+maxpool")
        else:
            stem = plan.packed("conv1", lambda: PackedConv(self.conv1.weight, device, bn=self.bn1, stride=2, pad=3, act=ACT_PRELU,
                                                           slope=prelu_slope(self.relu), cin_pad=4, kw_pad=8))
            assert (oh, ow) == tuple(stem.out_hw(H, W))
            bnt0 = None
            if batch_stats and mode == _STEM:    # conv1 -> z, statistics, apply; the pool below is the folded plan's
                z0 = torch.empty((N, oh, ow, 64), dtype=torch.float32, device=device)
                plan.conv(_IdentityEpilogue(stem, device), x4, z0, name="conv1")
                bnt0, scale0, shift0 = _bn_stats_step(plan, self.bn1, "bn1", z0)
                s_out = plan.pool.alloc((N, oh, ow, 64))
                _bn_apply_prelu_step(plan, z0, scale0, shift0, stem.slope, s_out)
            else:
                s_out = plan.conv(stem, x4, plan.pool.alloc((N, oh, ow, 64)), name="conv1")
            cur = plan.pool.alloc((N, ph, pw, 64))
            plan.call(lib().tsod_maxpool3x3s2_f32, ptr(s_out), N, oh, ow, 64, 64, ptr(cur), 64, keep=(s_out, cur))
            plan.alias_amax(cur, s_out)          # range words: max |pooled| <= max |stem output|
            if mode == _STEM:                    # the trained stem: the image and conv1's output stay out of the pool (x4 is never
                plan.stem_record = resnet_grads.stem_record(plan, self, x4, s_out, stem, bnt0)    # released), the node copies them
            else:
                plan.pool.release(s_out)
        # a training mode (with grad mode on): the section's blocks (the last ``mode`` of layer4, or a stage onward) run the same
        # launches, but what the autograd
        # node needs of them stays out of the pool (the node copies it after the run) and is recorded for it
        trained = {name for name, _ in self._section(mode)} if mode else set()
        plan.block_records = []
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(self, f"layer{li}")):
                record = f"layer{li}.{bi}" in trained
                name = f"layer{li}.{bi}"
                nxt = blk._emit_batch_stats(plan, cur, name) if record and batch_stats else blk._emit(plan, cur, name, record)
                if not record:
                    plan.pool.release(cur)
                cur = nxt
        plan.output_nhwc = cur
        plan.output_amax = plan.amax_ptr(cur)
        return plan.finalize()

    def forward(self, x):
        if self._active_mode() is not None:
            return self._forward_train(x, 0, nchw=True)
        feat = self.forward_nhwc(x)
        if self.include_top:
            raise TsodError("include_top=True (avgpool + fc classifier) is outside the detector forward path; "
                            "build with include_top=False")
        return hip_ops.nhwc_to_nchw(feat)


def resnet34(num_classes=25, include_top=True):
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes=num_classes, include_top=include_top)


def resnet50(num_classes=25, include_top=True):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes=num_classes, include_top=include_top)


def resnet101(num_classes=25, include_top=True):
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes=num_classes, include_top=include_top)


def resnext50_32x4d(num_classes=25, include_top=True):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes=num_classes, include_top=include_top, groups=32,
                  width_per_group=4)
