"""HarDNet backbones with the reference's module surface (models/hardnet.py of the reference) and a
HIP execution path (depth_wise=True variants: the only usable ones).

Same class names, sub-module names (``base.N.conv/norm/relu``, ``base.N.dwconv/norm``,
``base.N.layers.L.layer1/layer2``) and parameter shapes as the reference, created in the same order,
so checkpoints load with ``strict=True`` and a seed reproduces the same initial weights.

Execution (engine.Plan), all NHWC f32:
  * every HarDBlock owns ONE wide pixel-major buffer: slice 0 is the block input, slice i the output
    of layer i (each slice padded to a multiple of 4 channels, pad channels hold exact zeros).
    A layer's input "torch.cat(linked layers)" (reference :99-110) is never built: the 1x1 implicit
    GEMM gathers its K dimension from the linked slices (channel segments of the conv descriptor),
    and the producer of every tensor writes straight into its slice, so both concats of the
    reference (:108, :120) are free.
  * 1x1 conv + BN + ReLU6 -> f32 MFMA GEMM with fused epilogue; depthwise 3x3 + BN -> streaming
    stencil kernel writing into the block buffer; tail = 2 depthwise s2 + grouped-pair 1x1.
"""
from __future__ import annotations

from collections import namedtuple
from functools import partial

import torch
import torch.nn as nn

from .. import hip_ops
from .._ffi import ACT_NONE, ACT_RELU6, TsodError, lib, ptr, require_cuda
from ..engine import PackedConv, Plan, PlanOwner, _IdentityEpilogue, bn_fold_stats, fold_bn
from . import hardnet_grads
from .hardnet_grads import copy_pack, refresh_packs, rewrite_raw_conv


def _pad4(c: int) -> int:
    return (c + 3) // 4 * 4


class Flatten(nn.Module):
    def forward(self, x):
        return x.view(x.size(0), -1)


class ConvLayer(nn.Sequential):
    """conv(k, stride, pad k//2, no bias) + BN + ReLU6 (reference :38-55; ``dropout`` is unused there too)."""

    def __init__(self, in_channels, out_channels, kernel=3, stride=1, dropout=0.1, bias=False):
        super().__init__()
        self.add_module("conv", nn.Conv2d(in_channels, out_channels, kernel_size=kernel, stride=stride,
                                          padding=kernel // 2, groups=1, bias=bias))
        self.add_module("norm", nn.BatchNorm2d(out_channels))
        self.add_module("relu", nn.ReLU6(True))


class DWConvLayer(nn.Sequential):
    """depthwise 3x3 (pad 1) + BN, no activation (reference :21-36)."""

    def __init__(self, in_channels, stride=1, bias=False):
        super().__init__()
        self.add_module("dwconv", nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=stride, padding=1,
                                            groups=in_channels, bias=bias))
        self.add_module("norm", nn.BatchNorm2d(in_channels))


class CombConvLayer(nn.Sequential):
    def __init__(self, in_channels, out_channels, kernel=1, stride=1):
        super().__init__()
        self.add_module("layer1", ConvLayer(in_channels, out_channels, kernel))
        self.add_module("layer2", DWConvLayer(out_channels, stride=stride))


def hard_block_links(layer: int):
    """Inputs of HarDBlock layer ``layer`` >= 1: layer - 2^i for every i with layer % 2^i == 0 (newest first)."""
    return [layer - (1 << i) for i in range(10) if (1 << i) <= layer and layer % (1 << i) == 0]


class HarDBlock(nn.Module):
    def get_link(self, layer, base_ch, growth_rate, grmul):
        if layer == 0:
            return base_ch, 0, []
        link = hard_block_links(layer)
        out_channels = growth_rate
        for _ in range(len(link) - 1):
            out_channels *= grmul
        out_channels = int(int(out_channels + 1) / 2) * 2
        in_channels = sum(self.get_link(k, base_ch, growth_rate, grmul)[0] for k in link)
        return out_channels, in_channels, link

    def get_out_ch(self):
        return self.out_channels

    def __init__(self, in_channels, growth_rate, grmul, n_layers, keepBase=False, dwconv=False):
        super().__init__()
        self.keepBase = keepBase
        self.in_channels = in_channels
        self.links, self.layer_out = [], []
        self.out_channels = 0
        layers_ = []
        for i in range(n_layers):
            outch, inch, link = self.get_link(i + 1, in_channels, growth_rate, grmul)
            self.links.append(link)
            self.layer_out.append(outch)
            layers_.append(CombConvLayer(inch, outch) if dwconv else ConvLayer(inch, outch))
            if (i % 2 == 0) or (i == n_layers - 1):
                self.out_channels += outch
        self.layers = nn.ModuleList(layers_)
        self.dwconv = dwconv

    # slices of the block buffer: index 0 = block input, i = output of layer i
    def slice_table(self):
        real = [self.in_channels] + list(self.layer_out)
        offs, o = [], 0
        for c in real:
            offs.append(o)
            o += _pad4(c)
        return real, offs, o

    def output_slices(self):
        t = len(self.layers) + 1
        return [i for i in range(t) if (i == 0 and self.keepBase) or i == t - 1 or i % 2 == 1]


_ARCH = {
    68: dict(first_ch=(32, 64), grmul=1.7, gr=(14, 16, 20, 40, 160), n_layers=(8, 16, 16, 16, 4),
             ch_list=(128, 256, 320, 640, 1024), downSamp=(1, 0, 1, 1, 0)),
    85: dict(first_ch=(48, 96), grmul=1.7, gr=(24, 24, 28, 36, 48, 256), n_layers=(8, 16, 16, 16, 16, 4),
             ch_list=(192, 256, 320, 480, 720, 1024), downSamp=(1, 0, 1, 0, 1, 0)),
    39: dict(first_ch=(24, 48), grmul=1.6, gr=(16, 20, 64, 160), n_layers=(4, 16, 8, 4),
             ch_list=(96, 320, 640, 1024), downSamp=(1, 1, 1, 0)),
}


def _gathered_weight(w: torch.Tensor, src_real, cout_pad):
    """[Cout, sum(src_real), 1, 1] -> [cout_pad, 1, 1, sum(pad4(src_real))]: zero columns at the pad
    channels of every gathered slice, zero rows for the padded output channels."""
    cout = w.shape[0]
    w2 = w.detach().float().cpu().view(cout, -1)
    cols, o = [], 0
    for c in src_real:
        blk = torch.zeros(cout_pad, _pad4(c))
        blk[:cout, :c] = w2[:, o:o + c]
        cols.append(blk)
        o += c
    return torch.cat(cols, dim=1).view(cout_pad, 1, 1, -1).contiguous()


def _padded(v: torch.Tensor, n: int, fill=0.0):
    out = torch.full((n,), fill, dtype=torch.float32)
    out[:v.numel()] = v.float().cpu()
    return out


class _RawConv:
    """PackedConv-compatible holder for a pre-gathered 1x1 weight."""

    def __init__(self, w_packed, scale, shift, device, act, cin_real=None, cout_real=None):
        self.w = w_packed.to(device)
        self.cout, self.kh, self.kw, self.cin = self.w.shape
        self.kw_logical, self.cin_src = self.kw, (self.cin if cin_real is None else cin_real)   # for FLOP accounting
        self.cout_real = self.cout if cout_real is None else cout_real
        self.stride, self.pad, self.act, self.slope = 1, 0, act, 0.0
        self.scale = None if scale is None else scale.to(device)
        self.shift = None if shift is None else shift.to(device)

    def out_hw(self, H, W):
        return H, W


def _pw_pack(layer, src_real, device):
    """The packed form of a 1x1 ConvLayer that gathers slices of ``src_real`` channels (a HarDBlock layer's ``layer1`` or a
    transition layer): the weight gathered to the padded slices it reads, BN folded, padded to 4 output channels."""
    cout = layer.conv.weight.shape[0]
    cp = _pad4(cout)
    sc, sh = fold_bn(layer.norm)
    return _RawConv(_gathered_weight(layer.conv.weight, src_real, cp), _padded(sc, cp), _padded(sh, cp), device, ACT_RELU6,
                    cin_real=sum(src_real), cout_real=cout)


def _stem_pack(layer, device, **geometry):
    """The packed form of ``base.0`` (3x3 stride 2, the image padded to 4 channels) or ``base.1`` (1x1)."""
    return PackedConv(layer.conv.weight, device, bn=layer.norm, act=ACT_RELU6, **geometry)


def _dw_params(conv: nn.Conv2d, bn, device):
    """depthwise weights as [3][3][C_pad] + per-channel scale/shift (folded BN, or the conv bias)."""
    C = conv.weight.shape[0]
    cp = _pad4(C)
    w = torch.zeros(3, 3, cp)
    w[:, :, :C] = conv.weight.detach().float().cpu().view(C, 9).t().reshape(3, 3, C)
    if bn is not None:
        scale, shift = fold_bn(bn)
        scale, shift = _padded(scale, cp, 0.0), _padded(shift, cp, 0.0)
    else:
        scale = None
        shift = _padded(conv.bias.detach(), cp) if conv.bias is not None else None
    return (w.to(device), None if scale is None else scale.to(device), None if shift is None else shift.to(device), cp)


def _pair_params(m: nn.Conv2d, device):
    G = m.out_channels
    return (m.weight.detach().float().view(G, 2).contiguous().to(device),
            None if m.bias is None else m.bias.detach().float().to(device))


# One packed unit of the backbone: ``name`` is its key in ``_packed_cache`` (and its module's path, so ``name + "." + k`` names
# its parameters), ``index`` its place in ``base``, ``module`` what it is made from, ``make(device)`` its pack and
# ``write(owner, old, new)`` how a new pack goes into an old one's storage.
Unit = namedtuple("Unit", "name index module make write")


class HarDNetFeatureExtraction(PlanOwner, nn.Module):
    _train_mode = None           # set_train_mode(): a plain instance attribute once set - pickled and deep-copied, never in
                                 # the state_dict
    _batch_stats = False         # set_train_mode(batch_stats=): likewise
    _dropout = False             # set_train_mode(dropout=): likewise
    dropout_generator = None     # a CPU torch.Generator the dropout keys are drawn from (None: torch.default_generator)
    last_dropout_key = None      # (key_lo, key_hi) of the last forward that ran with active dropout
    _grads = hardnet_grads       # (PlanOwner._forward_train: its refresh_packs and feature_map_with_grads)

    def __init__(self, depth_wise=True, arch=39):
        super().__init__()
        cfg = _ARCH[arch if arch in (39, 85) else 68]          # any other value = HarDNet-68, like the reference
        self.arch, self.depth_wise = arch, depth_wise
        first_ch, ch_list, gr = cfg["first_ch"], cfg["ch_list"], cfg["gr"]
        n_layers, down, grmul = cfg["n_layers"], cfg["downSamp"], cfg["grmul"]
        second_kernel, max_pool = (1, False) if depth_wise else (3, True)
        self.base = nn.ModuleList([])
        self.base.append(ConvLayer(in_channels=3, out_channels=first_ch[0], kernel=3, stride=2, bias=False))
        self.base.append(ConvLayer(first_ch[0], first_ch[1], kernel=second_kernel))
        self.base.append(nn.MaxPool2d(kernel_size=3, stride=2, padding=1) if max_pool
                         else DWConvLayer(first_ch[1], stride=2))
        ch = first_ch[1]
        blks = len(n_layers)
        for i in range(blks):
            blk = HarDBlock(ch, gr[i], grmul, n_layers[i], dwconv=depth_wise)
            ch = blk.get_out_ch()
            self.base.append(blk)
            if i == blks - 1 and arch == 85:
                self.base.append(nn.Dropout(0.1))
            self.base.append(ConvLayer(ch, ch_list[i], kernel=1))
            ch = ch_list[i]
            if down[i] == 1:
                self.base.append(nn.MaxPool2d(kernel_size=2, stride=2) if max_pool else DWConvLayer(ch, stride=1))
        self.base.append(nn.Conv2d(ch_list[-1], ch_list[-1], 3, 2, 1, groups=ch_list[-1]))
        self.base.append(nn.ReLU())
        self.base.append(nn.Conv2d(ch_list[-1], ch_list[-1], 3, 2, 1, groups=ch_list[-1]))
        self.base.append(nn.Conv2d(ch_list[-1], 512, 1, groups=512))
        self._init_plan_owner()
        self.out_channels = 512

    def __getstate__(self):
        st = super().__getstate__()
        st.pop("_unit_table", None)                              # (rebuilt on demand)
        return st

    # -- the packed units ---------------------------------------------------------------------------
    def _units(self):
        """The backbone's packed units in ``base`` order ("The unit table"), built once per instance: one
        per key ``build_plan`` asks ``plan.packed`` for.  Every parameter of the module belongs to exactly one unit, in
        ``parameters()`` order, so "the units from index s on" are "the parameters from ``base[s]`` on": what a training mode
        reaches is what the refresh (``hardnet_grads.refresh_packs``) watches."""
        table = self.__dict__.get("_unit_table")
        if table is not None:
            return table
        if not self.depth_wise:
            raise TsodError("depth_wise=False HarDNet (max-pool variant) has no HIP path; the reference only "
                            "uses depth_wise=True")
        table, blk = [], None

        def add(name, i, module, make, write):
            table.append(Unit(name, i, module, make, write))

        def add_dw(name, i, layer):
            add(name, i, layer, partial(_dw_params, layer.dwconv, layer.norm), copy_pack)
        for i, m in enumerate(self.base):
            if i < 2:
                add(f"base.{i}", i, m, partial(_stem_pack, m, **(dict(stride=2, pad=1, cin_pad=4) if i == 0 else {})), rewrite_raw_conv)
            elif isinstance(m, HarDBlock):
                blk, real = m, m.slice_table()[0]
                for l, comb in enumerate(m.layers):
                    add(f"base.{i}.layers.{l}.layer1", i, comb.layer1, partial(_pw_pack, comb.layer1, [real[k] for k in m.links[l]]),
                        rewrite_raw_conv)
                    add_dw(f"base.{i}.layers.{l}.layer2", i, comb.layer2)
            elif isinstance(m, ConvLayer):                       # the transition layer of ``blk``: its output slices, oldest first
                real = blk.slice_table()[0]
                add(f"base.{i}", i, m, partial(_pw_pack, m, [real[k] for k in blk.output_slices()]), rewrite_raw_conv)
            elif isinstance(m, DWConvLayer):
                add_dw(f"base.{i}", i, m)
            elif isinstance(m, nn.Conv2d):                        # the tail: two depthwise 3x3, the grouped pair 1x1
                add(f"base.{i}", i, m, partial(_pair_params, m) if m.kernel_size == (1, 1) else partial(_dw_params, m, None), copy_pack)
        self.__dict__["_unit_table"] = table
        return table

    # -- training modes (DESIGN.md sections 4.17 - 4.19) ----------------------------------------------
    def _tail_indices(self):
        """Indices in ``base`` of the tail's three layers: dw3x3 s2 (+ ReLU), dw3x3 s2, grouped pair 1x1."""
        n = len(self.base)
        return n - 4, n - 2, n - 1

    def tail_parameters(self):
        """The six tail tensors, in the order of ``base``: two depthwise (weight, bias) pairs, the pair conv's weight, bias."""
        return [p for i in self._tail_indices() for p in (self.base[i].weight, self.base[i].bias)]

    def _block_indices(self):
        return [i for i, m in enumerate(self.base) if isinstance(m, HarDBlock)]

    @property
    def n_blocks(self) -> int:
        """The number of HarDBlocks: the largest ``n`` of ``train_blocks(n)``."""
        return len(self._block_indices())

    @property
    def train_mode(self):
        """None | "tail" | n (int >= 1) | "full": what ``set_train_mode`` was given last."""
        return self._train_mode

    def _mode_start(self, mode) -> int:
        """Index in ``base`` of the first module ``mode`` reaches (None: the tail's, for ``trainable_parameters``)."""
        if mode == "full":
            return 0
        return self._tail_indices()[0] if mode in (None, "tail") else self._block_indices()[-mode]

    def set_train_mode(self, mode, batch_stats=False, dropout=False):
        """How much of the backbone is differentiable: None (nothing, the default), "tail" (the last four modules of ``base``:
        the two depthwise 3x3 stride-2 convs, the ReLU between them, the grouped 1x1), ``n`` >= 1 (the tail and the last ``n``
        HarDBlocks: every ``CombConvLayer`` of those blocks, each block's transition ``ConvLayer``, any ``DWConvLayer`` between
        them; ValueError beyond ``n_blocks``) or "full" (every parameter: the stem ``base.0`` - ``base.2`` too).  Returns self.

        The contract of every mode: eval() only; BatchNorm stays folded - its ``weight`` / ``bias`` get gradients through the
        folded scale / shift, its running statistics are constants.  While a mode is on and grad mode enabled, the feature map
        that ``forward`` / ``forward_nhwc`` return carries an autograd node (``hardnet_grads._BackboneGrads``, HIP kernels of
        csrc/dw_grads.hip, pw_grads.hip, conv3x3_grads.hip) that gives the gradients of ``trainable_parameters()`` and nothing
        for the image.  The forward runs the same launches on a plan of its own (another plan-cache key) and returns the same
        bits.  In-place updates of the parameters (an optimizer step) are noticed through their ``_version`` before the next
        forward of ANY kind (grad mode on or off, the mode switched off again included) for everything the widest mode ever
        set reaches, and every packed image derived from a changed layer (gathered / packed f32 weight, folded scale / shift,
        bf16x3 / fp16x2 image, depthwise and pair packs) is rewritten in place - plans keep their pointers.

        The three wrappers keep two quirks: ``train_tail(True)`` never narrows - after ``train_full()`` or ``train_blocks(n)`` it
        leaves the mode as it is and only turns None into "tail" (``train_tail(False)`` sets None) - and ``train_blocks(0)`` is
        "tail", ``train_blocks(n)`` after ``train_full()`` goes back to everything but the stem.

        ``f.grad_fn.saved`` is the dict the backward reads (the node's own copies, so forwards and backwards interleave in any
        order): ``inputs`` / ``packs`` / ``C`` / ``tail_indices``: the tail's three inputs as (tensor, channel offset), packs,
        channels, indices; ``names``: the parameter names in ``trainable_parameters()`` order; ``blocks``: per trainable
        HarDBlock in ``base`` order a dict ``index``, ``buf`` (the block buffer [N,h,w,P]: slice 0 = the block's input, slice i =
        layer i's output), ``layers`` (per layer: ``y`` = the 1x1's output [N,h,w,cout_pad], ``off`` / ``cout`` = its slice,
        ``segs`` / ``seg_real`` / ``slices`` = what it gathers, ``w`` / ``scale`` / ``bn`` = its packed weight, folded scale and
        BN statistics, ``dw`` / ``dw_bn`` = the depthwise pack and its BN statistics), ``transition`` (the 1x1 keys for the
        block's transition layer, ``y`` its output - None for the last block, whose output is ``inputs[0]`` - ``index`` its
        place in ``base``) and ``down`` (the ``DWConvLayer`` in front of the block: ``index``, ``dw``, ``dw_bn``, ``stride``; or
        None); in "full" mode ``stem``: ``x4`` (the image as the plan staged it, [N,H,W,4]), ``y0`` (``base.0``'s output), ``w0`` /
        ``scale0`` / ``bn0`` (its packed weight [c0,3,3,4], folded scale, BN statistics), ``base1`` (``base.1`` with the keys of a
        block layer's 1x1, ``y`` its output) and ``dw`` / ``dw_bn`` (``base.2``'s).

        ``batch_stats=True`` (modes ``n`` and "full"; "tail" has no BatchNorm and ignores it) adds the reference's contract,
        ``.train()``: under ``.eval()`` nothing changes (same plan-cache key, same bits); under ``.train()`` with grad mode on the
        forward takes a plan of its own variant in which every BatchNorm from the mode's first module on normalises with the
        statistics of the current batch (over N, H, W), backpropagates through them and updates its ``running_mean``,
        ``running_var`` (momentum, unbiased variance) and ``num_batches_tracked`` in the module's own storage - current when
        ``forward`` returns; the section below stays folded on its running statistics (frozen BN) and its buffers do not change
        by a bit.  Per such layer the conv runs with an identity epilogue into a raw buffer z, then tsod_bn_stats_f32 and
        tsod_bn_apply_f32 write where the folded launch wrote; the backward runs tsod_bn_train_grad_f32
        on the masked gradient and feeds dz to the conv backward with unit scale.  The records then carry ``bnt`` / ``dw_bnt`` /
        ``bnt0`` (``z``, ``mean``, ``invstd``, ``gamma``, ``C``) where they carried ``bn`` / ``dw_bn`` / ``bn0`` (then None), and
        ``scale`` is ones.  Without ``dropout`` the ``nn.Dropout`` modules of ``base`` (HarDNet-85) stay the identity, as on
        every other path - a difference from the reference.  Under ``.train()`` with grad mode off, or without ``batch_stats``,
        the forward raises ``call .eval() first`` as before.  A BatchNorm of the section with ``momentum=None`` or
        ``track_running_stats=False``: NotImplementedError here.  Memory on top of the mode's: the raw z of every BatchNorm of
        the section, N x h x w x C_pad floats each, twice (plan and node) - for ``n = 1``, HarDNet-39, 600 x 600, batch 1:
        150 x 150 pixels x (2 x 988 + 1 024) channels x 4 B = 270 MB, twice.

        ``dropout=True`` (only with ``batch_stats=True``, i.e. modes ``n`` and "full": ValueError otherwise - nothing else runs
        under ``.train()``) makes the ``nn.Dropout`` modules of the mode's section active wherever the batch-statistics variant
        runs: the transition ConvLayer behind such a module (HarDNet-85: ``base.18`` behind the last
        HarDBlock and ``base.17`` = ``nn.Dropout(0.1)``; ``p`` is read when the plan is built) and its weight gradient read a
        DROPPED copy of the block's output slices (tsod_dropout_segs_f32: a Philox4x32-10 mask of the logical concatenated
        tensor, kept values times 1 / (1 - p)) at the same slice offsets, the layers inside the block keep reading the block buffer itself, and the
        backward masks the transition's input gradient in place with the same key before anything else adds to the block's
        gradient buffer.  Every such forward draws one 64-bit key on the host - from ``self.dropout_generator`` (a CPU
        ``torch.Generator``) if one is assigned, else ``torch.default_generator`` - without any device synchronisation, a kernel
        puts its two words where the plan's launches read them, the node keeps its own copy, and ``self.last_dropout_key`` =
        (lo, hi) afterwards.  No mask is stored: the node holds the key (``blocks[i]["dropout"]``: ``p``, ``ordinal``, ``segs``,
        ``C``, ``key``) and makes the dropped copy again from its copy of the block buffer when the backward runs.  Memory on top
        of ``batch_stats``: one more buffer of the block buffer's shape in the plan and one for the duration of the backward -
        HarDNet-85, 600 x 600, batch 1: 150 x 150 pixels x 2 408 channels x 4 B = 217 MB each; nothing more in the node.
        Where the section holds no ``nn.Dropout`` with p > 0 (HarDNet-39 / 68), under ``.eval()`` and with grad mode off the flag
        changes nothing: same plan-cache keys, same launches, same bits."""
        if mode not in (None, "tail", "full"):
            mode = int(mode)
            if mode < 1 or mode > self.n_blocks:
                raise ValueError(f"train_blocks: n must be 0..{self.n_blocks} (the HarDBlocks of this backbone), got {mode}")
        if dropout and (not batch_stats or mode in (None, "tail")):
            raise ValueError("dropout=True needs batch_stats=True and a mode with BatchNorm (a number of HarDBlocks or 'full'): "
                             f"only the batch-statistics variant runs under .train(); got mode={mode!r}, batch_stats={batch_stats!r}")
        batch_stats = bool(batch_stats) and mode not in (None, "tail")
        if batch_stats:
            for name, bn in self._section_norms(self._mode_start(mode)):
                if bn.momentum is None or not bn.track_running_stats or not bn.affine:
                    raise NotImplementedError(f"batch_stats: {name} has momentum=None, track_running_stats=False or affine=False; "
                                              "only the reference's BatchNorm2d (momentum, running statistics, affine) is built")
        self._train_mode, self._batch_stats, self._dropout = mode, batch_stats, bool(dropout)
        if mode is not None:                                     # the widest mode ever set: where the refresh starts
            self.__dict__["_watch_from"] = min(self._mode_start(mode), self.__dict__.get("_watch_from", len(self.base)))
        return self

    def train_tail(self, enabled: bool = True):
        """``set_train_mode("tail")`` unless a wider mode is on (it stays); False: ``set_train_mode(None)``.
        Memory: the plan keeps its three tail inputs out of its buffer pool and the node copies them - the first is the
        trunk's stride-4 output, N x H/4 x W/4 x 1024 floats (92 MB at 600x600 batch 1, 2.2 GB at 800x1333 batch 8), held until
        the node is freed; the plan for grad mode off is a second plan of the same shape."""
        return self.set_train_mode((self._train_mode or "tail") if enabled else None)

    def train_blocks(self, n: int, batch_stats=False, dropout=False):
        """``set_train_mode(n, batch_stats, dropout)``; ``n = 0`` is "tail".  The stem is never reached (``train_full`` adds it).
        Memory: the plan keeps the section's block buffers, 1x1 outputs and transition outputs out of its pool and the node
        copies them, per block N x h x w x (P + sum of the layers' padded widths + the transition's width) floats: for
        ``n = 1``, HarDNet-39, 600 x 600, batch 1 that is 150 x 150 pixels x (1 628 + 988 + 1 024) channels x 4 B = 328 MB,
        twice (plan and node), plus one zeroed gradient buffer of the block buffer's size per block during the backward."""
        return self.set_train_mode(int(n) or "tail", batch_stats, dropout)

    def train_full(self, batch_stats=False, dropout=False):
        """``set_train_mode("full", batch_stats, dropout)``: ``trainable_parameters()`` is then every parameter of the module in
        ``base`` order.
        Memory on top of ``train_blocks(all)``: N x H x W x 4 floats of image and N x H/2 x W/2 x (c0 + c1) floats of stem
        outputs, twice (plan and node), plus one gradient buffer of ``base.0``'s output during the backward: HarDNet-39 at
        600 x 600, batch 1: 5.8 + 25.9 MB; at 800 x 1333, batch 8: 137 + 615 MB."""
        return self.set_train_mode("full", batch_stats, dropout)

    def trainable_parameters(self):
        """The parameters the feature map's autograd node reaches, in ``base`` order: everything from the first module of the
        mode on (conv weights, BN ``weight`` / ``bias``, the six tail tensors last); with no mode on, ``tail_parameters()``."""
        return [p for _, p in self._trainable_named()]

    def _trainable_named(self):
        start = self._mode_start(self._train_mode)
        return [(f"{u.name}.{k}", p) for u in self._units() if u.index >= start for k, p in u.module.named_parameters()]

    def _active_mode(self):
        return self._train_mode if torch.is_grad_enabled() else None

    def _section_norms(self, start):
        """(name, BatchNorm2d) of every unit from ``base[start]`` on, in ``base`` order."""
        return [(u.name + ".norm", u.module.norm) for u in self._units() if u.index >= start and hasattr(u.module, "norm")]

    def _trains_in_plan(self) -> bool:
        """The batch-statistics variant is on: ``batch_stats`` set, ``.train()``, grad mode on."""
        return self._batch_stats and self.training and self._active_mode() not in (None, "tail")

    def _drops_in_plan(self) -> bool:
        """Active dropout is on: ``dropout`` set, the batch-statistics variant on, and an ``nn.Dropout`` with p > 0 in the section."""
        return (self._dropout and self._trains_in_plan()
                and any(isinstance(m, nn.Dropout) and m.p > 0 for m in self.base[self._mode_start(self._active_mode()):]))

    def _before_train_run(self, plan):
        """One 64-bit key per training forward with active dropout: drawn on the host, written by a kernel where the plan's
        dropout launches read it (stream-ordered, no synchronisation)."""
        if plan.dropout_key is not None:
            gen = self.dropout_generator if self.dropout_generator is not None else torch.default_generator
            lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64, generator=gen).tolist()
            hip_ops.dropout_key(plan.device, lo, hi, out=plan.dropout_key)
            self.last_dropout_key = (lo, hi)

    def _plan_variant(self):
        mode = self._active_mode()
        if mode is None:
            return ()
        key = ("train_" + mode,) if isinstance(mode, str) else ("train_blocks", mode)
        if self._trains_in_plan():
            key += ("batch_stats", "dropout") if self._drops_in_plan() else ("batch_stats",)
        return key

    def _mode_norms(self):
        return self._section_norms(self._mode_start(self._train_mode))

    def forward_nhwc(self, x, slot: int = 0):
        if self._active_mode() is not None:
            return self._forward_train(x, slot, nchw=False)
        refresh_packs(self)
        return super().forward_nhwc(x, slot)

    # -- plan (cache, invalidation, lookup: engine.PlanOwner) -----------------------------------
    def build_plan(self, N, H, W, device, slot=0) -> Plan:
        units = {u.name: u for u in self._units()}               # (raises for depth_wise=False: no HIP path)
        plan = self._new_plan(device, slot)
        L = lib()
        mods = list(self.base)
        x4 = plan.pool.alloc((N, H, W, 4))
        plan.input_nhwc = x4
        # a training mode (with grad mode on): everything from base[start] on is trainable; what the autograd node needs of it
        # stays out of the pool (the node copies it after the run) and is recorded for it; the launches are the same
        mode = self._active_mode()
        start = len(mods) if mode is None else self._mode_start(mode)
        plan.tail, plan.block_records, plan.stem_record, pending_down = [], [], None, None
        # the batch-statistics variant (section 4.20): a BatchNorm at base[i], i >= start, runs as conv with identity epilogue ->
        # raw z (kept for the node, outside the pool) -> tsod_bn_stats_f32 -> tsod_bn_apply_f32 into the folded launch's place
        batch_stats = plan.batch_stats = self._trains_in_plan()
        drops, n_dropouts = self._drops_in_plan(), 0             # (n_dropouts: the nn.Dropout modules met so far = the next ordinal)

        def pack(name, raw=False):
            pc = plan.packed(name, lambda: units[name].make(device))
            return _IdentityEpilogue(pc, device) if raw else pc

        def bn_pack(name, bn, cp):
            return None if batch_stats else plan.packed(name + ".bn", lambda: bn_fold_stats(bn, cp, device))

        def raw_like(dst_shape, cp):
            return torch.empty(tuple(dst_shape[:3]) + (cp,), dtype=torch.float32, device=device)

        def emit_bn(bn, z, C, act, dst, dst_off):
            """batch statistics of z [N,h,w,C_pad] and y = act(BN(z)) into dst's slice -> what the node keeps of it"""
            cp = z.shape[3]
            bnt, scale, shift = plan.bn_stats(bn, z, C, "a BatchNorm of the trainable section")
            M = z.numel() // cp
            plan.call(L.tsod_bn_apply_f32, ptr(z), M, C, cp, cp, 0, ptr(scale), ptr(shift), act, ptr(dst), dst.shape[3], dst_off,
                      plan.amax_ptr(dst) or None, keep=(dst,))
            return bnt

        def conv_bn(name, layer, rc, x, dst, dst_off, C, train, **kw):
            """a ConvLayer's launch(es): folded, or (train) conv -> z, batch statistics, apply; -> the node's ``bnt`` or None"""
            if not train:
                plan.conv(rc, x, dst, out_off=dst_off, name=name, **kw)
                return None
            z = raw_like(dst.shape, rc.cout)
            plan.conv(rc, x, z, name=name, **kw)
            return emit_bn(layer.norm, z, C, ACT_RELU6, dst, dst_off)

        def pw_record(name, index, rc, bn, cout, real, offs, slices, y, y_off=0, off=0, bnt=None):
            """a trainable 1x1 ConvLayer for the node (hardnet_grads.pw_copy)"""
            return dict(index=index, rc=rc, slices=list(slices), segs=[(offs[k], _pad4(real[k])) for k in slices],
                        seg_real=[real[k] for k in slices], cout=cout, y=y, y_off=y_off, off=off, bn=bn_pack(name, bn, rc.cout),
                        bnt=bnt)

        def dw_record(name, index, dw, bn, stride, C, x=None):
            """a trainable depthwise layer (or the pair conv) for the node (hardnet_grads.dw_copy)"""
            dw, bnt = (dw[:4], dw[4]) if len(dw) == 5 else (dw, None)
            return dict(index=index, dw=dw, stride=stride, C=C, x=x, dw_bn=None if bn is None else bn_pack(name, bn, dw[3]),
                        dw_bnt=bnt)

        def dest_for(next_idx, C, h, w):
            """Where the tensor feeding module ``next_idx`` must be written: slice 0 of the next
            HarDBlock's buffer, or a fresh tensor."""
            nxt = mods[next_idx] if next_idx < len(mods) else None
            if isinstance(nxt, HarDBlock):
                _, _, P = nxt.slice_table()
                return plan.pool.alloc((N, h, w, P)), 0
            return plan.pool.alloc((N, h, w, _pad4(C))), 0

        def emit_dw(name, src, src_off, stride, relu, dst, dst_off, bn=None):
            """``bn``: the layer's BatchNorm where it runs on batch statistics; the pack returned then has unit scale, zero shift
            and the node's ``dw_bnt`` as a fifth entry (dw_record takes it off)"""
            w33, scale, shift, cp = dw = pack(name)
            n, h, w_, P = src.shape
            out, out_off = dst, dst_off
            if bn is not None:
                scale, shift = plan.packed(("identity", cp), lambda: (torch.ones(cp, dtype=torch.float32, device=device),
                                                                      torch.zeros(cp, dtype=torch.float32, device=device)))
                out, out_off = raw_like(dst.shape, cp), 0
            plan.call(L.tsod_dwconv3x3_amax_f32, ptr(src), n, h, w_, cp, P, src_off, ptr(w33), ptr(scale), ptr(shift), stride,
                      1 if relu else 0, ptr(out), out.shape[3], out_off, plan.amax_ptr(out) or None, keep=(src, out, w33, scale, shift))
            if bn is not None:
                return (w33, scale, shift, cp, emit_bn(bn, out, bn.num_features, ACT_NONE, dst, dst_off))
            return dw

        # --- stem: 3x3 s2 conv (3 -> c0, input padded to 4 channels), 1x1 conv, dw3x3 s2
        stem_bn = batch_stats and start == 0
        pc0 = pack("base.0", stem_bn)
        h, w = pc0.out_hw(H, W)
        t0 = plan.pool.alloc((N, h, w, pc0.cout))
        bnt0 = conv_bn("base.0", mods[0], pc0, x4, t0, 0, mods[0].norm.num_features, stem_bn)
        pc1 = pack("base.1", stem_bn)
        t1 = plan.pool.alloc((N, h, w, pc1.cout))
        bnt1 = conv_bn("base.1", mods[1], pc1, t0, t1, 0, mods[1].norm.num_features, stem_bn)
        if start > 0:
            plan.pool.release(t0)
        h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        cur, cur_off = dest_for(3, pc1.cout, h2, w2)
        dw = emit_dw("base.2", t1, 0, 2, False, cur, cur_off, mods[2].norm if stem_bn else None)
        if start > 0:
            plan.pool.release(t1)
        else:                                                    # "full": the stem's two outputs and the staged image stay
            plan.stem_record = dict(y0=t0, pc0=pc0, bn0=bn_pack("base.0", mods[0].norm, pc0.cout), bnt0=bnt0,
                                    base1=pw_record("base.1", 1, pc1, mods[1].norm, pc1.cout, [pc1.cin], [0], [0], t1, bnt=bnt1),
                                    base2=dw_record("base.2", 2, dw, mods[2].norm, 2, pc1.cout))
        cur_C = pc1.cout
        h, w = h2, w2

        i = 3
        while i < len(mods):
            m = mods[i]
            if isinstance(m, HarDBlock):
                real, offs, P = m.slice_table()
                assert cur.shape[3] == P and cur_C == real[0]
                buf = cur
                rec = None
                if i >= start:                                   # its buffer, 1x1 outputs and transition output stay
                    rec = dict(index=i, buf=buf, layers=[], transition=None, down=pending_down)
                    plan.block_records.append(rec)
                pending_down = None
                for li, comb in enumerate(m.layers, start=1):
                    link = m.links[li - 1]
                    name = f"base.{i}.layers.{li - 1}"
                    bn_on = batch_stats and rec is not None
                    rc = pack(name + ".layer1", bn_on)
                    tmp = plan.pool.alloc((N, h, w, rc.cout))
                    bnt = conv_bn(name + ".layer1", comb.layer1, rc, buf, tmp, 0, real[li], bn_on,
                                  segs=[(offs[k], _pad4(real[k])) for k in link])
                    dw = emit_dw(name + ".layer2", tmp, 0, 1, False, buf, offs[li], comb.layer2.norm if bn_on else None)
                    if rec is not None:
                        rec["layers"].append((pw_record(name + ".layer1", i, rc, comb.layer1.norm, real[li], real, offs, link, tmp,
                                                        0, offs[li], bnt=bnt),
                                              dw_record(name + ".layer2", i, dw, comb.layer2.norm, 1, real[li])))
                    else:
                        plan.pool.release(tmp)
                # transition 1x1 conv gathers the block's output slices (oldest first)
                outs = m.output_slices()
                i += 1
                src = buf
                if isinstance(mods[i], nn.Dropout):
                    if drops and rec is not None and mods[i].p > 0:
                        # active dropout (section 4.26): the transition reads a dropped copy of the output slices, at their offsets
                        if plan.dropout_key is None:
                            plan.dropout_key = torch.zeros(2, dtype=torch.int32, device=device)
                        dsegs, C_out = [], 0
                        for k in outs:                           # (offset in the pixel, real width, first logical channel)
                            dsegs.append((offs[k], real[k], C_out))
                            C_out += real[k]
                        src, table = torch.empty_like(buf), hip_ops.dropout_seg_table(dsegs)
                        plan.call(L.tsod_dropout_segs_f32, ptr(buf), ptr(src), N, h, w, P, P, table, len(dsegs), C_out, float(mods[i].p),
                                  ptr(plan.dropout_key), n_dropouts, 0, keep=(buf, src, table, plan.dropout_key))
                        rec["dropout"] = dict(p=float(mods[i].p), ordinal=n_dropouts, segs=dsegs, C=C_out, key=plan.dropout_key)
                    n_dropouts += 1
                    i += 1
                rc = pack(f"base.{i}", batch_stats and rec is not None)
                dst, dst_off = dest_for(i + 1, rc.cout, h, w)
                if isinstance(mods[i + 1], DWConvLayer):          # "downsample" dw3x3 at stride 1 follows
                    plan.pool.release(dst)
                    dst, dst_off = plan.pool.alloc((N, h, w, rc.cout)), 0
                bnt = conv_bn(f"base.{i}", mods[i], rc, src, dst, dst_off, rc.cout_real, batch_stats and rec is not None,
                              segs=[(offs[k], _pad4(real[k])) for k in outs])
                if rec is not None:
                    # (the last block's transition output is the tail's first input: its mask is taken there)
                    last = not any(isinstance(later, HarDBlock) for later in mods[i + 1:])
                    rec["transition"] = pw_record(f"base.{i}", i, rc, mods[i].norm, rc.cout_real, real, offs, outs,
                                                  None if last else dst, dst_off, bnt=bnt)
                else:
                    plan.pool.release(buf)
                cur, cur_off, cur_C = dst, dst_off, rc.cout
                i += 1
            elif isinstance(m, DWConvLayer):
                dst, dst_off = dest_for(i + 1, cur_C, h, w)
                dw = emit_dw(f"base.{i}", cur, cur_off, m.dwconv.stride[0], False, dst, dst_off,
                             m.norm if batch_stats and i > start else None)
                if i > start:                                    # between two trainable blocks: its input stays
                    pending_down = dw_record(f"base.{i}", i, dw, m.norm, m.dwconv.stride[0], cur_C)
                else:
                    plan.pool.release(cur)
                cur, cur_off = dst, dst_off
                i += 1
            elif isinstance(m, nn.Conv2d) and m.groups == m.in_channels and m.kernel_size == (3, 3):
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                s = m.stride[0]
                nh, nw = (h - 1) // s + 1, (w - 1) // s + 1
                dst = plan.pool.alloc((N, nh, nw, _pad4(cur_C)))
                dw = emit_dw(f"base.{i}", cur, cur_off, s, relu, dst, 0)
                if i >= start:
                    plan.tail.append(dw_record(f"base.{i}", i, dw, None, s, cur_C, (cur, cur_off)))
                else:
                    plan.pool.release(cur)
                cur, cur_off, h, w = dst, 0, nh, nw
                i += 2 if relu else 1
            elif isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and m.groups == m.out_channels \
                    and m.in_channels == 2 * m.out_channels:
                G = m.out_channels
                wg, bias = pack(f"base.{i}")
                dst = plan.pool.alloc((N, h, w, G))
                plan.call(L.tsod_gconv1x1_pair_amax_f32, ptr(cur), N * h * w, G, cur.shape[3], ptr(wg), ptr(bias), ptr(dst), G,
                          plan.amax_ptr(dst) or None, keep=(cur, dst, wg, bias))
                if i >= start:
                    plan.tail.append(dw_record(f"base.{i}", i, (wg, bias), None, 1, G, (cur, cur_off)))
                else:
                    plan.pool.release(cur)
                cur, cur_off, cur_C = dst, 0, G
                i += 1
            else:
                raise TsodError(f"no HIP lowering for base.{i}: {type(m).__name__}")
        plan.tail_inputs = [r["x"] for r in plan.tail]           # (tensor, channel offset) of the three tail layers
        plan.output_nhwc = cur
        plan.output_amax = plan.amax_ptr(cur)
        return plan.finalize()

    def forward(self, x):
        if self._active_mode() is not None:
            return self._forward_train(x, 0, nchw=True)
        return hip_ops.nhwc_to_nchw(self.forward_nhwc(x))


class HarNetClassifier(nn.Module):
    """AdaptiveAvgPool2d(1) + Flatten (reference :203-212; attribute name ``clssifier`` kept).  Inside the
    detector it is fused into the RoI pooling kernel; stand-alone it averages an NCHW tensor's H*W."""

    def __init__(self):
        super().__init__()
        self.clssifier = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten())

    def forward(self, x):
        require_cuda(x, "HarNetClassifier")
        n, c, h, w = x.shape
        # mean over H*W as a GEMM against a constant 1/(H*W) row on the f32 MFMA path
        hw = h * w
        flat = torch.nn.functional.pad(x.reshape(n * c, hw), (0, _pad4(hw) - hw)).contiguous()   # K % 4 == 0 for the GEMM
        ones = torch.zeros((4, _pad4(hw)), dtype=torch.float32, device=x.device)
        ones[:, :hw] = 1.0 / hw
        return hip_ops.linear(flat, ones)[:, 0].reshape(n, c)
