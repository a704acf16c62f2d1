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

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _ffi, hip_ops
from .._ffi import ACT_NONE, ACT_RELU6, TsodError, lib, ptr, require_cuda
from ..engine import PackedConv, Plan, PlanOwner, fold_bn, stage_input


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


class _TailGrads(torch.autograd.Function):
    """The feature map of a ``train_tail`` forward as an autograd node over the six tail tensors.

    forward(saved, *params) hands out the map the plan computed; backward runs tsod_gconv1x1_pair_grad_f32 and
    tsod_dwconv3x3_grad_f32 twice on the node's OWN copies of the three tail inputs and of the packed weights of its forward,
    and returns the six gradients in torch's parameter layouts (autograd adds them into ``.grad``)."""

    @staticmethod
    def forward(ctx, saved, *params):
        ctx.saved = saved
        return saved.pop("out")

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        sv, need = ctx.saved, ctx.needs_input_grad[1:]
        g = hip_ops.nchw_to_nhwc(gy) if sv["nchw"] else gy.contiguous()
        (x0, off0), (a, _), (b, _) = sv["inputs"]
        (w1, _, sh1, _), (w2, _, sh2, _), (wg, bias) = sv["packs"]
        d_b, d_wg, d_bias = hip_ops.gconv1x1_pair_grad(b, wg, g, want_dw=need[4], want_dbias=need[5])
        d_a, d_w2, _, d_sh2 = hip_ops.dwconv3x3_grad(a, w2, None, sh2, 2, False, d_b)
        _, d_w1, _, d_sh1 = hip_ops.dwconv3x3_grad(x0, w1, None, sh1, 2, True, d_a, want_dx=False, in_off=off0)
        C = sv["C"]

        def conv_weight(d):                                   # [3][3][C_pad] -> torch's [C,1,3,3]
            return d[:, :, :C].reshape(9, C).t().reshape(C, 1, 3, 3)
        grads = (conv_weight(d_w1), d_sh1[:C], conv_weight(d_w2), d_sh2[:C],
                 None if d_wg is None else d_wg.view(-1, 2, 1, 1), d_bias)
        return (None,) + tuple(d if n else None for d, n in zip(grads, need))


def _bn_stats(bn, C_pad, device):
    """(running mean, 1 / sqrt(running var + eps)) of an eval-mode BatchNorm, padded to ``C_pad`` with zeros: what turns
    (dscale, dshift) into the gradients of ``weight`` / ``bias`` (scale = weight * inv, shift = bias - mean * scale)."""
    inv = 1.0 / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    return _padded(bn.running_mean.detach(), C_pad).to(device), _padded(inv, C_pad).to(device)


def _bn_grads(dscale, dshift, stats, C):
    """d weight = (dscale - mean * dshift) * inv, d bias = dshift (DESIGN.md section 4.17's folding rule), on [C] vectors."""
    mean, inv = stats
    return (dscale[:C] - mean[:C] * dshift[:C]) * inv[:C], dshift[:C]


def _conv33_weight(d, C):                                     # [3][3][C_pad] -> torch's [C,1,3,3]
    return d[:, :, :C].reshape(9, C).t().reshape(C, 1, 3, 3)


class _BlockGrads(torch.autograd.Function):
    """The feature map of a ``train_blocks(n >= 1)`` forward as an autograd node over ``trainable_parameters()`` (DESIGN.md
    section 4.18): the tail's backward of ``_TailGrads``, whose first depthwise conv now also returns the masked gradient of
    the last transition layer (tsod_dwconv3x3_grad_act_f32), then per HarDBlock from the last one down: the transition's
    tsod_pw_wgrad_f32 / tsod_pw_dgrad_f32 into a zeroed block-shaped gradient buffer, the layers in descending order (depthwise
    backward with the fused ReLU6 mask, then the 1x1's wgrad and dgrad into the slices it gathered from, added in that order),
    and the ``DWConvLayer`` in front of the block.  Everything runs on the node's own copies (``ctx.saved``)."""

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

        def dw_layer(prefix, x, pack, stats, C, stride, dy, dy_off):
            """backward of a DWConvLayer whose input x is a ReLU6 output -> that layer's masked gradient"""
            w33, sc, sh = pack
            want = need[prefix + ".dwconv.weight"] or any(wants(prefix + ".norm"))
            g, d_w, d_sc, d_sh = hip_ops.dwconv3x3_grad(x, w33, sc, sh, stride, False, dy, want_params=want, dy_off=dy_off,
                                                        act_dx=True)
            if want:
                out[prefix + ".dwconv.weight"] = _conv33_weight(d_w, C)
                out[prefix + ".norm.weight"], out[prefix + ".norm.bias"] = _bn_grads(d_sc, d_sh, stats, C)
            return g

        def pw_layer(prefix, buf, lay, g, dbuf, want_seg):
            """backward of a 1x1 ConvLayer from its masked gradient g: parameter gradients, and dx added into dbuf"""
            want_w, (want_g, want_b) = need[prefix + ".conv.weight"], wants(prefix + ".norm")
            _, d_w, d_sc, d_sh = hip_ops.conv1x1_bn_relu6_grad(
                buf, lay["segs"], lay["w"], lay["scale"], None, g, seg_real=lay["seg_real"], seg_want=want_seg, cout=lay["cout"],
                dx=dbuf, accumulate=True, want_dx=any(want_seg), want_dw=want_w, want_dscale=want_g, want_dshift=want_g or want_b)
            if want_w:
                out[prefix + ".conv.weight"] = d_w.view(d_w.shape[0], d_w.shape[1], 1, 1)
            if want_g or want_b:
                zero = d_sh if d_sc is None else d_sc
                out[prefix + ".norm.weight"], out[prefix + ".norm.bias"] = _bn_grads(zero, d_sh, lay["bn"], lay["cout"])

        # ---- the tail (section 4.17), with the last transition's mask fused into its first layer's dx gather
        g0 = hip_ops.nchw_to_nhwc(gy) if sv["nchw"] else gy.contiguous()
        (x0, off0), (a, _), (b, _) = sv["inputs"]
        (w1, _, sh1, _), (w2, _, sh2, _), (wg, bias) = sv["packs"]
        i1, i2, ip = sv["tail_indices"]
        d_b, d_wg, d_bias = hip_ops.gconv1x1_pair_grad(b, wg, g0, want_dw=need[f"base.{ip}.weight"], want_dbias=need[f"base.{ip}.bias"])
        d_a, d_w2, _, d_sh2 = hip_ops.dwconv3x3_grad(a, w2, None, sh2, 2, False, d_b)
        g, d_w1, _, d_sh1 = hip_ops.dwconv3x3_grad(x0, w1, None, sh1, 2, True, d_a, in_off=off0, act_dx=True)
        C = sv["C"]
        out.update({f"base.{i1}.weight": _conv33_weight(d_w1, C), f"base.{i1}.bias": d_sh1[:C],
                    f"base.{i2}.weight": _conv33_weight(d_w2, C), f"base.{i2}.bias": d_sh2[:C],
                    f"base.{ip}.weight": None if d_wg is None else d_wg.view(-1, 2, 1, 1), f"base.{ip}.bias": d_bias})

        # ---- the blocks, last first; g = the masked gradient of the block's transition layer
        blocks, stem = sv["blocks"], sv.get("stem")
        for bi in range(len(blocks) - 1, -1, -1):
            blk = blocks[bi]
            first, buf = bi == 0, blk["buf"]
            dbuf = torch.zeros_like(buf)
            tr = blk["transition"]
            skip0 = first and stem is None                        # the first block's input slice: wanted by the stem only
            pw_layer(f"base.{tr['index']}", buf, tr, g, dbuf, [not (skip0 and k == 0) for k in tr["slices"]])
            for li in range(len(blk["layers"]), 0, -1):
                lay = blk["layers"][li - 1]
                prefix = f"base.{blk['index']}.layers.{li - 1}"
                g = dw_layer(prefix + ".layer2", lay["y"], lay["dw"], lay["dw_bn"], lay["cout"], 1, dbuf, lay["off"])
                pw_layer(prefix + ".layer1", buf, lay, g, dbuf, [not (skip0 and k == 0) for k in lay["slices"]])
            if first:
                break
            prev = blocks[bi - 1]["transition"]
            down = blk["down"]
            if down is not None:                                  # the DWConvLayer between the blocks
                g = dw_layer(f"base.{down['index']}", prev["y"], down["dw"], down["dw_bn"], prev["cout"], down["stride"], dbuf, 0)
            else:                                                 # the transition wrote slice 0 itself
                g = hip_ops.relu6_grad_mask(prev["y"], dbuf, 0)
        # ---- the stem (section 4.19): base.2 reads slice 0 of the first block's gradient, base.1 is a one-segment 1x1 layer,
        # base.0 has parameter gradients only (tsod_conv3x3_wgrad_f32 takes its mask from the saved output)
        if stem is not None:
            lay1 = stem["base1"]
            g = dw_layer("base.2", lay1["y"], stem["dw"], stem["dw_bn"], lay1["cout"], 2, dbuf, 0)
            d0 = torch.zeros_like(stem["y0"])
            pw_layer("base.1", stem["y0"], lay1, g, d0, [True])
            want_w, (want_g, want_b) = need["base.0.conv.weight"], wants("base.0.norm")
            if want_w or want_g or want_b:
                c0 = stem["y0"].shape[3]
                d_w, d_sc, d_sh = hip_ops.conv3x3_bn_relu6_grad(stem["x4"], stem["w0"], stem["scale0"], stem["y0"], d0, stride=2,
                                                                want_dw=want_w, want_dscale=want_g, want_dshift=True)
                out["base.0.conv.weight"] = d_w
                out["base.0.norm.weight"], out["base.0.norm.bias"] = _bn_grads(d_sh if d_sc is None else d_sc, d_sh,
                                                                               stem["bn0"], c0)
        return (None,) + tuple(out.get(k) if n else None for k, n in need.items())


class HarDNetFeatureExtraction(PlanOwner, nn.Module):
    _train_tail = False          # train_tail(): the last four modules of ``base`` are differentiable (default off)
    _train_blocks = 0            # train_blocks(n): ... and the last n HarDBlocks with their transition layers (default 0)
    _train_full = False          # train_full(): ... and the stem, base.0 - base.2: every parameter (default off)

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

    # -- the trainable tail ---------------------------------------------
    def _tail_indices(self):
        """Indices in ``base`` of the tail's three layers: dw3x3 s2 (+ ReLU), dw3x3 s2, grouped pair 1x1."""
        n = len(self.base)
        return n - 4, n - 2, n - 1

    def tail_parameters(self):
        """The six tail tensors, in the order of ``base``: two depthwise (weight, bias) pairs, the pair conv's weight, bias."""
        return [p for i in self._tail_indices() for p in (self.base[i].weight, self.base[i].bias)]

    def train_tail(self, enabled: bool = True):
        """Make the last four modules of ``base`` (the two depthwise 3x3 stride-2 convs, the ReLU between them and the grouped
        1x1) differentiable: while on, with grad mode enabled and the module in eval(), the feature map that ``forward`` /
        ``forward_nhwc`` return carries an autograd node whose backward (HIP kernels, csrc/dw_grads.hip) gives the gradients
        of the six tail tensors.  The forward's launches and values are unchanged; nothing is returned for the input or the
        body's parameters.  In-place updates of the six tensors (an optimizer step) are noticed through their ``_version``
        and the tail's packed weights refreshed before the next forward of ANY kind (grad mode on or off, ``train_tail``
        switched off again included), from the first ``train_tail(True)`` on.

        Memory: a ``train_tail`` forward keeps its three tail inputs out of the plan's buffer pool and the node copies
        them - the first is the trunk's stride-4 output, N x H/4 x W/4 x 1024 floats (92 MB at 600x600 batch 1, 2.2 GB at
        800x1333 batch 8), held until the node is freed; the plan for grad mode off is a second plan of the same shape."""
        self._train_tail = bool(enabled)
        if not enabled:
            self._train_blocks, self._train_full = 0, False
        return self

    # -- the trainable HarDBlocks -----------------------------------------
    def _block_indices(self):
        return [i for i, m in enumerate(self.base) if isinstance(m, HarDBlock)]

    def _section_start(self, n: int) -> int:
        """Index in ``base`` of the earliest of the last ``n`` HarDBlocks."""
        return self._block_indices()[-n]

    def train_blocks(self, n: int):
        """Make the tail AND the last ``n`` HarDBlocks differentiable - every ``CombConvLayer`` of those blocks, each block's
        transition ``ConvLayer`` and any ``DWConvLayer`` between them; ``n = 0`` is ``train_tail(True)``'s state, ``n`` larger
        than the number of HarDBlocks raises ValueError.  The stem (``base.0`` - ``base.2``) is never reached (``train_full``
        adds it), and BatchNorm
        stays in eval mode: its ``weight`` / ``bias`` get gradients through the folded scale / shift, its running statistics
        are constants.  Contract as ``train_tail``: eval() only; with grad mode on the feature map carries an autograd node
        (``_BlockGrads``; HIP kernels of csrc/pw_grads.hip and csrc/dw_grads.hip) that gives the gradients of
        ``trainable_parameters()`` and nothing for the input; the forward runs the same launches on a plan of its own (another
        plan-cache key) and returns the same bits; in-place updates of the trainable tensors are noticed through their
        ``_version`` before the next forward of any kind and every packed image derived from a changed layer (gathered f32
        weight, folded scale / shift, bf16x3 / fp16x2 image) is rewritten in place - plans keep their pointers.

        ``f.grad_fn.saved`` is the dict the backward reads (the node's own copies, so forwards and backwards interleave in any
        order): ``inputs`` / ``packs`` / ``C`` as ``train_tail``; ``names``: the parameter names in ``trainable_parameters()``
        order; ``blocks``: per trainable HarDBlock in ``base`` order a dict ``index``, ``buf`` (the block buffer
        [N,h,w,P]: slice 0 = the block's input, slice i = layer i's output), ``layers`` (per layer: ``y`` = the 1x1's output
        [N,h,w,cout_pad], ``off`` / ``cout`` = its slice, ``segs`` / ``seg_real`` / ``slices`` = what it gathers, ``w`` /
        ``scale`` = its packed weight and folded scale, ``dw`` = the depthwise pack), ``transition`` (the same keys for the
        block's transition layer, ``y`` its output, ``index`` its place in ``base``) and ``down`` (the ``DWConvLayer`` in front
        of the block, or None).

        Memory: the plan keeps the section's block buffers, 1x1 outputs and transition outputs out of its pool and the node
        copies them, per block N x h x w x (P + sum of the layers' padded widths + the transition's width) floats: for
        ``n = 1``, HarDNet-39, 600 x 600, batch 1 that is 150 x 150 pixels x (1 628 + 988 + 1 024) channels x 4 B = 328 MB,
        twice (plan and node), plus one zeroed gradient buffer of the block buffer's size per block during the backward."""
        n = int(n)
        if n < 0 or n > len(self._block_indices()):
            raise ValueError(f"train_blocks: n must be 0..{len(self._block_indices())} (the HarDBlocks of this backbone), got {n}")
        self._train_tail, self._train_blocks, self._train_full = True, n, False
        self.__dict__["_blocks_watch"] = max(n, self.__dict__.get("_blocks_watch", 0))
        return self

    # -- the whole backbone ------------------------------------------------
    def train_full(self):
        """``train_blocks(all the HarDBlocks)`` plus the stem: ``base.0`` (3x3 stride-2 ConvLayer on the image), ``base.1`` (1x1
        ConvLayer) and ``base.2`` (stride-2 DWConvLayer).  ``trainable_parameters()`` is then every parameter of the module in
        ``base`` order.  The contract is ``train_blocks``' otherwise: eval() only, BatchNorm folded (``weight`` / ``bias`` get
        gradients through the folded scale / shift), a plan of its own that runs the same launches and returns the same bits,
        nothing for the image, in-place updates noticed through ``_version`` before the next forward of any kind and every
        image the packed ``base.0`` / ``base.1`` hold (f32 pack, folded scale / shift, bf16x3 and fp16x2 images) and
        ``base.2``'s depthwise pack rewritten in place.  ``train_blocks(n)`` goes back to "everything but the stem",
        ``train_tail(False)`` switches everything off.

        ``f.grad_fn.saved`` gains ``stem``: ``x4`` (the image as the plan staged it, [N,H,W,4]), ``y0`` (``base.0``'s output),
        ``w0`` / ``scale0`` / ``bn0`` (its packed weight [c0,3,3,4], folded scale, BN statistics), ``base1`` (``base.1`` with the
        keys of a block layer, ``y`` its output) and ``dw`` / ``dw_bn`` (``base.2``'s depthwise pack and BN statistics).

        Memory on top of ``train_blocks(all)``: N x H x W x 4 floats of image and N x H/2 x W/2 x (c0 + c1) floats of stem
        outputs, twice (plan and node), plus one gradient buffer of ``base.0``'s output during the backward: HarDNet-39 at
        600 x 600, batch 1: 5.8 + 25.9 MB; at 800 x 1333, batch 8: 137 + 615 MB."""
        self.train_blocks(len(self._block_indices()))
        self._train_full = True
        self.__dict__["_stem_watch"] = True
        return self

    def trainable_parameters(self):
        """The parameters the feature map's autograd node reaches, in ``base`` order: with ``train_blocks(n >= 1)`` everything
        from the earliest of the last ``n`` HarDBlocks on (conv weights, BN ``weight`` / ``bias``), then the six tail tensors;
        otherwise ``tail_parameters()``."""
        return [p for _, p in self._trainable_named()]

    def _trainable_named(self):
        if not self._train_blocks:
            i1, i2, ip = self._tail_indices()
            return [(f"base.{i}.{k}", getattr(self.base[i], k)) for i in (i1, i2, ip) for k in ("weight", "bias")]
        first = 0 if self._train_full else self._section_start(self._train_blocks)
        return [(f"base.{i}.{k}", p) for i in range(first, len(self.base)) for k, p in self.base[i].named_parameters()]

    def _tail_active(self) -> bool:
        return self._train_tail and torch.is_grad_enabled()

    def _blocks_active(self) -> int:
        return self._train_blocks if self._tail_active() else 0

    def _full_active(self) -> bool:
        return self._train_full and self._blocks_active() > 0

    def _plan_variant(self):
        if self._full_active():
            return ("train_full",)
        if self._blocks_active():
            return ("train_blocks", self._blocks_active())
        return ("train_tail",) if self._tail_active() else ()

    def _refresh_block_packs(self):
        """Rewrite in place the packed images of every layer of the widest section ``train_blocks`` was ever given whose
        parameters changed since they were last known to match (``_refresh_tail_packs`` for the body)."""
        n = self.__dict__.get("_blocks_watch", 0)
        if not n:
            return
        seen = self.__dict__.setdefault("_block_versions", {})
        stale = []
        first = 0 if self.__dict__.get("_stem_watch") else self._section_start(n)     # (train_full was on: the stem too)
        for i in range(first, self._tail_indices()[0]):
            m = self.base[i]
            units = [(f"base.{i}", m)] if not isinstance(m, HarDBlock) else \
                [(f"base.{i}.layers.{l}.{k}", getattr(comb, k)) for l, comb in enumerate(m.layers) for k in ("layer1", "layer2")]
            for name, mod in units:
                v = tuple(p._version for p in mod.parameters())
                if seen.get(name) != v:
                    seen[name] = v
                    stale.append(name)
        for name in stale:
            for (key, device), old in list(self._packed_cache.items()):
                if key != name:
                    continue
                with torch.inference_mode():                  # (the packs may have been made under inference mode)
                    if isinstance(old, PackedConv):           # the stem's base.0 / base.1
                        self._rewrite_raw_conv(old, self._stem_pack(name, device))
                    elif isinstance(old, _RawConv):
                        self._rewrite_raw_conv(old, self._pw_pack(name, device))
                    else:
                        parts = name.split(".")
                        mod = self.base[int(parts[1])] if len(parts) == 2 else self.base[int(parts[1])].layers[int(parts[3])].layer2
                        for o, t in zip(old, self._dw_params(mod.dwconv, mod.norm, device)):
                            if isinstance(o, torch.Tensor):
                                o.copy_(t)

    def _rewrite_raw_conv(self, old, new):
        """``new``'s images into ``old``'s storage.  The fp16x2 exponent is part of every launch descriptor that reads the
        image: it is kept while the new weights fit it (graphs stay valid); otherwise the descriptors of every plan follow and
        captured graphs of those plans are dropped (they hold the old exponent by value)."""
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
                for plan in self._plans.values():
                    for st in plan.conv_steps:
                        if st.pc is old and int(st.desc.precision) == _ffi.PREC_FP16X2:
                            st.desc.w_scale_exp = int(e)
                            plan.graph = None
                self._bump_version()
            img.copy_(hip_ops.pack_conv_weight_fp16x2(old.w, e))
            old.w2 = (img, e)

    def _stem_pack(self, name, device):
        """The packed form of ``base.0`` (3x3 stride 2, the image padded to 4 channels) or ``base.1`` (1x1)."""
        if name == "base.0":
            m0 = self.base[0]
            return PackedConv(m0.conv.weight, device, bn=m0.norm, stride=2, pad=1, act=ACT_RELU6, cin_pad=4)
        m1 = self.base[1]
        return PackedConv(m1.conv.weight, device, bn=m1.norm, act=ACT_RELU6)

    def _pw_pack(self, name, device):
        """The packed form of the 1x1 ConvLayer ``name`` (a HarDBlock layer's ``layer1`` or a transition layer): the weight
        gathered to the padded slices it reads, BN folded, padded to 4 output channels."""
        parts = name.split(".")
        if len(parts) == 2:                                       # transition: base.<i>, the block is the HarDBlock before it
            i = int(parts[1])
            bi = max(b for b in self._block_indices() if b < i)
            blk, tr = self.base[bi], self.base[i]
            real = blk.slice_table()[0]
            outs = blk.output_slices()
            wg = _gathered_weight(tr.conv.weight, [real[k] for k in outs], tr.conv.weight.shape[0])
            sc, sh = fold_bn(tr.norm)
            return _RawConv(wg, sc, sh, device, ACT_RELU6, cin_real=sum(real[k] for k in outs))
        blk, li = self.base[int(parts[1])], int(parts[3]) + 1
        real = blk.slice_table()[0]
        comb, link = blk.layers[li - 1], blk.links[li - 1]
        cout, cp = real[li], _pad4(real[li])
        wg = _gathered_weight(comb.layer1.conv.weight, [real[k] for k in link], cp)
        sc, sh = fold_bn(comb.layer1.norm)
        return _RawConv(wg, _padded(sc, cp), _padded(sh, cp), device, ACT_RELU6, cin_real=sum(real[k] for k in link),
                        cout_real=cout)

    def _refresh_tail_packs(self):
        """Rewrite the tail's packed weights (and only those) in place when one of the six tensors changed since they were
        last known to match: plans and graphs keep their pointers; an autograd node of an earlier forward holds copies."""
        if not self._train_tail and "_tail_versions" not in self.__dict__:
            return                                               # train_tail was never on: today's contract (invalidate_packed)
        self._refresh_block_packs()
        versions = tuple(p._version for p in self.tail_parameters())
        if versions == self.__dict__.get("_tail_versions"):
            return
        i1, i2, ip = self._tail_indices()
        for (name, device), pack in list(self._packed_cache.items()):
            if name in (f"base.{i1}", f"base.{i2}"):
                new = self._dw_params(self.base[i1 if name == f"base.{i1}" else i2], None, device)
            elif name == f"base.{ip}":
                new = self._pair_params(self.base[ip], device)
            else:
                continue
            with torch.inference_mode():                      # (the packs may have been made under inference mode)
                for old, t in zip(pack, new):
                    if isinstance(old, torch.Tensor):
                        old.copy_(t)
        self.__dict__["_tail_versions"] = versions

    def _forward_tail(self, x, slot, nchw):
        if self.training:
            raise TsodError("the HIP path implements the inference forward only: call .eval() first")
        self._refresh_tail_packs()
        plan = self._plan_for(x, slot)
        stage_input(plan, x)
        plan.run()
        self.publish_range_word(plan)                            # (fp16x2 range violations of this forward: raise_if_error)
        out = plan.output_nhwc
        saved = dict(out=hip_ops.nhwc_to_nchw(out) if nchw else out.clone(), nchw=nchw,
                     inputs=[(t.clone(), off) for t, off in plan.tail_inputs],
                     packs=[tuple(t.clone() if isinstance(t, torch.Tensor) else t for t in pack) for pack in plan.tail_packs],
                     C=self.base[self._tail_indices()[0]].weight.shape[0])
        if not self._train_blocks:
            return _TailGrads.apply(saved, *self.tail_parameters())

        def layer_copy(rec):
            rc = rec["rc"]
            return dict(index=rec["index"], off=rec["off"], cout=rec["cout"], segs=rec["segs"], seg_real=rec["seg_real"],
                        slices=rec["slices"], w=rc.w.view(rc.cout, -1).clone(), scale=rc.scale.clone(), bn=rec["bn"],
                        y=None if rec["y"] is None else rec["y"][..., rec["y_off"]:rec["y_off"] + rc.cout].clone(),
                        dw=None if rec["dw"] is None else tuple(t.clone() for t in rec["dw"][:3]), dw_bn=rec["dw_bn"])
        saved.update(tail_indices=self._tail_indices(), names=[k for k, _ in self._trainable_named()],
                     blocks=[dict(index=b["index"], buf=b["buf"].clone(), layers=[layer_copy(r) for r in b["layers"]],
                                  transition=layer_copy(b["transition"]),
                                  down=None if b["down"] is None else dict(b["down"], dw=tuple(t.clone() for t in b["down"]["dw"][:3])))
                             for b in plan.block_records])
        if plan.stem_record is not None:
            sr = plan.stem_record
            pc0, pc1 = sr["pc0"], sr["pc1"]
            saved["stem"] = dict(
                x4=plan.input_nhwc.clone(), y0=sr["y0"].clone(), w0=pc0.w.clone(), scale0=pc0.scale.clone(), bn0=sr["bn0"],
                base1=dict(index=1, off=0, cout=pc1.cout, segs=[(0, pc1.cin)], seg_real=[pc1.cin], slices=[0],
                           w=pc1.w.view(pc1.cout, -1).clone(), scale=pc1.scale.clone(), bn=sr["bn1"], y=sr["y1"].clone()),
                dw=tuple(t.clone() for t in sr["dw"][:3]), dw_bn=sr["dw_bn"])
        return _BlockGrads.apply(saved, *self.trainable_parameters())

    def forward_nhwc(self, x, slot: int = 0):
        if self._tail_active():
            return self._forward_tail(x, slot, nchw=False)
        self._refresh_tail_packs()
        return super().forward_nhwc(x, slot)

    @staticmethod
    def _pair_params(m: nn.Conv2d, device):
        G = m.out_channels
        return (m.weight.detach().float().view(G, 2).contiguous().to(device),
                None if m.bias is None else m.bias.detach().float().to(device))

    # -- plan (cache, invalidation, lookup: engine.PlanOwner) -----------------------------------
    @staticmethod
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

    def build_plan(self, N, H, W, device, slot=0) -> Plan:
        if not self.depth_wise:
            raise TsodError("depth_wise=False HarDNet (max-pool variant) has no HIP path; the reference only "
                            "uses depth_wise=True")
        plan = self._new_plan(device, slot)
        L = lib()
        mods = list(self.base)
        x4 = plan.pool.alloc((N, H, W, 4))
        plan.input_nhwc = x4
        # train_tail: the tail's three inputs stay out of the pool (the autograd node copies them after the run) and the
        # packs are listed for it; the launches are the same
        tail = self._tail_active()
        plan.tail_inputs, plan.tail_packs = [], []
        section = self._section_start(self._blocks_active()) if self._blocks_active() else None
        plan.block_records, pending_down = [], None
        full = self._full_active()
        plan.stem_record = None

        def dest_for(next_idx, C, h, w):
            """Where the tensor feeding module ``next_idx`` must be written: slice 0 of the next
            HarDBlock's buffer, or a fresh tensor."""
            nxt = mods[next_idx] if next_idx < len(mods) else None
            if isinstance(nxt, HarDBlock):
                _, _, P = nxt.slice_table()
                return plan.pool.alloc((N, h, w, P)), 0
            return plan.pool.alloc((N, h, w, _pad4(C))), 0

        def emit_dw(src, src_off, C, conv, bn, stride, relu, dst, dst_off, name):
            w33, scale, shift, cp = plan.packed(name, lambda: self._dw_params(conv, bn, device))
            n, h, w_, P = src.shape
            plan.call(L.tsod_dwconv3x3_amax_f32, ptr(src), n, h, w_, cp, P, src_off, ptr(w33), ptr(scale), ptr(shift), stride,
                      1 if relu else 0, ptr(dst), dst.shape[3], dst_off, plan.amax_ptr(dst) or None, keep=(src, dst, w33, scale, shift))
            return w33, scale, shift, cp

        # --- stem: 3x3 s2 conv (3 -> c0, input padded to 4 channels), 1x1 conv, dw3x3 s2
        m0, m1, m2 = mods[0], mods[1], mods[2]
        pc0 = plan.packed("base.0", lambda: self._stem_pack("base.0", device))
        h, w = pc0.out_hw(H, W)
        t0 = plan.conv(pc0, x4, plan.pool.alloc((N, h, w, pc0.cout)), name="base.0")
        pc1 = plan.packed("base.1", lambda: self._stem_pack("base.1", device))
        t1 = plan.conv(pc1, t0, plan.pool.alloc((N, h, w, pc1.cout)), name="base.1")
        if not full:
            plan.pool.release(t0)
        h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        cur, cur_off = dest_for(3, pc1.cout, h2, w2)
        pack2 = emit_dw(t1, 0, pc1.cout, m2.dwconv, m2.norm, 2, False, cur, cur_off, "base.2")
        if full:
            # train_full: the stem's two outputs stay out of the pool (the autograd node copies them and the staged image after
            # the run); the launches are the same
            plan.stem_record = dict(
                y0=t0, y1=t1, pc0=pc0, pc1=pc1, dw=pack2,
                bn0=plan.packed("base.0.bn", lambda: _bn_stats(m0.norm, pc0.cout, device)),
                bn1=plan.packed("base.1.bn", lambda: _bn_stats(m1.norm, pc1.cout, device)),
                dw_bn=plan.packed("base.2.bn", lambda: _bn_stats(m2.norm, pack2[3], device)))
        else:
            plan.pool.release(t1)
        cur_C = pc1.cout
        h, w = h2, w2

        i = 3
        while i < len(mods):
            m = mods[i]
            if isinstance(m, HarDBlock):
                real, offs, P = m.slice_table()
                assert cur.shape[3] == P and cur_C == real[0]
                buf = cur
                # train_blocks: a block of the section keeps its buffer, its 1x1 outputs and its transition's output out of
                # the pool (the autograd node copies them after the run); the launches are the same
                rec = None
                if section is not None and i >= section:
                    rec = dict(index=i, buf=buf, layers=[], transition=None, down=pending_down)
                    plan.block_records.append(rec)
                pending_down = None

                def pw_record(name, rc, slices, y, y_off, off, bn, dw=None, dw_bn=None):
                    return dict(index=int(name.split(".")[1]), rc=rc, slices=list(slices), segs=[(offs[k], _pad4(real[k])) for k in slices],
                                seg_real=[real[k] for k in slices], cout=rc.cout_real, y=y, y_off=y_off, off=off, dw=dw, dw_bn=dw_bn,
                                bn=plan.packed(name + ".bn", lambda: _bn_stats(bn, rc.cout, device)))
                for li, comb in enumerate(m.layers, start=1):
                    link = m.links[li - 1]
                    segs = [(offs[k], _pad4(real[k])) for k in link]
                    cout, cp = real[li], _pad4(real[li])
                    name = f"base.{i}.layers.{li - 1}.layer1"
                    rc = plan.packed(name, lambda name=name: self._pw_pack(name, device))
                    tmp = plan.pool.alloc((N, h, w, cp))
                    plan.conv(rc, buf, tmp, segs=segs, name=name)
                    pack = emit_dw(tmp, 0, cout, comb.layer2.dwconv, comb.layer2.norm, 1, False, buf, offs[li],
                                   f"base.{i}.layers.{li - 1}.layer2")
                    if rec is not None:
                        rec["layers"].append(pw_record(name, rc, link, tmp, 0, offs[li], comb.layer1.norm, pack, plan.packed(
                            f"base.{i}.layers.{li - 1}.layer2.bn", lambda comb=comb, cp=cp: _bn_stats(comb.layer2.norm, cp, device))))
                    else:
                        plan.pool.release(tmp)
                # transition 1x1 conv gathers the block's output slices (oldest first)
                outs = m.output_slices()
                i += 1
                if isinstance(mods[i], nn.Dropout):
                    i += 1
                tr = mods[i]
                rc = plan.packed(f"base.{i}", lambda name=f"base.{i}": self._pw_pack(name, device))
                dst, dst_off = dest_for(i + 1, rc.cout, h, w)
                if isinstance(mods[i + 1], DWConvLayer):          # "downsample" dw3x3 at stride 1 follows
                    plan.pool.release(dst)
                    dst, dst_off = plan.pool.alloc((N, h, w, rc.cout)), 0
                plan.conv(rc, buf, dst, segs=[(offs[k], _pad4(real[k])) for k in outs], out_off=dst_off, name=f"base.{i}")
                if rec is not None:
                    # (the last block's transition output is the tail's first input: its mask is taken there)
                    last = not any(isinstance(later, HarDBlock) for later in mods[i + 1:])
                    rec["transition"] = pw_record(f"base.{i}", rc, outs, None if last else dst, dst_off, 0, tr.norm)
                else:
                    plan.pool.release(buf)
                cur, cur_off, cur_C = dst, dst_off, rc.cout
                i += 1
            elif isinstance(m, DWConvLayer):
                dst, dst_off = dest_for(i + 1, cur_C, h, w)
                pack = emit_dw(cur, cur_off, cur_C, m.dwconv, m.norm, m.dwconv.stride[0], False, dst, dst_off, f"base.{i}")
                if section is not None and i > section:           # between two blocks of the section: its input stays
                    pending_down = dict(index=i, dw=pack, stride=m.dwconv.stride[0], dw_bn=plan.packed(
                        f"base.{i}.bn", lambda m=m, cp=pack[3]: _bn_stats(m.norm, cp, device)))
                else:
                    plan.pool.release(cur)
                cur, cur_off = dst, dst_off
                i += 1
            elif isinstance(m, nn.Conv2d) and m.groups == m.in_channels and m.kernel_size == (3, 3):
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                s = m.stride[0]
                nh, nw = (h - 1) // s + 1, (w - 1) // s + 1
                dst = plan.pool.alloc((N, nh, nw, _pad4(cur_C)))
                pack = emit_dw(cur, cur_off, cur_C, m, None, s, relu, dst, 0, f"base.{i}")
                if tail:
                    plan.tail_inputs.append((cur, cur_off))
                    plan.tail_packs.append(pack)
                else:
                    plan.pool.release(cur)
                cur, cur_off, h, w = dst, 0, nh, nw
                i += 2 if relu else 1
            elif isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and m.groups == m.out_channels \
                    and m.in_channels == 2 * m.out_channels:
                G = m.out_channels
                wg, bias = plan.packed(f"base.{i}", lambda m=m: self._pair_params(m, device))
                dst = plan.pool.alloc((N, h, w, G))
                plan.call(L.tsod_gconv1x1_pair_amax_f32, ptr(cur), N * h * w, G, cur.shape[3], ptr(wg), ptr(bias), ptr(dst), G,
                          plan.amax_ptr(dst) or None, keep=(cur, dst, wg, bias))
                if tail:
                    plan.tail_inputs.append((cur, cur_off))
                    plan.tail_packs.append((wg, bias))
                else:
                    plan.pool.release(cur)
                cur, cur_off, cur_C = dst, 0, G
                i += 1
            else:
                raise TsodError(f"no HIP lowering for base.{i}: {type(m).__name__}")
        plan.output_nhwc = cur
        plan.output_amax = plan.amax_ptr(cur)
        return plan.finalize()

    def forward(self, x):
        if self._tail_active():
            return self._forward_tail(x, 0, nchw=True)
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
