"""float64 restatement of the backward of ResNet's stem and of the whole-backbone section, with the error
bar of tests/resnet_grads_restated.py: |err| <= (n + 8) 2^-24 T.

    z = scale (*) conv7x7(x, w, stride 2, pad 3) + shift,   y = prelu(z, a),   p = max_pool2d(y, 3, 2, 1)

From dp = d loss / d p, with the saved y:

    dy[oh, ow] = the sum of dp over the windows whose FIRST maximum (ascending (kh, kw), taps outside the image skipped, a strict
                 > to replace) is (oh, ow): at most four windows
    g = dy m(y),  m(y) = (y > 0 ? 1 : a);   d a = sum dy y [y < 0] / a;   conv1.weight, bn1.weight, bn1.bias from g as in every stage

Only the backward is under test: masks and pool winners are taken from the saved y, which holds the very f32 numbers the HIP
forward compared, so neither needs a band.  The linear part is differentiated by torch autograd in float64, once on the values
and once on absolute values (T), by tests/resnet_stage_grads_restated.py's strided stage.  Shared by
tests/test_resnet_stem_grads_abi.py, tests/test_resnet_stem_grads_gpu.py and tests/test_resnet_stem_block_grads.py; plain CPU
torch."""
import torch
import torch.nn.functional as F

from resnet_stage_grads_restated import (assert_within, block_reference, projection_block_reference,  # noqa: F401
                                         strided_stage_reference)

POOL_TERMS = 4                                                    # an element of y lies in at most four windows


def pool_winners(y):
    """y [N,C,OH,OW] -> idx [N,C,PH,PW] int64: the tap 3 kh + kw at which window (ph, pw) (rows 2 ph - 1 .. 2 ph + 1) first
    meets its maximum: the scan starts below every number, a tap replaces the best so far only where it is strictly larger,
    taps outside the image never do."""
    N, C, OH, OW = y.shape
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    yp = F.pad(y.double(), (1, 1, 1, 1), value=float("-inf"))
    best = torch.full((N, C, PH, PW), float("-inf"), dtype=torch.float64)
    idx = torch.zeros((N, C, PH, PW), dtype=torch.int64)
    for kh in range(3):
        for kw in range(3):
            v = yp[:, :, kh:kh + 2 * PH - 1:2, kw:kw + 2 * PW - 1:2]
            take = v > best
            best = torch.where(take, v, best)
            idx = torch.where(take, torch.full_like(idx, 3 * kh + kw), idx)
    return idx


def pool_gather_reference(y, dp, dpT=None):
    """The backward of max_pool2d(y, 3, 2, 1): y [N,C,OH,OW] the saved input, dp [N,C,PH,PW] -> (dy, T, POOL_TERMS)."""
    N, C, OH, OW = y.shape
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    assert tuple(dp.shape) == (N, C, PH, PW), (dp.shape, y.shape)
    idx = pool_winners(y)
    d, dT = dp.double(), (dp.double().abs() if dpT is None else dpT.double())
    out = []
    for val in (d, dT):
        acc = torch.zeros((N, C, OH + 2, OW + 2), dtype=torch.float64)
        for kh in range(3):
            for kw in range(3):
                acc[:, :, kh:kh + 2 * PH - 1:2, kw:kw + 2 * PW - 1:2] += torch.where(idx == 3 * kh + kw, val, torch.zeros_like(val))
        out.append(acc[:, :, 1:OH + 1, 1:OW + 1])
    return out[0], out[1], POOL_TERMS


def prelu_pool_reference(y, dp, a, dpT=None, up=0):
    """tsod_prelu_grad_pool_f32's two results from y and dp (NCHW): {"g": (g, T, n), "dslope_num": (sum, T, n)}."""
    dy, dyT, n = pool_gather_reference(y, dp, dpT)
    y = y.double()
    m = torch.where(y > 0, 1.0, float(a))
    neg = (y < 0).double()
    return {"g": (dy * m, dyT * m, up + n + 1),
            "dslope_num": ((dy * y * neg).sum(), (dyT * y.abs() * neg).sum(), up + n + 1 + int(neg.sum()) + 1)}


def stem_reference(conv, bn, relu, saved, dp, dpT=None, up=0):
    """The stem.  ``conv`` / ``bn`` / ``relu``: conv1, bn1 and the PReLU in float64 on the CPU; ``saved``: dict of the image ``x``
    [N,3,H,W] and the saved ``y`` [N,64,OH,OW] (NCHW); dp = d loss / d (pooled map) with T ``dpT`` (default |dp|) and ``up``
    products behind it.  -> {"conv1.weight" | "bn1.weight" | "bn1.bias" | "relu.weight": (gradient, T, n)}."""
    a = float(relu.weight.detach())
    pr = prelu_pool_reference(saved["y"], dp, a, dpT, up)
    g, gT, up = pr["g"]
    inv = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    mean = bn.running_mean.detach().double()
    st = strided_stage_reference(saved["x"].double(), conv.weight.detach().double(), bn.weight.detach().double() * inv, g,
                                 conv.stride[0], conv.padding[0], gT)
    (dsc, dscT, n_sc), (dsh, dshT, n_sh) = st["dscale"], st["dshift"]
    s, sT, n_s = pr["dslope_num"]
    return {"conv1.weight": (st["dw"][0], st["dw"][1], up + st["dw"][2]),
            "bn1.weight": ((dsc - mean * dsh) * inv, (dscT + mean.abs() * dshT) * inv, up + n_sc + 2),
            "bn1.bias": (dsh, dshT, up + n_sh),
            "relu.weight": ((s / a).reshape(1), (sT / a).reshape(1), n_s)}


def stem_section_reference(stem, blocks, gy):
    """The whole backbone: ``stem`` = (module with conv1 / bn1 / relu in float64, saved dict of x and y) in front of ``blocks``
    ([(prefix, module in float64, saved dict)] in forward order, tests/resnet_stage_grads_restated.py's section); ``gy`` the
    gradient of the last block's output (NCHW).  -> {parameter name: (gradient, T, n)}."""
    ref = {}
    d, dT, up = gy.double(), None, 0
    for prefix, blk, saved in reversed(blocks):
        one = block_reference if blk.downsample is None else projection_block_reference
        out, (d, dT, up) = one(blk, saved, d, dT, up)
        ref.update({f"{prefix}.{k}": v for k, v in out.items()})
    owner, saved = stem
    ref.update(stem_reference(owner.conv1, owner.bn1, owner.relu, saved, d, dT, up))
    return ref


def stem_forward_plain(conv, bn, relu, x):
    """The reference's stem with torch functionals (any dtype) -> (y, pooled)."""
    z = F.batch_norm(F.conv2d(x, conv.weight, None, conv.stride, conv.padding), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                     False, 0.0, bn.eps)
    y = F.prelu(z, relu.weight)
    return y, F.max_pool2d(y, 3, 2, 1)
