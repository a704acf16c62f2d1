"""float64 statements of train-mode BatchNorm for tests/test_bn_train_abi.py, test_bn_train_gpu.py,
test_hardnet_bn_train.py and test_trainer_bn_train.py: torch on the CPU, ``F.batch_norm(training=True)`` and autograd.

The operator sweep: rows M in {2, 3, R - 1, R, R + 1, 3 R + 5} (R = the rows one workgroup reduces, read from the binding),
(C_real, C_pad) in {(4, 4), (10, 12), (68, 68)}, the channels at offset OFF inside rows of LD floats whose other columns are
NaN, data of unit scale ("unit") and data of mean 1e3, standard deviation 1 ("offset": the case a cancelling variance fails).

The yardstick is torch's own float32 CPU batch_norm, forward and backward, against the float64 values on the same inputs;
the bound of a quantity is 4 x the largest error torch-f32 shows for it over the three channel configurations of a
(data, M) cell - the margin is for a different, equally valid summation order.  The error of a tensor is
max |got - ref| / max |ref| over its real channels; for invstd (positive, never near zero) it is the largest elementwise
|got - ref| / ref.  M = 2 and 3 have large dz figures for everybody: there dz is the small difference of O(1) terms (with two
rows the normalised output is +-1 whatever the input, so the true gradient is ~eps / var of its terms); at (offset, M = 2) the
bound exceeds 1 and the "dz" row asserts nothing.  "dz_abs" is what holds those cells: the same dz with its error taken
against the size of its terms, max (gamma invstd) x max |g|, instead of against the cancelled result.

Measured on the CPU with ``measure_yardstick()`` (torch 2.10, R = 128), error of torch-f32 per quantity, largest over M and the
channel configurations, and the bound it gives (the per-cell table the tests use is YARDSTICK below, bound = 4 x entry):

    quantity        unit: torch-f32 err   bound      offset: torch-f32 err   bound
    mean            2.17e-07              8.67e-07   1.46e-07                5.82e-07
    invstd          5.94e-08              2.38e-07   1.39e-07                5.56e-07
    y               3.91e-06              1.56e-05   3.60e-04                1.44e-03
    y_relu6         3.91e-06              1.56e-05   3.62e-04                1.45e-03
    running_mean    7.20e-08              2.88e-07   4.08e-08                1.63e-07
    running_var     4.54e-08              1.81e-07   4.17e-08                1.67e-07
    dgamma          2.95e-06              1.18e-05   8.69e-04                3.48e-03
    dbeta           2.32e-07              9.28e-07   1.51e-07                6.05e-07
    dz              1.52e-03              6.09e-03   1.57e+00                6.26e+00
    dz_abs          1.44e-06              5.77e-06   3.46e-04                1.38e-03

tests/test_bn_train_abi.py re-measures the table on the CPU and fails when YARDSTICK no longer describes torch-f32.

Module level (tests/test_hardnet_bn_train.py): the gradients are held to tests/test_block_grads.py's bar through
``bn_section_reference`` below (the backward from the saved forward).  The 4 x torch-f32 rule is kept for exactly three kinds of
quantity, forward results for which that file has no bar: the train-mode feature map, running_mean and running_var
(``module_oracle``: the whole step in float64 and, for the yardstick, in float32)."""
import functools

import torch
import torch.nn.functional as F

OFF, LD_EXTRA = 8, 12                 # the channels sit at [OFF, OFF + C_pad) of rows of OFF + C_pad + LD_EXTRA floats
CHANNELS = ((4, 4), (10, 12), (68, 68))
KINDS = ("unit", "offset")
EPS, MOMENTUM = 1e-5, 0.1
QUANTITIES = ("mean", "invstd", "y", "y_relu6", "running_mean", "running_var", "dgamma", "dbeta", "dz", "dz_abs")
MARGIN = 4.0


def row_counts(R):
    return {"2": 2, "3": 3, "R-1": R - 1, "R": R, "R+1": R + 1, "3R+5": 3 * R + 5}


@functools.lru_cache(maxsize=None)
def case(M, C_real, C_pad, kind):
    """The inputs of one cell (f32, CPU): z / g [M, LD] with NaN outside the slice and exact zeros at its pad channels, gamma,
    beta, running_mean, running_var [C_real]."""
    gen = torch.Generator().manual_seed(1000 * M + 10 * C_real + KINDS.index(kind))
    ld = OFF + C_pad + LD_EXTRA

    def rows(mean):
        t = torch.full((M, ld), float("nan"))
        t[:, OFF:OFF + C_pad] = 0.0
        t[:, OFF:OFF + C_real] = torch.randn(M, C_real, generator=gen) + mean
        return t
    z = rows(1e3 if kind == "offset" else 0.0)
    g = rows(0.0)
    gamma = torch.rand(C_real, generator=gen) + 0.5
    beta = torch.randn(C_real, generator=gen) * 0.3
    rm = torch.randn(C_real, generator=gen) * 0.2 + (1e3 if kind == "offset" else 0.0)
    rv = torch.rand(C_real, generator=gen) + 0.5
    return dict(M=M, C_real=C_real, C_pad=C_pad, ld=ld, z=z, g=g, gamma=gamma, beta=beta, running_mean=rm, running_var=rv)


def torch_batch_norm(c, dtype):
    """Every checked quantity of a cell from torch's CPU batch_norm and autograd in ``dtype``."""
    sl = slice(OFF, OFF + c["C_real"])
    z = c["z"][:, sl].to(dtype).requires_grad_()
    gamma, beta = c["gamma"].to(dtype).requires_grad_(), c["beta"].to(dtype).requires_grad_()
    rm, rv = c["running_mean"].to(dtype).clone(), c["running_var"].to(dtype).clone()
    y = F.batch_norm(z, rm, rv, gamma, beta, True, MOMENTUM, EPS)
    dz, dgamma, dbeta = torch.autograd.grad(y, (z, gamma, beta), c["g"][:, sl].to(dtype))
    zd = z.detach()
    mean = zd.mean(0)
    var = ((zd - mean) ** 2).mean(0)
    out = dict(y=y.detach(), y_relu6=F.hardtanh(y.detach(), 0.0, 6.0), running_mean=rm, running_var=rv, dgamma=dgamma, dbeta=dbeta,
               dz=dz, dz_abs=dz)
    if dtype == torch.float64:
        out.update(mean=mean, invstd=1.0 / torch.sqrt(var + EPS))
        out["dz_terms"] = float((gamma.detach() * out["invstd"]).abs().max() * c["g"][:, sl].abs().max())
    else:                                             # what torch itself saves for its backward
        saved = torch.native_batch_norm(zd, gamma.detach(), beta.detach(), rm.clone(), rv.clone(), True, MOMENTUM, EPS)
        out.update(mean=saved[1], invstd=saved[2])
    return out


@functools.lru_cache(maxsize=None)
def reference(M, C_real, C_pad, kind):
    return torch_batch_norm(case(M, C_real, C_pad, kind), torch.float64)


def error(name, got, ref, terms=None):
    """``terms``: the reference's "dz_terms" (for "dz_abs")"""
    got, ref = got.double(), ref.double()
    if name == "invstd":
        return float(((got - ref).abs() / ref).max())
    if name == "dz_abs":
        return float((got - ref).abs().max()) / terms
    return float((got - ref).abs().max() / ref.abs().max())


def measure_yardstick(R):
    """{(kind, M label): {quantity: torch-f32's error, largest over CHANNELS}}"""
    table = {}
    for kind in KINDS:
        for label, M in row_counts(R).items():
            cell = dict.fromkeys(QUANTITIES, 0.0)
            for C_real, C_pad in CHANNELS:
                ref, f32 = reference(M, C_real, C_pad, kind), torch_batch_norm(case(M, C_real, C_pad, kind), torch.float32)
                for q in QUANTITIES:
                    cell[q] = max(cell[q], error(q, f32[q], ref[q], ref["dz_terms"]))
            table[(kind, label)] = cell
    return table


def bound(kind, label, quantity):
    return MARGIN * YARDSTICK[(kind, label)][quantity]


# torch-f32's error per (data, M) cell, QUANTITIES order; measured with measure_yardstick(128)
YARDSTICK = {
    ('unit', '2'): (5.454e-08, 5.121e-08, 3.906e-06, 3.906e-06, 3.857e-08, 3.322e-08, 2.952e-06, 3.361e-08, 1.522e-03, 1.443e-06),
    ('unit', '3'): (6.120e-08, 5.034e-08, 1.433e-07, 1.031e-07, 7.201e-08, 4.536e-08, 1.471e-07, 4.559e-08, 2.741e-07, 1.121e-07),
    ('unit', 'R-1'): (1.786e-07, 5.938e-08, 1.137e-07, 9.551e-08, 2.782e-08, 4.183e-08, 7.555e-08, 1.313e-07, 1.148e-07, 9.215e-08),
    ('unit', 'R'): (2.167e-07, 5.827e-08, 1.228e-07, 7.992e-08, 5.083e-08, 4.169e-08, 6.606e-08, 1.393e-07, 1.067e-07, 8.865e-08),
    ('unit', 'R+1'): (1.522e-07, 5.350e-08, 9.961e-08, 9.961e-08, 2.437e-08, 3.878e-08, 7.877e-08, 1.522e-07, 1.077e-07, 1.062e-07),
    ('unit', '3R+5'): (1.178e-07, 5.577e-08, 1.304e-07, 1.309e-07, 3.590e-08, 3.839e-08, 6.439e-08, 2.321e-07, 1.129e-07, 1.077e-07),
    ('offset', '2'): (3.051e-08, 1.389e-07, 3.603e-04, 3.622e-04, 3.355e-08, 3.605e-08, 5.292e-04, 3.490e-08, 1.566e+00, 1.903e-04),
    ('offset', '3'): (8.132e-08, 1.142e-07, 2.460e-04, 2.694e-04, 3.458e-08, 3.365e-08, 8.691e-04, 4.579e-08, 9.437e-04, 3.461e-04),
    ('offset', 'R-1'): (1.456e-07, 5.585e-08, 2.783e-05, 3.248e-05, 3.963e-08, 4.053e-08, 1.014e-04, 9.681e-08, 1.818e-05, 1.203e-05),
    ('offset', 'R'): (1.173e-07, 5.923e-08, 3.005e-05, 3.806e-05, 4.080e-08, 4.172e-08, 7.818e-05, 1.273e-07, 6.681e-06, 4.885e-06),
    ('offset', 'R+1'): (1.145e-07, 6.100e-08, 2.687e-05, 2.895e-05, 3.898e-08, 4.090e-08, 1.061e-04, 1.235e-07, 9.467e-06, 8.055e-06),
    ('offset', '3R+5'): (1.133e-07, 5.402e-08, 3.099e-05, 3.097e-05, 3.965e-08, 4.107e-08, 1.005e-04, 1.511e-07, 7.886e-06, 7.373e-06),
}
YARDSTICK = {k: dict(zip(QUANTITIES, v)) for k, v in YARDSTICK.items()}


# ---------------------------------------------------------------------------------------------------- the module-level oracle
def plain_forward(base, x):
    """The reference's HarDNetFeatureExtraction.forward with the repo's modules called as torch modules (any dtype, CPU)."""
    from pw_grads_restated import block_forward_plain
    from two_stage_object_detection_amd.models.hardnet import HarDBlock
    mods, i = list(base), 0
    while i < len(mods):
        if isinstance(mods[i], HarDBlock):
            x = block_forward_plain(mods[i], mods[i + 1], x)[0]
            i += 2
        else:
            x = mods[i](x)
            i += 1
    return x


def module_oracle(model, start, x, gy, dtype, buffers=None):
    """One training step of ``model.base`` (a copy, on the CPU in ``dtype``) as torch runs it: the modules from ``base[start]`` on
    in .train() (batch statistics, running updates), everything below in .eval(), every dropout at p = 0 -> (feature map,
    {parameter name: gradient} of the section, {buffer name: value after the forward} of every BatchNorm, the copy).  ``buffers``: BatchNorm buffers to start from instead
    of the model's present ones."""
    import copy
    base = copy.deepcopy(model.base).cpu().eval()
    with torch.no_grad():
        for k, t in base.named_buffers():                      # (``buffers``: the state the step under test started from)
            if buffers is not None and f"base.{k}" in buffers:
                t.copy_(buffers[f"base.{k}"])
    base = base.to(dtype)
    for mod in base.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for mod in list(base)[start:]:
        mod.train()
    params = {f"base.{k}": p for k, p in base.named_parameters() if int(k.split(".")[0]) >= start}
    for p in params.values():
        p.requires_grad_(True)
    out = plain_forward(base, x.cpu().to(dtype))
    grads = torch.autograd.grad(out, list(params.values()), gy.cpu().to(dtype))
    buffers = {f"base.{k}": b.detach().clone() for k, b in base.named_buffers()}
    return out.detach(), dict(zip(params, grads)), buffers, base


def norm_error(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------ the backward from the saved forward, with its bar
class _AbsBatchNorm(torch.autograd.Function):
    """The majorant of a batch-statistics BatchNorm's backward: every term of dz = k (g - mean g - xhat mean(g xhat)), dgamma =
    sum g xhat, dbeta = sum g with its absolute value (``xhat`` = |xhat|, ``k`` = |gamma| invstd, the incoming g >= 0)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, xhat, k):
        ctx.save_for_backward(xhat, k)
        return z * k.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        xhat, k = ctx.saved_tensors
        d = (0, 2, 3)
        dz = k.view(1, -1, 1, 1) * (g + g.mean(d, keepdim=True) + xhat * (g * xhat).mean(d, keepdim=True))
        return dz, (g * xhat).sum(d), g.sum(d), None, None


def bn_section_reference(section, tail, x_in, gy, tail_mask=None, stem=None):
    """tests/pw_grads_restated.py's ``section_reference`` for a section whose BatchNorms ran on batch statistics: float64 autograd
    of the same graph in which every conv output is replaced, straight-through, by the raw ``z`` the HIP run saved and every layer
    output by the saved output, so that only the backward is under test - F.batch_norm(training=True) on the saved z, the ReLU6
    mask from the saved output - and T from the same graph on absolute values with ``_AbsBatchNorm`` for the BatchNorm.
    ``section`` as there plus, per block, ``zs`` (the saved raw 1x1 outputs), ``dw_zs`` (the saved raw depthwise outputs),
    ``tr_z`` and ``down_z``; ``stem``: None or dict ``mods`` (base.0, base.1, base.2), ``y0`` / ``z0``, ``y1`` / ``z1``, ``z2``
    (``x_in`` is then the image and the first block's slice 0 the stem's saved output).
    -> {parameter name: (gradient, T, n)}.  n is ``section_reference``'s count along the deepest path plus, for every BatchNorm
    from the parameter's own layer to the output, its pixels + 3 (the two means over the pixels that enter every dz)."""
    from pw_grads_restated import TAIL_N, _upstream_counts
    pixels, order = {}, []                                  # pixels per layer, layers with a BatchNorm in forward order

    def run(absval):
        P = {}
        f = (lambda t: t.detach().double().abs()) if absval else (lambda t: t.detach().double())

        def leaf(name, t):
            P[name] = f(t).clone().requires_grad_()
            return P[name]

        def st(v, hip):
            return v + (f(hip) - v).detach()

        def bn(z, prefix, norm, z_hip):
            z = st(z, z_hip)
            gamma, beta = leaf(prefix + ".weight", norm.weight), leaf(prefix + ".bias", norm.bias)
            if not absval:
                return F.batch_norm(z, None, None, gamma, beta, True, 0.0, norm.eps)
            zh = z_hip.detach().double()
            d = (0, 2, 3)
            inv = 1.0 / torch.sqrt(zh.var(d, unbiased=False, keepdim=True) + norm.eps)
            xhat = ((zh - zh.mean(d, keepdim=True)) * inv).abs()
            return _AbsBatchNorm.apply(z, gamma, beta, xhat, norm.weight.detach().double().abs() * inv.reshape(-1))

        def conv_layer(x, prefix, m, y_hip, z_hip):
            z = F.conv2d(x, leaf(prefix + ".conv.weight", m.conv.weight), None, m.conv.stride, m.conv.padding)
            yh = y_hip.detach().double()
            pixels[prefix] = z.shape[0] * z.shape[2] * z.shape[3]
            if not absval:
                order.append(prefix)
            return st(bn(z, prefix + ".norm", m.norm, z_hip) * ((yh > 0) & (yh < 6)).double(), y_hip)

        def dw_layer(x, prefix, m, hip, z_hip):
            z = F.conv2d(x, leaf(prefix + ".dwconv.weight", m.dwconv.weight), None, m.dwconv.stride, 1, groups=x.shape[1])
            pixels[prefix] = z.shape[0] * z.shape[2] * z.shape[3]
            if not absval:
                order.append(prefix)
            return st(bn(z, prefix + ".norm", m.norm, z_hip), hip)

        x = f(x_in)
        if stem is not None:
            m0, m1, m2 = stem["mods"]
            x = conv_layer(x, "base.0", m0, stem["y0"], stem["z0"])
            x = conv_layer(x, "base.1", m1, stem["y1"], stem["z1"])
            x = dw_layer(x, "base.2", m2, section[0]["slices"][0], stem["z2"])
        for b in section:
            if b.get("down") is not None:
                x = dw_layer(x, f"base.{b['down_index']}", b["down"], b["slices"][0], b["down_z"])
            blk, layers_ = b["block"], [x]
            for li, comb in enumerate(blk.layers, start=1):
                tin = torch.cat([layers_[k] for k in blk.links[li - 1]], 1)
                prefix = f"base.{b['index']}.layers.{li - 1}"
                y = conv_layer(tin, prefix + ".layer1", comb.layer1, b["ys"][li - 1], b["zs"][li - 1])
                layers_.append(dw_layer(y, prefix + ".layer2", comb.layer2, b["slices"][li], b["dw_zs"][li - 1]))
            x = conv_layer(torch.cat([layers_[k] for k in blk.output_slices()], 1), f"base.{b['tr_index']}", b["transition"],
                           b["tr_y"], b["tr_z"])
        if tail is not None:
            i1, c1, i2, c2, ip, pair = tail
            C = x.shape[1]
            y1 = F.conv2d(x, leaf(f"base.{i1}.weight", c1.weight), leaf(f"base.{i1}.bias", c1.bias), 2, 1, groups=C)
            bb = F.conv2d(y1 * tail_mask.double(), leaf(f"base.{i2}.weight", c2.weight), leaf(f"base.{i2}.bias", c2.bias), 2, 1, groups=C)
            x = F.conv2d(bb, leaf(f"base.{ip}.weight", pair.weight), leaf(f"base.{ip}.bias", pair.bias), groups=pair.out_channels)
        names = list(P)
        return names, torch.autograd.grad(x, [P[k] for k in names], f(gy))

    names, grads = run(False)
    _, Ts = run(True)
    n = {}
    up = TAIL_N if tail is not None else 0
    for b in reversed(section):
        blk = b["block"]
        up_slice, up_g = _upstream_counts(blk, up, b["transition"].conv.out_channels)
        tr = f"base.{b['tr_index']}"
        n[tr + ".conv.weight"] = n[tr + ".norm.bias"] = up + pixels[tr]
        n[tr + ".norm.weight"] = up + pixels[tr] + b["transition"].conv.in_channels
        for li, comb in enumerate(blk.layers, start=1):
            p1, p2 = f"base.{b['index']}.layers.{li - 1}.layer1", f"base.{b['index']}.layers.{li - 1}.layer2"
            n[p2 + ".dwconv.weight"] = n[p2 + ".norm.bias"] = up_slice[li] + pixels[p2]
            n[p2 + ".norm.weight"] = up_slice[li] + pixels[p2] + 9
            n[p1 + ".conv.weight"] = n[p1 + ".norm.bias"] = up_g[li] + pixels[p1]
            n[p1 + ".norm.weight"] = up_g[li] + pixels[p1] + comb.layer1.conv.in_channels
        up = up_slice[0]
        if b.get("down") is not None:
            d = f"base.{b['down_index']}"
            n[d + ".dwconv.weight"] = n[d + ".norm.bias"] = up + pixels[d]
            n[d + ".norm.weight"] = up + pixels[d] + 9
            up += 9
    if stem is not None:
        m0, m1, _ = stem["mods"]
        n["base.2.dwconv.weight"] = n["base.2.norm.bias"] = up + pixels["base.2"]
        n["base.2.norm.weight"] = up + pixels["base.2"] + 9
        up += 9
        n["base.1.conv.weight"] = n["base.1.norm.bias"] = up + pixels["base.1"]
        n["base.1.norm.weight"] = up + pixels["base.1"] + m1.conv.in_channels
        up += m1.conv.out_channels
        n["base.0.conv.weight"] = n["base.0.norm.bias"] = up + pixels["base.0"]
        n["base.0.norm.weight"] = up + pixels["base.0"] + 27
    if tail is not None:
        big = max(pixels.values())
        for k in names:
            n.setdefault(k, big + 9)
    # the BatchNorms between a parameter's layer and the output: pixels + 3 terms each
    after = 0
    extra = {}
    for prefix in reversed(order):
        after += pixels[prefix] + 3
        extra[prefix] = after
    for k in names:
        layer = k.rsplit(".", 2)[0]
        n[k] += extra.get(layer, 0)
    return {k: (g, T, n[k]) for k, g, T in zip(names, grads, Ts)}
