"""float64 statements of train-mode BatchNorm with ResNet's epilogue for tests/test_bn_prelu_abi.py and
test_bn_prelu_gpu.py: torch on the CPU, ``F.prelu(F.batch_norm(training=True) + R)`` and its autograd.

The sweep is tests/bn_train_restated.py's, whose inputs it reuses (``case``: z, the output gradient, gamma, beta, the running
statistics): rows M in {2, 3, R - 1, R, R + 1, 3 R + 5}, data of unit scale and data of mean 1e3, and one more channel
configuration, (260, 260): 65 channel quads, so a second blockIdx.y chunk with one live quad.  On top of it:
  the three forms of R   "none", "residual" (a tensor r), "second" (another BatchNorm on z2, with its own gamma2 / beta2)
  two slopes             0.25 (the reference's initial value) and 0.01
Every tensor has its own pitch and a non-zero offset inside NaN-filled rows (LAYOUT): source, residual, destination, saved
output, gradients.

The bound is section 4.20's rule: 4 x the error torch's own float32 CPU evaluation of the same expression shows against the
same float64 values, the largest over the channel configurations and the slopes of a (data, M, form) cell; ``yardstick`` measures
it when a test first asks (nothing is stored).  Errors are bn_train_restated.error's: max |got - ref| / max |ref| over the real
channels, "dz_abs" against the size of dz's terms, max (gamma invstd) x max |g|.

The backward's inputs are the same for all sides: y is the float64 forward rounded to float32, so the mask y > 0 ? 1 : slope is
one and the same in the float64 reference, in torch-f32 and on the GPU (a mask taken from each side's own forward would differ
where a pre-activation rounds across zero, and would show as an error of the size of dy there).  Both torch sides therefore
run autograd through ``torch.where(y > 0, pre, a * pre)`` - F.prelu's expression with the mask given.  The reference's
dslope_num is the entry point's definition, sum dy * y * [y < 0] in float64 on the saved y; torch-f32's is a * (autograd's
slope gradient)."""
import functools

import torch
import torch.nn.functional as F

import bn_train_restated as BT

CHANNELS = BT.CHANNELS + ((260, 260),)
KINDS = BT.KINDS
FORMS = ("none", "residual", "second")
SLOPES = (0.25, 0.01)
EPS, MOMENTUM = BT.EPS, BT.MOMENTUM
MARGIN = BT.MARGIN
QUANTITIES = ("y", "dgamma", "dbeta", "dz", "dz_abs", "dslope")
row_counts = BT.row_counts
# (offset, floats beyond the slice) per tensor; z and dy are bn_train_restated's rows (offset 8, 12 beyond)
LAYOUT = dict(z=(BT.OFF, BT.LD_EXTRA), dy=(BT.OFF, BT.LD_EXTRA), r=(12, 4), z2=(4, 0), y=(4, 4), dz=(12, 8), g=(16, 4))


def rows_of(name, M, C_pad, fill=float("nan")):
    off, extra = LAYOUT[name]
    return torch.full((M, off + C_pad + extra), fill)


def put(name, t, C_pad):
    """``t`` [M, C_real] inside NaN-filled rows of ``name``'s layout, exact zeros at the pad channels"""
    off = LAYOUT[name][0]
    out = rows_of(name, t.shape[0], C_pad)
    out[:, off:off + C_pad] = 0.0
    out[:, off:off + t.shape[1]] = t
    return out


def sl(name, C):
    return slice(LAYOUT[name][0], LAYOUT[name][0] + C)


@functools.lru_cache(maxsize=None)
def case(M, C_real, C_pad, kind):
    """bn_train_restated.case plus the residual r, the second operand z2 (of the data's kind) and its gamma2 / beta2."""
    c = dict(BT.case(M, C_real, C_pad, kind))
    gen = torch.Generator().manual_seed(77000 + 1000 * M + 10 * C_real + KINDS.index(kind))
    c["dy"] = c.pop("g")
    c["r"] = put("r", torch.randn(M, C_real, generator=gen), C_pad)
    c["z2"] = put("z2", torch.randn(M, C_real, generator=gen) * 1.5 + (1e3 if kind == "offset" else 0.0), C_pad)
    c["gamma2"] = torch.rand(C_real, generator=gen) + 0.5
    c["beta2"] = torch.randn(C_real, generator=gen) * 0.3
    return c


def pre_activation(c, form, dtype, z=None, gamma=None, beta=None):
    C = c["C_real"]
    z = c["z"][:, sl("z", C)].to(dtype) if z is None else z
    gamma = c["gamma"].to(dtype) if gamma is None else gamma
    beta = c["beta"].to(dtype) if beta is None else beta
    pre = F.batch_norm(z, None, None, gamma, beta, True, 0.0, EPS)
    if form == "residual":
        pre = pre + c["r"][:, sl("r", C)].to(dtype)
    elif form == "second":
        pre = pre + F.batch_norm(c["z2"][:, sl("z2", C)].to(dtype), None, None, c["gamma2"].to(dtype), c["beta2"].to(dtype), True, 0.0,
                                 EPS)
    return pre


def forward(c, form, slope, dtype):
    return F.prelu(pre_activation(c, form, dtype), torch.tensor([slope], dtype=dtype))


@functools.lru_cache(maxsize=None)
def saved_output(M, C_real, C_pad, kind, form, slope):
    """The backward's y: the float64 forward rounded to float32, [M, C_real]"""
    return forward(case(M, C_real, C_pad, kind), form, float(torch.tensor(slope, dtype=torch.float32)), torch.float64).float()


def backward(c, form, slope, y_saved, dtype):
    """dz, dgamma, dbeta and a * dslope by autograd in ``dtype`` with the mask of ``y_saved``"""
    C = c["C_real"]
    z = c["z"][:, sl("z", C)].to(dtype).clone().requires_grad_()     # (clone: .to() of a float32 tensor is the case's own)
    gamma, beta = c["gamma"].to(dtype).clone().requires_grad_(), c["beta"].to(dtype).clone().requires_grad_()
    a = torch.tensor(slope, dtype=dtype).requires_grad_()             # (the float32 nearest to the slope, as the kernel gets it)
    pre = pre_activation(c, form, dtype, z, gamma, beta)
    out = torch.where(y_saved > 0, pre, a * pre)
    dz, dgamma, dbeta, da = torch.autograd.grad(out, (z, gamma, beta, a), c["dy"][:, sl("dy", C)].to(dtype))
    return dict(dz=dz, dz_abs=dz, dgamma=dgamma, dbeta=dbeta, dslope=(a.detach() * da).reshape(1))


@functools.lru_cache(maxsize=None)
def reference(M, C_real, C_pad, kind, form, slope):
    """Every checked quantity of one run in float64, plus "g" (the masked gradient in float32, exact) and "dz_terms"."""
    c = case(M, C_real, C_pad, kind)
    ys = saved_output(M, C_real, C_pad, kind, form, slope)
    a32 = torch.tensor(slope, dtype=torch.float32)
    dy = c["dy"][:, sl("dy", C_real)]
    out = backward(c, form, float(a32), ys, torch.float64)
    out["y"] = forward(c, form, float(a32), torch.float64)
    out["dslope"] = (dy.double() * ys.double() * (ys < 0)).sum().reshape(1)
    out["g"] = torch.where(ys > 0, dy, a32 * dy)
    z = c["z"][:, sl("z", C_real)].double()
    invstd = 1.0 / torch.sqrt(z.var(0, unbiased=False) + EPS)
    out["dz_terms"] = float((c["gamma"].double() * invstd).abs().max() * out["g"].abs().max())
    return out


def torch_f32(M, C_real, C_pad, kind, form, slope):
    c = case(M, C_real, C_pad, kind)
    out = backward(c, form, slope, saved_output(M, C_real, C_pad, kind, form, slope), torch.float32)
    out["y"] = forward(c, form, slope, torch.float32)
    return out


def error(name, got, ref, terms=None):
    if name == "dslope":
        return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
    return BT.error(name, got, ref, terms)


@functools.lru_cache(maxsize=None)
def yardstick(R, kind, label, form):
    """{quantity: torch-f32's error, largest over CHANNELS and SLOPES} of one (data, M, form) cell"""
    M = row_counts(R)[label]
    cell = dict.fromkeys(QUANTITIES, 0.0)
    for C_real, C_pad in CHANNELS:
        for slope in SLOPES:
            ref, f32 = reference(M, C_real, C_pad, kind, form, slope), torch_f32(M, C_real, C_pad, kind, form, slope)
            for q in QUANTITIES:
                cell[q] = max(cell[q], error(q, f32[q], ref[q], ref["dz_terms"]))
    return cell


def bound(R, kind, label, form, quantity):
    return MARGIN * yardstick(R, kind, label, form)[quantity]
