"""hip_ops.batch_norm_train / batch_norm_train_grad (csrc/bn_train.hip) against float64 on the sweep of
tests/bn_train_restated.py: every quantity within 4 x what torch's own float32 CPU batch_norm shows in the same cell."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_train_restated as R  # noqa: E402

from two_stage_object_detection_amd import _ffi  # noqa: E402

ROWS = R.row_counts(_ffi.BN_ROWS_PER_WORKGROUP)


def run(dev, c, act):
    """One forward + backward of a cell on the GPU, everything at a non-zero offset inside NaN-filled rows."""
    from two_stage_object_detection_amd import hip_ops
    C, cp, ld, M = c["C_real"], c["C_pad"], c["ld"], c["M"]
    z, g = c["z"].to(dev), c["g"].to(dev)
    gamma, beta = c["gamma"].to(dev), c["beta"].to(dev)
    rm, rv = c["running_mean"].to(dev), c["running_var"].to(dev)
    nbt = torch.tensor(7, dtype=torch.int64, device=dev)
    out = torch.full((M, cp + 8), float("nan"), device=dev)
    words = hip_ops.new_amax_words(dev)
    y, mean, invstd = hip_ops.batch_norm_train(z, gamma, beta, R.EPS, R.MOMENTUM, rm, rv, act=act, off=R.OFF, out=out, out_off=4,
                                               C_real=C, num_batches_tracked=nbt, amax_out=words)
    assert y is out
    dz = torch.full((M, cp + 8), float("nan"), device=dev)
    got = hip_ops.batch_norm_train_grad(g, z, mean, invstd, gamma, g_off=R.OFF, z_off=R.OFF, dz=dz, dz_off=4, C_real=C)
    assert got[0] is dz
    return dict(y=out, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, nbt=nbt, dz=dz, dgamma=got[1], dbeta=got[2],
                amax=hip_ops.amax_value(words), z=z, g=g)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("channels", R.CHANNELS, ids=lambda c: f"{c[0]}of{c[1]}")
@pytest.mark.parametrize("label", list(ROWS))
def test_forward_and_backward_against_float64(dev, label, channels, kind):
    M, (C, cp) = ROWS[label], channels
    c, ref = R.case(M, C, cp, kind), R.reference(M, C, cp, kind)
    a, b = run(dev, c, _ffi.ACT_NONE), run(dev, c, _ffi.ACT_RELU6)
    got = dict(mean=a["mean"], invstd=a["invstd"], y=a["y"][:, 4:4 + cp], y_relu6=b["y"][:, 4:4 + cp], running_mean=a["running_mean"],
               running_var=a["running_var"], dgamma=a["dgamma"], dbeta=a["dbeta"], dz=a["dz"][:, 4:4 + cp])
    got["dz_abs"] = got["dz"]
    report, bad = [], []
    for q in R.QUANTITIES:
        t = got[q].cpu()
        real = t[..., :C]
        err, lim = R.error(q, real, ref[q], ref["dz_terms"]), R.bound(kind, label, q)
        report.append(f"{q} {err:.2e}/{lim:.2e}")
        if not err <= lim:
            bad.append(q)
        if q not in ("running_mean", "running_var"):                     # ([C_real] vectors of the module: no pad channels)
            assert t.shape[-1] == cp and bool((t[..., C:] == 0).all()), f"{q}: pad channels must be exact zeros"
    print(f"{kind} M={M} C={C}/{cp}: err/bound " + ", ".join(report))
    assert not bad, (bad, report)
    # nothing outside the slices was touched; the inputs are as they were
    for r in (a, b):
        assert bool(torch.isnan(r["y"][:, :4]).all() and torch.isnan(r["y"][:, 4 + cp:]).all())
        assert bool(torch.isnan(r["dz"][:, :4]).all() and torch.isnan(r["dz"][:, 4 + cp:]).all())
        assert torch.equal(r["z"].cpu().nan_to_num(nan=-7.0), c["z"].nan_to_num(nan=-7.0)) and int(r["nbt"]) == 8
    # the range words hold the abs-max of what was stored
    assert a["amax"] == float(a["y"][:, 4:4 + cp].abs().max()) and b["amax"] == float(b["y"][:, 4:4 + cp].abs().max())
    # a second run gives the same bits
    again = run(dev, c, _ffi.ACT_NONE)
    for k in ("y", "mean", "invstd", "running_mean", "running_var", "dz", "dgamma", "dbeta"):
        assert torch.equal(a[k].nan_to_num(nan=-7.0), again[k].nan_to_num(nan=-7.0)), k


@pytest.mark.gpu
def test_one_row_is_refused(dev):
    from two_stage_object_detection_amd import hip_ops
    z = torch.randn(1, 8, device=dev)
    one = torch.ones(8, device=dev)
    with pytest.raises(ValueError, match="more than one value per channel"):
        hip_ops.batch_norm_train(z, one, one, 1e-5, 0.1)
    with pytest.raises(ValueError):
        hip_ops.batch_norm_train_grad(z, z, one, one, one)


@pytest.mark.gpu
def test_a_tensor_of_many_workgroups_and_256_channel_chunks(dev):
    """More channel quads than one workgroup is wide (two chunks of 64 quads), more partials than one merge run (> 16), default
    arguments (a new output, no running statistics): against float64 at the bound of the (unit, 3R+5) cell."""
    from two_stage_object_detection_amd import hip_ops
    rows, C = 4 * _ffi.BN_ROWS_PER_WORKGROUP + 1, 322               # 5 x rows = 20 R + 5 pixel rows
    gen = torch.Generator().manual_seed(9)
    z, g = torch.randn(5, rows, C + 2, generator=gen), torch.randn(5, rows, C + 2, generator=gen)
    z[..., C:] = 0
    g[..., C:] = 0
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    zd = z[..., :C].double().reshape(-1, C).requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    yr = torch.nn.functional.batch_norm(zd, None, None, gd, bd, True, 0.1, 1e-5)
    ref = dict(zip(("dz", "dgamma", "dbeta"), torch.autograd.grad(yr, (zd, gd, bd), g[..., :C].double().reshape(-1, C))), y=yr.detach())
    y, mean, invstd = hip_ops.batch_norm_train(z.to(dev), gamma.to(dev), beta.to(dev), 1e-5, 0.1)
    dz, dgamma, dbeta = hip_ops.batch_norm_train_grad(g.to(dev), z.to(dev), mean, invstd, gamma.to(dev))
    assert y.shape == z.shape and dz.shape == z.shape and mean.shape == (C + 2,)
    for q, t in (("y", y), ("dz", dz), ("dgamma", dgamma), ("dbeta", dbeta)):
        t = t.cpu().reshape(-1, C + 2) if t.dim() > 1 else t.cpu()
        err = R.error(q, t[..., :C], ref[q])
        print(f"{q}: err {err:.2e} bound {R.bound('unit', '3R+5', q):.2e}")
        assert err <= R.bound("unit", "3R+5", q) and bool((t[..., C:] == 0).all()), q
