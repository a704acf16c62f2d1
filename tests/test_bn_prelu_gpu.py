"""hip_ops.batch_norm_prelu_train / batch_norm_prelu_train_grad (csrc/bn_train.hip) against float64
on the sweep of tests/bn_prelu_restated.py: every quantity within 4 x what torch's own float32 CPU evaluation of the same
expression shows in the same (data, M, form) cell; no cell is skipped."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_prelu_restated as R  # noqa: E402
from resnet_grads_restated import assert_within, prelu_reference  # noqa: E402

from two_stage_object_detection_amd import _ffi  # noqa: E402

RW = _ffi.BN_ROWS_PER_WORKGROUP
ROWS = R.row_counts(RW)
NAN = -7.0


def _nn(t):
    return t.nan_to_num(nan=NAN)


def run(dev, c, form, slope, y_saved):
    """One forward and one backward of a cell on the GPU, every tensor on its own pitch at a non-zero offset inside NaN-filled
    rows; the backward takes ``y_saved`` (not the forward's own output)."""
    from two_stage_object_detection_amd import hip_ops
    C, cp, M = c["C_real"], c["C_pad"], c["M"]
    z, dy = c["z"].to(dev), c["dy"].to(dev)
    gamma, beta = c["gamma"].to(dev), c["beta"].to(dev)
    rm, rv = c["running_mean"].to(dev), c["running_var"].to(dev)
    nbt = torch.tensor(7, dtype=torch.int64, device=dev)
    kw = {}
    if form == "residual":
        kw = dict(residual=c["r"].to(dev), residual_off=R.LAYOUT["r"][0])
    elif form == "second":
        z2 = c["z2"].to(dev)
        _, _, scale2, shift2 = hip_ops.batch_norm_stats(z2, c["gamma2"].to(dev), c["beta2"].to(dev), R.EPS, R.MOMENTUM,
                                                        off=R.LAYOUT["z2"][0], C_real=C)
        kw = dict(second=(z2, scale2, shift2, R.LAYOUT["z2"][0]))
    out = R.rows_of("y", M, cp).to(dev)
    words = hip_ops.new_amax_words(dev)
    y, mean, invstd = hip_ops.batch_norm_prelu_train(z, gamma, beta, R.EPS, R.MOMENTUM, slope, rm, rv, off=R.LAYOUT["z"][0], out=out,
                                                     out_off=R.LAYOUT["y"][0], C_real=C, num_batches_tracked=nbt, amax_out=words, **kw)
    assert y is out
    ys = R.put("y", y_saved, cp).to(dev)
    dz, g = R.rows_of("dz", M, cp).to(dev), R.rows_of("g", M, cp).to(dev)
    got = hip_ops.batch_norm_prelu_train_grad(ys, dy, z, mean, invstd, gamma, slope, y_off=R.LAYOUT["y"][0], dy_off=R.LAYOUT["dy"][0],
                                              z_off=R.LAYOUT["z"][0], dz=dz, dz_off=R.LAYOUT["dz"][0], C_real=C, g=g,
                                              g_off=R.LAYOUT["g"][0])
    assert got[0] is dz and got[4] is g
    # the pair it replaces, on the same inputs
    gp, nump = hip_ops.prelu_grad(ys[:, R.sl("y", cp)].contiguous(), dy, slope, dy_off=R.LAYOUT["dy"][0])
    pair = hip_ops.batch_norm_train_grad(gp, z, mean, invstd, gamma, z_off=R.LAYOUT["z"][0], C_real=C)
    return dict(y=out, mean=mean, invstd=invstd, nbt=nbt, dz=dz, dgamma=got[1], dbeta=got[2], dslope=got[3], g=g,
                amax=hip_ops.amax_value(words), z=z, ys=ys, dy=dy,
                pair=dict(dz=pair[0], dz_abs=pair[0], dgamma=pair[1], dbeta=pair[2], dslope=nump, g=gp))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("channels", R.CHANNELS, ids=lambda c: f"{c[0]}of{c[1]}")
@pytest.mark.parametrize("label", list(ROWS))
def test_forward_and_backward_against_float64(dev, label, channels, kind):
    M, (C, cp) = ROWS[label], channels
    c = R.case(M, C, cp, kind)
    bad = []
    for form in R.FORMS:
        for slope in R.SLOPES:
            ref, ys = R.reference(M, C, cp, kind, form, slope), R.saved_output(M, C, cp, kind, form, slope)
            a = run(dev, c, form, slope, ys)
            got = {q: a[q if q != "dz_abs" else "dz"] for q in R.QUANTITIES}
            report = []
            for q in R.QUANTITIES:
                t = got[q].cpu()
                name = {"dz_abs": "dz"}.get(q, q)
                if t.dim() == 2:                                          # rows: the slice, nothing outside it touched
                    whole, t = t, t[:, R.sl(name, cp)]
                    assert bool(torch.isnan(whole[:, :R.LAYOUT[name][0]]).all() and
                                torch.isnan(whole[:, R.LAYOUT[name][0] + cp:]).all()), f"{q}: written outside its slice"
                err, lim = R.error(q, t[..., :C], ref[q], ref["dz_terms"]), R.bound(RW, kind, label, form, q)
                report.append(f"{q} {err:.2e}/{lim:.2e}")
                if not err <= lim:
                    bad.append((form, slope, q, err, lim))
                if q != "dslope":
                    assert t.shape[-1] == cp and bool((t[..., C:] == 0).all()), f"{q}: pad channels must be exact zeros"
                # the fused backward against prelu_grad + batch_norm_train_grad on the same inputs: within the sum of the two
                # sides' bounds - batch_norm_train_grad's is this cell's (section 4.20's rule), prelu_grad's float32 slope sum has
                # tests/test_resnet_grads_gpu.py's: (terms + 9) 2^-24 sum |dy y| [y < 0]
                if q != "y":
                    p = a["pair"][q].cpu()
                    p = p if q == "dslope" else p[..., :C]
                    scale = ref["dz_terms"] if q == "dz_abs" else float(ref[q].double().abs().max())
                    diff = float((t[..., :C].double() - p.double()).abs().max()) / scale
                    other = lim
                    if q == "dslope":
                        _, T, n = prelu_reference(ys, c["dy"][:, R.sl("dy", C)], slope)["dslope_num"]
                        other = (n + 8) * 2.0 ** -24 * float(T) / scale
                    report.append(f"(pair {diff:.1e}/{lim + other:.1e})")
                    if not diff <= lim + other:
                        bad.append((form, slope, q + " vs pair", diff, lim + other))
            print(f"{kind} M={M} C={C}/{cp} {form} a={slope}: err/bound " + ", ".join(report))
            # g is one float32 product: exact, and the pair's bits
            g = a["g"].cpu()[:, R.sl("g", cp)]
            assert torch.equal(g[:, :C], ref["g"]) and bool((g[:, C:] == 0).all()) and torch.equal(g[:, :C], a["pair"]["g"].cpu()[:, :C])
            # the inputs are as they were, the batch counter moved once, the range words hold the abs-max of what was stored
            assert torch.equal(_nn(a["z"].cpu()), _nn(c["z"])) and torch.equal(_nn(a["dy"].cpu()), _nn(c["dy"])) and int(a["nbt"]) == 8
            assert a["amax"] == float(a["y"][:, R.sl("y", cp)].abs().max())
            # a second run gives the same bits
            again = run(dev, c, form, slope, ys)
            for k in ("y", "mean", "invstd", "dz", "dgamma", "dbeta", "dslope", "g"):
                assert torch.equal(_nn(a[k]), _nn(again[k])), (form, slope, k)
    assert not bad, bad


@pytest.mark.gpu
def test_optional_outputs_and_refusals(dev):
    """Without g and without the slope's sum the other outputs keep their bits; one row, and r with z2, are refused."""
    from two_stage_object_detection_amd import hip_ops
    gen = torch.Generator().manual_seed(3)
    M, C = RW + 3, 260
    z, dy, r = (torch.randn(M, C, generator=gen).to(dev) for _ in range(3))
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(dev), torch.randn(C, generator=gen).to(dev)
    y, mean, invstd = hip_ops.batch_norm_prelu_train(z, gamma, beta, 1e-5, 0.1, 0.25, residual=r)
    full = hip_ops.batch_norm_prelu_train_grad(y, dy, z, mean, invstd, gamma, 0.25, want_g=True)
    lean = hip_ops.batch_norm_prelu_train_grad(y, dy, z, mean, invstd, gamma, 0.25, want_dslope=False)
    assert lean[3] is None and lean[4] is None and full[4].shape == y.shape
    for a, b in zip(full[:3], lean[:3]):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="more than one value per channel"):
        hip_ops.batch_norm_prelu_train(z[:1], gamma, beta, 1e-5, 0.1, 0.25)
    with pytest.raises(ValueError):
        hip_ops.batch_norm_prelu_train_grad(y[:1], dy[:1], z[:1], mean, invstd, gamma, 0.25)
    _, _, sc, sh = hip_ops.batch_norm_stats(z, gamma, beta, 1e-5, 0.1)
    with pytest.raises(ValueError, match="not both"):
        hip_ops.batch_norm_prelu_train(z, gamma, beta, 1e-5, 0.1, 0.25, residual=r, second=(z, sc, sh, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("M,C,cp", [(3, 10, 12), (RW + 1, 68, 68), (3 * RW + 5, 258, 260)], ids=lambda v: str(v))
def test_slope_one_is_the_plain_path_bit_for_bit(dev, M, C, cp):
    """One kernel family: at slope 1 the PReLU forward is ``batch_norm_train(act=ACT_NONE)`` and the
    backward from the saved output is ``batch_norm_train_grad`` on dy, in every bit; the slope's sum is the float64 one within
    tests/test_resnet_grads_gpu.py's bound.  Cells: one workgroup with pad channels and fewer rows than row lanes; a one-row
    second workgroup; two chunks of 64 quads with pad channels in the last quad.  z sits 50 off zero per channel, so scale * z
    and shift cancel."""
    from two_stage_object_detection_amd import hip_ops
    gen = torch.Generator().manual_seed(1000 * M + C)
    z = torch.randn(M, cp, generator=gen) + 50.0 * (1 + torch.arange(cp) % 3)
    y, dy = torch.randn(M, cp, generator=gen), torch.randn(M, cp, generator=gen)
    y[torch.rand(M, cp, generator=gen) < 0.1] = 0.0
    assert bool((y > 0).any() and (y < 0).any() and (y == 0).any())
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    z, y, dy, gamma, beta = (t.to(dev) for t in (z, y, dy, gamma, beta))
    fwd = []
    for f, extra in ((hip_ops.batch_norm_prelu_train, (1.0,)), (hip_ops.batch_norm_train, ())):
        rm, rv, words = torch.zeros(C, device=dev), torch.ones(C, device=dev), hip_ops.new_amax_words(dev)
        kw = dict(act=hip_ops.ACT_NONE) if not extra else {}
        out = f(z, gamma, beta, 1e-5, 0.1, *extra, rm, rv, C_real=C, amax_out=words, **kw)
        fwd.append(out + (rm, rv, torch.tensor(hip_ops.amax_value(words))))
    for name, a, b in zip(("y", "mean", "invstd", "running_mean", "running_var", "range word"), *fwd):
        assert torch.equal(a, b), name
    mean, invstd = fwd[0][1:3]
    fused = hip_ops.batch_norm_prelu_train_grad(y, dy, z, mean, invstd, gamma, 1.0, C_real=C)
    plain = hip_ops.batch_norm_train_grad(dy, z, mean, invstd, gamma, C_real=C)
    for name, a, b in zip(("dz", "dgamma", "dbeta"), fused, plain):
        assert torch.equal(a, b), name
    num, T, n = prelu_reference(y[:, :C].cpu(), dy[:, :C].cpu(), 1.0)["dslope_num"]
    assert_within(fused[3], num.reshape(1), T.reshape(1), n, f"slope sum {M}x{C}")
