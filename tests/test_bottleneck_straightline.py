"""tsod_bottleneck_fp16x2 after its wave ownership became compile-time: the one-launch bottleneck against the
f64 CPU block at the smallest shapes that reach every tile pipeline, with the bars of test_hip_ops.py's two bottleneck tests.

* one tile of 8 rows (1 x 8 x 16) and a ragged 2 x 2 tiling (1 x 11 x 17): the 8-row kernel, whose four waves run ONE pipeline
  (3 + 3 halo blocks, 2 + 2 tile blocks), with partial tiles on both edges;
* a shape at which the launcher's rule really picks 10 rows: the 8-row tiling needs more than one round of the device (two
  workgroups per CU), the 10-row tiling fits in one.  There waves 0, 1 run the 4 / 3-block pipeline and waves 2, 3 the 3 / 2-block
  one, chosen by one scalar branch.  The width follows from the device's CU count.
Each with the identity shortcut and with the projection shortcut (stacked-K conv3).

The bar here is one max-norm tolerance per tensor; tests/test_fused_kernels_gpu.py holds the same kernels to a per-element bound
derived in tests/fused_restated.py, at every geometry, pitch, BatchNorm sign, slope and scale switch."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SLOPE = 0.25


@pytest.fixture(scope="module")
def ops():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops


def _act(t):
    return torch.where(t >= 0, t, SLOPE * t)


def _v4(v):
    return v.double().view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def _block(H, W, Cin, Cout):
    """Inputs, weights and the f64 outputs (identity where Cout == Cin, and projection) of one block; computed once per shape."""
    g = torch.Generator().manual_seed(4321 + H)
    x = torch.randn(1, Cin, H, W, generator=g)
    x = torch.maximum(x, 0.25 * x)
    w1 = torch.randn(64, Cin, 1, 1, generator=g) / math.sqrt(Cin)
    w2 = torch.randn(64, 64, 3, 3, generator=g) / math.sqrt(576)
    w3 = torch.randn(Cout, 64, 1, 1, generator=g) / 8.0
    wd = torch.randn(Cout, Cin, 1, 1, generator=g) / math.sqrt(Cin)
    bn = [torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5,
          torch.randn(64, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1]
    sd, bd = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    y = _act(F.conv2d(x.double(), w1.double()) * _v4(bn[0]) + _v4(bn[1]))
    y = _act(F.conv2d(y, w2.double(), padding=1) * _v4(bn[2]) + _v4(bn[3]))
    main = F.conv2d(y, w3.double()) * _v4(bn[4]) + _v4(bn[5])
    ref_id = _act(main + x.double()).float() if Cout == Cin else None
    ref_proj = _act(main + F.conv2d(x.double(), wd.double()) * _v4(sd) + _v4(bd)).float()
    return dict(x=x, w1=w1, w2=w2, w3=w3, wd=wd, bn=bn, sd=sd, bd=bd, ref_id=ref_id, ref_proj=ref_proj)


def _run(ops, dev, H, W, Cin, Cout, projection):
    b = _block(H, W, Cin, Cout)
    bn = b["bn"]
    xn = ops.nchw_to_nhwc(b["x"].to(dev))
    w2p = ops.pack_conv_weight(b["w2"].to(dev))
    if projection:
        stacked = torch.cat([b["w3"].double().flatten(1) * bn[4].double().view(-1, 1),
                             b["wd"].double().flatten(1) * b["sd"].double().view(-1, 1)], dim=1).float()
        stream, exps = ops.pack_bottleneck_wstream(b["w1"].view(64, Cin).to(dev), w2p, stacked.to(dev), projection=True)
        bnv = torch.cat(bn[:4] + [torch.ones(Cout), (bn[5].double() + b["bd"].double()).float()]).to(dev)
        ref = b["ref_proj"]
    else:
        stream, exps = ops.pack_bottleneck_wstream(b["w1"].view(64, Cin).to(dev), w2p, b["w3"].view(Cout, 64).to(dev))
        bnv = torch.cat(bn).to(dev)
        ref = b["ref_id"]
    words = ops.absmax(xn, ops.new_amax_words(dev, 1))
    wout = ops.new_amax_words(dev, 1)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = dict(cin=Cin) if projection else {}
    out = ops.bottleneck_fused(xn, stream, exps, bnv, Cout, SLOPE, amax_in=words, amax_out=wout, range_flag=flag, **kw)
    got = ops.nhwc_to_nchw(out).cpu()
    tol = (3e-6 * math.sqrt(576) + 1e-5) * float(ref.abs().max()) / 4.0 + 1e-6
    err = (got - ref).abs().max().item()
    print(f"H={H} W={W} Cin={Cin} Cout={Cout} projection={projection}: max |err| {err:.3e} (bar {tol:.3e})")
    assert err <= tol, (err, tol)
    assert int(flag.item()) == 0
    assert ops.amax_value(wout) == float(out.abs().max())
    # a non-finite value in the LAST pixel (the last pixel block of the last tile) must be reported
    xb = xn.clone()
    xb[0, H - 1, W - 1, 3] = float("nan")
    ops.bottleneck_fused(xb, stream, exps, bnv, Cout, SLOPE, amax_in=ops.absmax(xb, ops.new_amax_words(dev, 1)), range_flag=flag, **kw)
    assert int(flag.item()) == 1


@pytest.mark.parametrize("projection", [False, True])
@pytest.mark.parametrize("H,W", [(8, 16), (11, 17)])
def test_bottleneck_eight_row_tiles_match_the_f64_block(ops, dev, H, W, projection):
    _run(ops, dev, H, W, 64, 256 if projection else 64, projection)


@pytest.mark.parametrize("projection", [False, True])
def test_bottleneck_ten_row_tiles_match_the_f64_block(ops, dev, projection):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    slots = 2 * cus                                       # two workgroups per CU: one round of the launch
    tiles_x = slots // 5 + 1                              # 39 rows: five 8-row tiles or four 10-row tiles per column
    H, W = 39, 16 * tiles_x - 5                           # (ragged on both edges)
    assert 5 * tiles_x > slots >= 4 * tiles_x, "the 8-row tiling must need two rounds and the 10-row tiling one"
    # the launcher's rule: rounds x MFMAs of the slowest wave; Cin = Cout = 64 (projection: 8 chunks per conv3 slice instead of 4)
    c3 = 8 if projection else 4
    assert 2 * 3 * (3 * 4 + 2 * 36 + 2 * c3) > 1 * 3 * (4 * 4 + 3 * 36 + 3 * c3)
    _run(ops, dev, H, W, 64, 64, projection)
