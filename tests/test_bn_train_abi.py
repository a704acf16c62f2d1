"""Train-mode BatchNorm's C ABI, the switches of HarDNetFeatureExtraction / FasterRCNNTrainer that need no
device, and the torch-f32 yardstick of tests/bn_train_restated.py: everything here runs without a GPU."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_train_restated as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from two_stage_object_detection_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi, _ffi.lib()


def _status(L, rc):
    return L.tsod_status_str(rc).decode().upper()


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    raw_text = open(os.path.join(ROOT, "include", "tsod.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_bn_train_workspace_bytes", 2), ("tsod_bn_stats_f32", 20), ("tsod_bn_apply_f32", 14),
                         ("tsod_bn_train_grad_f32", 20)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
    assert int(re.search(r"#define TSOD_BN_ROWS_PER_WORKGROUP (\d+)", raw_text).group(1)) == _ffi.BN_ROWS_PER_WORKGROUP
    assert _ffi._SIGNATURES["tsod_bn_stats_f32"][1][8:10] == [ctypes.c_double, ctypes.c_double]       # eps, momentum


def test_argument_errors():
    """Every argument check returns its code on the host, before any launch (the pointers are never dereferenced)."""
    _, L = _lib()
    A, odd = 0x10000, 0x10004
    ws = L.tsod_bn_train_workspace_bytes(70, 12)
    assert ws > 0 and L.tsod_bn_train_workspace_bytes(1, 12) == 0 and L.tsod_bn_train_workspace_bytes(70, 10) == 0

    def stats(z=A, M=70, C_real=10, C_pad=12, ld=32, off=8, gamma=A, beta=A, mean=A, invstd=A, scale=A, shift=A, w=A, wb=ws):
        return L.tsod_bn_stats_f32(z, M, C_real, C_pad, ld, off, gamma, beta, 1e-5, 0.1, None, None, None, mean, invstd, scale,
                                   shift, w, wb, None)

    def apply(z=A, M=70, C_real=10, C_pad=12, z_ld=32, z_off=8, scale=A, shift=A, act=2, y=A, y_ld=12, y_off=0, amax=None):
        return L.tsod_bn_apply_f32(z, M, C_real, C_pad, z_ld, z_off, scale, shift, act, y, y_ld, y_off, amax, None)

    def grad(g=A, g_ld=12, g_off=0, z=A, z_ld=32, z_off=8, M=70, C_real=10, C_pad=12, mean=A, invstd=A, gamma=A, dz=A, dz_ld=16,
             dz_off=4, dgamma=A, dbeta=A, w=A, wb=ws):
        return L.tsod_bn_train_grad_f32(g, g_ld, g_off, z, z_ld, z_off, M, C_real, C_pad, mean, invstd, gamma, dz, dz_ld, dz_off,
                                        dgamma, dbeta, w, wb, None)
    # a null required pointer
    for fn, names in ((stats, ("z", "gamma", "beta", "mean", "invstd", "scale", "shift")), (apply, ("z", "scale", "shift", "y")),
                      (grad, ("g", "z", "mean", "invstd", "gamma", "dz", "dgamma", "dbeta"))):
        for k in names:
            assert "INVALID" in _status(L, fn(**{k: None})), (fn.__name__, k)
        # C_pad % 4, a misaligned pointer
        assert "ALIGN" in _status(L, fn(C_pad=10)), fn.__name__
        assert "ALIGN" in _status(L, fn(z=odd)), fn.__name__
        # more real channels than padded ones
        assert "INVALID" in _status(L, fn(C_real=13)), fn.__name__
    # fewer than two rows (torch refuses one value per channel in training mode); apply is elementwise and takes one
    assert "INVALID" in _status(L, stats(M=1)) and "INVALID" in _status(L, grad(M=1)) and "INVALID" in _status(L, apply(M=0))
    # offsets beyond ld, pitches and offsets that are no multiples of 4
    assert "INVALID" in _status(L, stats(off=24)) and "INVALID" in _status(L, stats(off=-4))
    assert "INVALID" in _status(L, apply(z_off=24)) and "INVALID" in _status(L, apply(y_off=4))
    assert "INVALID" in _status(L, grad(g_off=4)) and "INVALID" in _status(L, grad(z_off=24)) and "INVALID" in _status(L, grad(dz_off=8))
    assert "ALIGN" in _status(L, stats(ld=34)) and "ALIGN" in _status(L, stats(off=6))
    assert "ALIGN" in _status(L, apply(y_ld=14)) and "ALIGN" in _status(L, apply(scale=odd)) and "ALIGN" in _status(L, apply(amax=A + 16))
    assert "ALIGN" in _status(L, grad(dz_ld=18)) and "ALIGN" in _status(L, grad(mean=odd))
    # activation, workspace
    assert "UNSUPPORTED" in _status(L, apply(act=1))
    for fn in (stats, grad):
        assert "WORKSPACE" in _status(L, fn(w=None)) and "WORKSPACE" in _status(L, fn(wb=ws - 8)), fn.__name__


def test_workspace_is_one_partial_pair_per_workgroup_plus_the_totals():
    _ffi, L = _lib()
    Rw = _ffi.BN_ROWS_PER_WORKGROUP
    q = L.tsod_bn_train_workspace_bytes
    for M in (2, Rw, Rw + 1, 3 * Rw + 5, 90000):
        assert q(M, 68) == (-(-M // Rw) + 1) * 2 * 68 * 8


def test_modes_and_trainer_arguments():
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    m = HarDNetFeatureExtraction(depth_wise=True, arch=39)
    keys = list(m.state_dict())
    assert m.train_blocks(1, batch_stats=True) is m and m._batch_stats and m.train_mode == 1
    assert m.eval()._plan_variant() == m.train_blocks(1)._plan_variant() == ("train_blocks", 1)     # eval(): the key is unchanged
    assert m.train_blocks(1, batch_stats=True).train()._plan_variant() == ("train_blocks", 1, "batch_stats")
    with torch.no_grad():
        assert m._plan_variant() == () and not m._trains_in_plan()
    assert m.train_full(batch_stats=True)._plan_variant() == ("train_full", "batch_stats")
    assert not m.train_blocks(0, batch_stats=True)._batch_stats and not m.set_train_mode("tail", True)._batch_stats   # no BN there
    assert not m.train_blocks(2)._batch_stats and list(m.state_dict()) == keys
    m.base[12].layers[1].layer2.norm.momentum = None
    m.train_blocks(1)                                                     # folded: nothing to refuse
    with pytest.raises(NotImplementedError, match="base.12.layers.1.layer2.norm"):
        m.train_blocks(1, batch_stats=True)
    m.base[12].layers[1].layer2.norm.momentum = 0.1
    m.base[0].norm.track_running_stats = False
    m.train_blocks(4, batch_stats=True)                                   # the stem is not reached
    with pytest.raises(NotImplementedError, match="base.0.norm"):
        m.train_full(batch_stats=True)
    with pytest.raises(ValueError, match="bn_batch_stats"):
        FasterRCNNTrainer("train", 20, bn_batch_stats=True)
    with pytest.raises(ValueError, match="bn_batch_stats"):
        FasterRCNNTrainer("train", 20, backbone_grads="tail", bn_batch_stats=True)
    assert FasterRCNNTrainer("train", 20, backbone_grads=1, bn_batch_stats=True).bn_batch_stats
    assert not FasterRCNNTrainer("train", 20, backbone_grads=1).bn_batch_stats


def test_refresh_watches_the_batchnorm_buffers():
    """refresh_packs' version tuple covers the running statistics: an in-place edit of a buffer makes its unit stale."""
    from two_stage_object_detection_amd.models import hardnet_grads
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    m = HarDNetFeatureExtraction(depth_wise=True, arch=39).train_blocks(1)
    hardnet_grads.refresh_packs(m)
    seen = dict(m.__dict__["_pack_versions"])
    m.base[13].norm.running_var.mul_(2.0)
    torch.autograd.graph.increment_version(m.base[12].layers[0].layer2.norm.running_mean)
    hardnet_grads.refresh_packs(m)
    now = m.__dict__["_pack_versions"]
    assert {k for k in now if now[k] != seen[k]} == {"base.13", "base.12.layers.0.layer2"}


def test_yardstick_table_describes_torch_f32():
    """YARDSTICK is what torch's float32 CPU batch_norm shows against float64 on the sweep's inputs (within a factor 2: other
    builds of torch may add in another order), and the float64 reference is torch's formula."""
    _ffi, _ = _lib()
    table = R.measure_yardstick(_ffi.BN_ROWS_PER_WORKGROUP)
    assert set(table) == set(R.YARDSTICK)
    for cell, row in table.items():
        for q, v in row.items():
            assert 0.5 * R.YARDSTICK[cell][q] <= v <= 2.0 * R.YARDSTICK[cell][q], (cell, q, v, R.YARDSTICK[cell][q])
    c, ref = R.case(3, 10, 12, "offset"), R.reference(3, 10, 12, "offset")
    z = c["z"][:, R.OFF:R.OFF + 10].double()
    xhat = (z - ref["mean"]) * ref["invstd"]
    g = c["g"][:, R.OFF:R.OFF + 10].double()
    assert torch.allclose(ref["y"], xhat * c["gamma"].double() + c["beta"].double(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["dgamma"], (g * xhat).sum(0), rtol=1e-10) and torch.allclose(ref["dbeta"], g.sum(0), rtol=1e-12)
    want = c["gamma"].double() * ref["invstd"] * (g - g.mean(0) - xhat * (g * xhat).mean(0))
    assert float((ref["dz"].detach() - want).abs().max()) <= 1e-9 * float((c["gamma"].double() * ref["invstd"]).max())
    var = z.var(0, unbiased=True)
    assert torch.allclose(ref["running_var"], 0.9 * c["running_var"].double() + 0.1 * var, rtol=1e-12)


def test_saved_forward_restatement_against_plain_autograd():
    """bn_section_reference, fed the plain float64 forward's own z / outputs as the 'saved' ones, is plain autograd of the modules
    in .train() (stem, a DWConvLayer in front of the second block, two HarDBlocks), and T bounds every gradient."""
    from pw_grads_restated import block_forward_plain
    from two_stage_object_detection_amd.models.hardnet import ConvLayer, DWConvLayer, HarDBlock
    torch.manual_seed(5)
    mods = [ConvLayer(3, 8, kernel=3, stride=2), ConvLayer(8, 10, kernel=1), DWConvLayer(10, stride=2),
            HarDBlock(10, 6, 1.6, 4, dwconv=True), None, DWConvLayer(12, stride=1), HarDBlock(12, 6, 1.6, 2, dwconv=True), None]
    mods[4], mods[7] = ConvLayer(mods[3].get_out_ch(), 12, kernel=1), ConvLayer(mods[6].get_out_ch(), 8, kernel=1)
    base = torch.nn.ModuleList(mods).double().train()
    for mod in base.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    seen = {}
    for name, mod in base.named_modules():
        if isinstance(mod, (torch.nn.Conv2d, ConvLayer, DWConvLayer)):
            mod.register_forward_hook(lambda _m, _i, out, name=name: seen.__setitem__(name, out.detach()))
    x = torch.randn(2, 3, 12, 20, dtype=torch.float64)

    def forward(t):
        t = base[2](base[1](base[0](t)))
        t, s3, _ = block_forward_plain(base[3], base[4], t)
        t, s6, _ = block_forward_plain(base[6], base[7], base[5](t))
        return t, s3, s6
    out, s3, s6 = forward(x)
    gy = torch.randn_like(out)
    params = {f"base.{k}": p for k, p in base.named_parameters()}
    plain = torch.autograd.grad(out, list(params.values()), gy)

    def block(i, slices, down):
        blk = base[i]
        L = range(len(blk.layers))
        return dict(index=i, block=blk, tr_index=i + 1, transition=base[i + 1], down=down, down_index=i - 1,
                    down_z=seen.get(f"{i - 1}.dwconv"), slices=[s.detach() for s in slices],
                    ys=[seen[f"{i}.layers.{l}.layer1"] for l in L], zs=[seen[f"{i}.layers.{l}.layer1.conv"] for l in L],
                    dw_zs=[seen[f"{i}.layers.{l}.layer2.dwconv"] for l in L], tr_y=seen[f"{i + 1}"], tr_z=seen[f"{i + 1}.conv"])
    stem = dict(mods=(base[0], base[1], base[2]), y0=seen["0"], z0=seen["0.conv"], y1=seen["1"], z1=seen["1.conv"], z2=seen["2.dwconv"])
    ref = R.bn_section_reference([block(3, s3, None), block(6, s6, base[5])], None, x, gy, stem=stem)
    assert set(ref) == set(params)
    for (name, p), g in zip(params.items(), plain):
        got, T, n = ref[name]
        assert got.shape == p.shape and n > 0 and bool((T >= got.abs() * (1 - 1e-9)).all()), name
        assert float((got - g).abs().max()) <= 1e-10 * max(float(g.abs().max()), float(T.max()) * 1e-3), name
    assert ref["base.7.norm.bias"][2] < ref["base.0.conv.weight"][2]          # (more BatchNorms above the stem than above the end)
