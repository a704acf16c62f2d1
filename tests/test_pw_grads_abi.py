"""The 1x1 ConvLayer backward's C ABI, the public switches of section 4.18 and the float64 restatement the GPU tests lean on:
everything here runs without a GPU."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_grads_restated import block_forward_plain, section_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, ALIGNMENT, WORKSPACE = "INVALID_ARG", "ALIGNMENT", "WORKSPACE"


def _lib():
    from two_stage_object_detection_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi, _ffi.lib()


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_dwconv3x3_grad_act_f32", 25), ("tsod_relu6_grad_mask_f32", 10), ("tsod_pw_wgrad_workspace_bytes", 3),
                         ("tsod_pw_wgrad_f32", 16), ("tsod_pw_dgrad_f32", 11)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
    assert L.tsod_version() == 242
    assert ctypes.sizeof(_ffi.PwSegs) == 4 * (1 + 4 * _ffi.PW_MAX_SEGMENTS)


def _status(L, rc):
    return L.tsod_status_str(rc).decode().upper()


def test_argument_errors():
    """The entry points refuse bad arguments on the host, before any launch (the pointers are never dereferenced)."""
    from two_stage_object_detection_amd import hip_ops
    _ffi, L = _lib()
    A, odd = 0x10000, 0x10004                                   # a 16-byte aligned address and a misaligned one
    sg = hip_ops.pw_segs([(0, 12), (20, 8)], real=[10, 6])
    by = ctypes.byref
    # mask pass: NULL, misaligned pointer, pitch not a multiple of 4
    assert L.tsod_relu6_grad_mask_f32(None, 70, 8, 8, A, 8, 0, A, 8, None) != 0
    assert "ALIGN" in _status(L, L.tsod_relu6_grad_mask_f32(odd, 70, 8, 8, A, 8, 0, A, 8, None))
    assert "ALIGN" in _status(L, L.tsod_relu6_grad_mask_f32(A, 70, 8, 10, A, 8, 0, A, 8, None))
    assert L.tsod_relu6_grad_mask_f32(A, 70, 8, 4, A, 8, 0, A, 8, None) != 0          # pitch below C
    # wgrad: no output at all, NULL operands, misaligned x, bad pitch, segment outside the pitch, short workspace
    ws = L.tsod_pw_wgrad_workspace_bytes(70, 8, 20)
    assert ws > 0
    assert L.tsod_pw_wgrad_f32(A, 70, 8, 8, A, 40, by(sg), A, A, 6, None, None, None, A, ws, None) != 0
    assert L.tsod_pw_wgrad_f32(None, 70, 8, 8, A, 40, by(sg), A, A, 6, A, A, A, A, ws, None) != 0
    assert L.tsod_pw_wgrad_f32(A, 70, 8, 8, A, 40, None, A, A, 6, A, A, A, A, ws, None) != 0
    assert "ALIGN" in _status(L, L.tsod_pw_wgrad_f32(A, 70, 8, 8, odd, 40, by(sg), A, A, 6, A, A, A, A, ws, None))
    assert "ALIGN" in _status(L, L.tsod_pw_wgrad_f32(A, 70, 8, 8, A, 42, by(sg), A, A, 6, A, A, A, A, ws, None))
    assert L.tsod_pw_wgrad_f32(A, 70, 8, 8, A, 24, by(sg), A, A, 6, A, A, A, A, ws, None) != 0
    assert L.tsod_pw_wgrad_f32(A, 70, 8, 8, A, 40, by(sg), A, A, 9, A, A, A, A, ws, None) != 0      # n_real > N
    assert "WORKSPACE" in _status(L, L.tsod_pw_wgrad_f32(A, 70, 8, 8, A, 40, by(sg), A, A, 6, A, A, A, A, ws - 4, None))
    assert "WORKSPACE" in _status(L, L.tsod_pw_wgrad_f32(A, 70, 8, 8, A, 40, by(sg), A, A, 6, A, A, A, None, ws, None))
    bad = hip_ops.pw_segs([(0, 12), (22, 8)], real=[10, 6])                            # offset not a multiple of 4
    assert "ALIGN" in _status(L, L.tsod_pw_wgrad_f32(A, 70, 8, 8, A, 40, by(bad), A, A, 6, A, A, A, A, ws, None))
    # dgrad
    assert L.tsod_pw_dgrad_f32(A, 70, 8, 8, A, A, by(sg), None, 40, 0, None) != 0
    assert "ALIGN" in _status(L, L.tsod_pw_dgrad_f32(odd, 70, 8, 8, A, A, by(sg), A, 40, 0, None))
    assert "ALIGN" in _status(L, L.tsod_pw_dgrad_f32(A, 70, 8, 10, A, A, by(sg), A, 40, 0, None))
    assert L.tsod_pw_dgrad_f32(A, 70, 8, 8, A, A, by(sg), A, 24, 0, None) != 0
    none = hip_ops.pw_segs([(0, 12), (20, 8)], real=[10, 6], want=[False, False])
    assert L.tsod_pw_dgrad_f32(A, 70, 8, 8, A, A, by(none), A, 40, 0, None) == 0          # nobody wants a segment: no launch
    # the fused-mask depthwise entry point keeps tsod_dwconv3x3_grad_f32's checks
    assert L.tsod_dwconv3x3_grad_act_f32(None, 1, 4, 4, 8, 8, 0, A, None, None, 1, 0, A, 8, 0, A, 8, 0, 0, None, None, None, None, 0,
                                         None) != 0
    assert "ALIGN" in _status(L, L.tsod_dwconv3x3_grad_act_f32(A, 1, 4, 4, 8, 10, 0, A, None, None, 1, 0, A, 8, 0, A, 8, 0, 0, None,
                                                                None, None, None, 0, None))
    with pytest.raises(ValueError):
        hip_ops.pw_segs([(0, 4)] * 17)


def test_workspace_queries_are_monotone_and_of_the_order_of_the_operands():
    _, L = _lib()
    q = L.tsod_pw_wgrad_workspace_bytes
    assert q(0, 8, 8) == 0 and q(8, 0, 8) == 0 and q(8, 8, 0) == 0
    for N, K in ((8, 20), (412, 1056), (1024, 732)):
        sizes = [q(M, N, K) for M in (70, 874, 5000, 22500, 90000, 534400)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (N, K, sizes)
        n_pad, k_pad = -(-N // 64) * 64, -(-K // 128) * 128
        tile = n_pad * (k_pad + 1) * 4                                              # one slice: a padded tile + its column sums
        assert sizes[0] == tile                                                     # few rows: one slice
        for M, s in zip((5000, 22500, 90000, 534400), sizes[2:]):
            assert s % tile == 0 and 1 <= s // tile <= 512
            assert (s // tile) * n_pad * k_pad <= max(n_pad * k_pad, M * (N + K)), (M, N, K, s)   # never more slab floats than operands
    assert q(22500, 1024, 732) >= q(22500, 412, 732) and q(22500, 412, 1056) >= q(22500, 412, 732)
    assert q(874, 1024, 732) < L.tsod_wgrad_workspace_bytes(874, 1024, 732)       # (that rule: slabs 3x the operands here)


def test_train_blocks_and_backbone_grads_arguments():
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    m = HarDNetFeatureExtraction(depth_wise=True, arch=39)
    keys = list(m.state_dict())
    with pytest.raises(ValueError, match="train_blocks"):
        m.train_blocks(5)
    with pytest.raises(ValueError, match="train_blocks"):
        m.train_blocks(-1)
    assert m.train_blocks(0) is m and m.train_mode == "tail"
    assert [id(p) for p in m.trainable_parameters()] == [id(p) for p in m.tail_parameters()]
    m.train_blocks(1)
    names = [k for k, _ in m._trainable_named()]
    assert names[0] == "base.12.layers.0.layer1.conv.weight" and names[-1] == "base.17.bias"
    assert len(names) == 4 * 6 + 3 + 6 and list(m.state_dict()) == keys
    want = [p for i in range(12, 18) for p in m.base[i].parameters()]
    assert [id(p) for p in m.trainable_parameters()] == [id(p) for p in want]
    m.train_blocks(2)
    assert [k for k, _ in m._trainable_named()][0] == "base.9.layers.0.layer1.conv.weight"
    assert any(k.startswith("base.11.dwconv") for k, _ in m._trainable_named())
    assert len(m.train_blocks(4).trainable_parameters()) == len(list(m.parameters())) - 9     # everything but the stem
    assert m.train_tail(False).train_mode is None
    with pytest.raises(ValueError, match="backbone_grads"):
        FasterRCNNTrainer("train", 20, backbone_grads=-1)
    with pytest.raises(ValueError, match="backbone_grads"):
        FasterRCNNTrainer("train", 20, backbone_grads=0)
    with pytest.raises(ValueError, match="backbone_grads"):
        FasterRCNNTrainer("train", 20, backbone_grads=True)
    with pytest.raises(ValueError, match="HarDBlocks"):
        FasterRCNNTrainer("train", 20, backbone_grads=5)
    with pytest.raises(ValueError, match="backbone_grads"):
        FasterRCNNTrainer("train", 20, backbone="resnet50", backbone_grads=1)
    assert FasterRCNNTrainer("train", 20, backbone_grads=2).backbone_grads == 2


def test_restatement_against_plain_autograd_of_a_small_hardblock():
    """section_reference, fed the plain forward's own float64 outputs as the 'saved' ones, is plain autograd of the modules."""
    from two_stage_object_detection_amd.models.hardnet import ConvLayer, HarDBlock
    torch.manual_seed(3)
    blk = HarDBlock(10, 6, 1.6, 4, dwconv=True).double().eval()
    tr = ConvLayer(blk.get_out_ch(), 12, kernel=1).double().eval()
    for mod in list(blk.modules()) + list(tr.modules()):
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    x = torch.randn(2, 10, 5, 7, dtype=torch.float64)
    gy = torch.randn(2, 12, 5, 7, dtype=torch.float64)
    params = dict([(f"base.0.{k}", p) for k, p in blk.named_parameters()] + [(f"base.1.{k}", p) for k, p in tr.named_parameters()])
    out, slices, ys = block_forward_plain(blk, tr, x)
    plain = torch.autograd.grad(out, list(params.values()), gy)
    with torch.no_grad():
        out, slices, ys = block_forward_plain(blk, tr, x)
    sat = sum(int(((y <= 0) | (y >= 6)).sum()) for y in ys + [out])
    assert sat > 0                                                     # (the mask is exercised)
    ref = section_reference([dict(index=0, block=blk, tr_index=1, transition=tr, down=None, slices=slices, ys=ys, tr_y=out)],
                            None, x, gy)
    assert set(ref) == set(params)
    for (name, p), g in zip(params.items(), plain):
        got, T, n = ref[name]
        assert got.shape == p.shape and n > 0 and bool((T >= got.abs() * (1 - 1e-12)).all()), name
        assert float((got - g).abs().max()) <= 1e-12 * float(g.abs().max()), name
