"""Active dropout without a device: the generator's known answers (NumPy restatement and csrc/philox.h
through tsod_philox4x32_host), the C ABI and its refusals, the switches of HarDNetFeatureExtraction / FasterRCNNTrainer, and the
keep rate of the mask."""
import copy
import ctypes
import math
import os
import pickle
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_restated as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def _lib():
    from two_stage_object_detection_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi, _ffi.lib()


def _status(L, rc):
    return L.tsod_status_str(rc).decode().upper()


def test_known_answers_restatement_and_header():
    _, L = _lib()
    for ctr, key, want in KNOWN:
        assert tuple(int(v) for v in D.philox4x32_10(ctr, key)) == want
        out = (ctypes.c_uint32 * 4)()
        L.tsod_philox4x32_host((ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), out)
        assert tuple(out) == want
    # a batch of counters is the single calls side by side, and words() takes the lanes in element order
    ctrs = [np.array([c[i] for c, _, _ in KNOWN[::2]], dtype=np.uint32) for i in range(4)]
    assert [int(v[0]) for v in D.philox4x32_10(ctrs, (0, 0))] == list(KNOWN[0][2])
    w = D.words(7, (5, 6), ordinal=3, e0=(1 << 34) - 6)
    e = (1 << 34) - 6
    for i in range(7):
        c = (e + i) >> 2
        assert int(w[i]) == int(D.philox4x32_10((c & 0xFFFFFFFF, c >> 32, 3, 0), (5, 6))[(e + i) & 3])


def test_threshold_and_scale_are_the_restatements():
    _, L = _lib()
    for p in (0.0, 0.1, 0.25, 0.3, 0.5, 0.9, 1.0, 1e-10, 1.0 - 2.0 ** -24):
        thr, scale = ctypes.c_uint64(), ctypes.c_float()
        assert L.tsod_dropout_params(p, ctypes.byref(thr), ctypes.byref(scale)) == 0
        want_thr, want_scale = D.params(p)
        assert thr.value == want_thr and np.float32(scale.value) == want_scale, p
    assert D.params(0.1) == (429496736, np.float32(1.0 / (1.0 - float(np.float32(0.1)))))        # p arrives as a C float
    assert D.params(0.1, as_float32=False)[0] == 429496730 and D.params(1.0) == (1 << 32, np.float32(0.0))
    for p in (-0.25, 1.5, float("nan"), float("inf")):
        assert "INVALID" in _status(L, L.tsod_dropout_params(p, ctypes.byref(ctypes.c_uint64()), ctypes.byref(ctypes.c_float())))
    assert "INVALID" in _status(L, L.tsod_dropout_params(0.5, None, ctypes.byref(ctypes.c_float())))


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    raw_text = open(os.path.join(ROOT, "include", "tsod.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_dropout_segs_f32", 15), ("tsod_dropout_key_set", 4), ("tsod_dropout_params", 3),
                         ("tsod_philox4x32_host", 3)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name) and name in _ffi.EXPORTED_SYMBOLS, name
    assert int(re.search(r"#define TSOD_DROPOUT_MAX_SEGMENTS (\d+)", raw_text).group(1)) == _ffi.DROPOUT_MAX_SEGMENTS
    sig = _ffi._SIGNATURES["tsod_dropout_segs_f32"][1]
    assert sig[10] is ctypes.c_float and sig[12] is ctypes.c_uint32 and sig[13] is ctypes.c_uint64      # p, ordinal, e0
    assert ctypes.sizeof(_ffi.DropoutSeg) == 12 and [f[0] for f in _ffi.DropoutSeg._fields_] == ["off", "real", "first"]
    assert "dropout.hip" in open(os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "Makefile")).read()


def test_argument_errors():
    """Every refusal returns its code on the host, before any launch (the pointers are never dereferenced)."""
    from two_stage_object_detection_amd import hip_ops
    _, L = _lib()
    A, odd = 0x10000, 0x10004
    good = [(4, 6, 0), (16, 10, 6), (32, 2, 16)]

    def call(src=A, dst=A + 0x1000, N=1, H=3, W=5, sp=40, dp=40, segs=good, n=None, C=18, p=0.1, key=A + 0x2000, table=True):
        t = hip_ops.dropout_seg_table(segs) if table else None
        return _status(L, L.tsod_dropout_segs_f32(src, dst, N, H, W, sp, dp, t, len(segs) if n is None else n, C, p, key, 0, 0, None))
    # null pointers, sizes
    for kw in (dict(src=None), dict(dst=None), dict(key=None), dict(table=False)):
        assert "INVALID" in call(**kw), kw
    for kw in (dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(n=0), dict(sp=0), dict(dp=-4)):
        assert "INVALID" in call(**kw), kw
    # p outside [0, 1], NaN
    for p in (-1e-6, 1.0 + 2.0 ** -20, float("nan"), float("inf")):
        assert "INVALID" in call(p=p), p
    # pitches and offsets that are no multiples of 4, misaligned pointers
    assert "ALIGN" in call(sp=42) and "ALIGN" in call(dp=38) and "ALIGN" in call(segs=[(6, 6, 0)], C=6)
    assert "ALIGN" in call(src=odd) and "ALIGN" in call(dst=A + 8) and "ALIGN" in call(key=A + 0x2002)
    # a slice that does not fit its pitch (with its pad lanes), in src or in dst; negative fields
    assert "INVALID" in call(segs=[(32, 10, 0)], C=10) and "INVALID" in call(segs=[(36, 5, 0)], C=5)
    assert "INVALID" in call(dp=32) and "INVALID" in call(sp=32)
    assert "INVALID" in call(segs=[(-4, 6, 0)], C=6) and "INVALID" in call(segs=[(4, 0, 0)], C=6) and "INVALID" in call(segs=[(4, 6, -1)], C=6)
    # logical channels that overlap or exceed C; slices that share a lane of the pixel
    assert "INVALID" in call(C=17) and "INVALID" in call(segs=[(4, 6, 0), (16, 10, 5)])
    assert "INVALID" in call(segs=[(4, 6, 0), (8, 4, 6)], C=10)                      # (lanes [4, 12) and [8, 12))
    # more slices than the table holds
    many = [(4 * i, 4, 4 * i) for i in range(17)]
    assert "UNSUPPORTED" in call(segs=many, sp=68, dp=68, C=68)
    assert "INVALID" in _status(L, L.tsod_dropout_key_set(None, 1, 2, None))
    assert "ALIGN" in _status(L, L.tsod_dropout_key_set(A + 2, 1, 2, None))


def test_modes_and_trainer_arguments():
    from two_stage_object_detection_amd.models.hardnet import HarDNetFeatureExtraction
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    m = HarDNetFeatureExtraction(depth_wise=True, arch=85)
    keys = list(m.state_dict())
    for args in (("tail", False, True), (None, False, True), ("tail", True, True), (1, False, True), ("full", False, True)):
        with pytest.raises(ValueError, match="batch_stats"):
            m.set_train_mode(*args)
    with pytest.raises(ValueError, match="batch_stats"):
        m.train_blocks(1, dropout=True)
    with pytest.raises(ValueError, match="batch_stats"):
        m.train_blocks(0, batch_stats=True, dropout=True)
    with pytest.raises(ValueError, match="batch_stats"):
        m.train_full(dropout=True)
    assert m.train_blocks(1, batch_stats=True, dropout=True) is m and m._dropout and m._batch_stats
    # the plan-variant key gains "dropout" only where the batch-statistics variant runs and the section holds a Dropout
    assert m.eval()._plan_variant() == ("train_blocks", 1)
    assert m.train()._plan_variant() == ("train_blocks", 1, "batch_stats", "dropout") and m._drops_in_plan()
    import torch
    with torch.no_grad():
        assert m._plan_variant() == () and not m._drops_in_plan()
    assert m.train_full(True, True)._plan_variant() == ("train_full", "batch_stats", "dropout")
    assert m.train_blocks(1, batch_stats=True)._plan_variant() == ("train_blocks", 1, "batch_stats") and not m._dropout
    assert m.train_blocks(1).eval()._plan_variant() == ("train_blocks", 1)
    drop, = [mod for mod in m.base if isinstance(mod, torch.nn.Dropout)]
    assert drop is m.base[17] and drop.p == 0.1
    drop.p = 0.0                                                        # nothing to drop: today's key
    assert m.train_blocks(1, True, True).train()._plan_variant() == ("train_blocks", 1, "batch_stats")
    drop.p = 0.1
    # pickling and deep copy keep the flag, the state_dict never sees it
    m.train_blocks(2, batch_stats=True, dropout=True)
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c._dropout and c._batch_stats and c.train_mode == 2 and c.train()._plan_variant()[-1] == "dropout"
    assert list(m.state_dict()) == keys
    # HarDNet-39 / 68 have no Dropout: the flag is accepted and changes no key
    for arch in (39, 68):
        a = HarDNetFeatureExtraction(depth_wise=True, arch=arch)
        for mode, want in ((1, ("train_blocks", 1)), ("full", ("train_full",))):
            with_flag = a.set_train_mode(mode, True, True).train()._plan_variant()
            assert with_flag == a.set_train_mode(mode, True).train()._plan_variant() == want + ("batch_stats",)
            assert a.set_train_mode(mode, True, True).eval()._plan_variant() == want and not a._drops_in_plan()
    # the trainer
    with pytest.raises(ValueError, match="bn_batch_stats"):
        FasterRCNNTrainer("train", 3, backbone="hardnet85", backbone_grads=1, dropout=True)
    with pytest.raises(TypeError):
        FasterRCNNTrainer("train", 3, 16, [8, 16, 32], [0.5, 1, 2], "hardnet85", "pool", "chw", False, 1, True, True)   # keyword-only
    tr = FasterRCNNTrainer("train", 3, backbone="hardnet85", head_grads=True, backbone_grads=1, bn_batch_stats=True, dropout=True)
    assert tr.dropout and tr.bn_batch_stats
    assert not FasterRCNNTrainer("train", 3, backbone="hardnet85", backbone_grads=1, bn_batch_stats=True).dropout


def test_keep_count_of_the_restatement():
    """2^20 elements, key (0x1234, 0x5678), p = the double 0.1: 944 625 kept at thr = 429 496 730 - 2.95 sigma from n (1 - p);
    the bar is 4 sigma of the binomial."""
    n, p = 1 << 20, 0.1
    thr = D.params(p, as_float32=False)[0]
    assert thr == 429496730
    kept = int(D.keep_mask(n, 1, p, (0x1234, 0x5678), thr=thr).sum())
    sigma = math.sqrt(n * p * (1 - p))
    print(f"kept {kept} of {n}: {(kept - n * (1 - p)) / sigma:+.2f} sigma")
    assert kept == 944625
    assert abs(kept - n * (1 - p)) <= 4 * sigma
    # the element index alone decides: any split of the same range gives the same words, another ordinal other ones
    w = D.words(1000, (0x1234, 0x5678))
    assert np.array_equal(np.concatenate([D.words(333, (0x1234, 0x5678)), D.words(667, (0x1234, 0x5678), e0=333)]), w)
    assert not np.array_equal(D.words(1000, (0x1234, 0x5678), ordinal=1), w)


def test_section_restatement_against_plain_autograd():
    """tests/hardnet_dropout_restated.py, fed a plain float64 forward's own z / outputs as the 'saved' ones: with a mask of ones it
    is bn_train_restated.bn_section_reference (gradients, T and n), with a dropout mask it is plain autograd of the modules in
    .train() with the multiply in front of the transition layer."""
    import torch
    import bn_train_restated as R
    import hardnet_dropout_restated as H
    from two_stage_object_detection_amd.models.hardnet import ConvLayer, HarDBlock
    torch.manual_seed(7)
    blk = HarDBlock(10, 6, 1.6, 4, dwconv=True)
    base = torch.nn.ModuleList([blk, ConvLayer(blk.get_out_ch(), 12, kernel=1)]).double().train()
    for mod in base.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    seen = {}
    for name, mod in base.named_modules():
        if isinstance(mod, (torch.nn.Conv2d, ConvLayer)) or name.endswith("layer2"):
            mod.register_forward_hook(lambda _m, _i, out, name=name: seen.__setitem__(name, out.detach()))
    x = torch.randn(2, 10, 5, 7, dtype=torch.float64)
    C = blk.get_out_ch()
    keep = D.keep_mask(2 * 5 * 7, C, 0.3, (9, 10))
    mask = (torch.from_numpy(keep).double() * float(D.params(0.3)[1])).view(2, 5, 7, C).permute(0, 3, 1, 2)
    params = {f"base.{k}": p for k, p in base.named_parameters()}
    for m_ in (torch.ones_like(mask), mask):
        layers_ = [x]
        for li, comb in enumerate(blk.layers, start=1):
            layers_.append(comb(torch.cat([layers_[k] for k in blk.links[li - 1]], 1)))
        out = base[1](torch.cat([layers_[k] for k in blk.output_slices()], 1) * m_)
        gy = torch.randn(out.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        plain = torch.autograd.grad(out, list(params.values()), gy)
        L = range(len(blk.layers))
        b = dict(index=0, block=blk, tr_index=1, transition=base[1], down=None, slices=[s.detach() for s in layers_],
                 ys=[seen[f"0.layers.{l}.layer1"] for l in L], zs=[seen[f"0.layers.{l}.layer1.conv"] for l in L],
                 dw_zs=[seen[f"0.layers.{l}.layer2.dwconv"] for l in L], tr_y=seen["1"], tr_z=seen["1.conv"])
        ref = H.section_reference(b, None, gy, None, m_)
        assert set(ref) == set(params)
        for (name, p), g in zip(params.items(), plain):
            got, T, n = ref[name]
            assert got.shape == p.shape and n > 0 and bool((T >= got.abs() * (1 - 1e-9)).all()), name
            assert float((got - g).abs().max()) <= 1e-10 * max(float(g.abs().max()), float(T.max()) * 1e-3), name
        if bool((m_ == 1).all()):
            same = R.bn_section_reference([b], None, x, gy)
            for name in params:
                assert torch.equal(ref[name][0], same[name][0]) and torch.equal(ref[name][1], same[name][1]), name
                assert ref[name][2] == same[name][2], name
