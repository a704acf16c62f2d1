"""Every (tile, arithmetic) pair of the implicit-GEMM convolution library (csrc/conv_igemm_f32.hip) at its gather, epilogue
and K-slice switches, against the float64 restatement of tests/conv_restated.py with the bars derived there.

The unmarked tests run on any machine: the restatement against F.conv2d, the reciprocal k -> (tap, channel) split against
integer division, the coverage the case table gives every pair, and the restated scheduler against the library's resolver.
The gpu tests call tsod_conv2d_dual_f32 through the C ABI with descriptors of their own (res_off, pad_h != pad_w and offset
base pointers are not expressible through hip_ops.conv2d_nhwc), one test per (arithmetic, tile).

Data: randn activations and weights / sqrt(K); FAR in every input and residual channel outside the selected ones; image n
times 1000^n where a filter crosses image borders; outputs into SENTINEL-filled buffers whose bytes outside the written slice
must keep their bits; every launch twice, bit-identical.  Pass condition, per element: |got - y| <= bar(arithmetic, K, S) T.

With TSOD_CONV_KERNELS_JSONL=<path> the largest err / (bar T) of every (arithmetic, tile family, gather path, epilogue body,
schedule) is appended to that file, one JSON line each (TSOD_CONV_KERNELS_COMMIT names the commit in them)."""
import ctypes
import json
import math
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_restated as R  # noqa: E402

gpu = pytest.mark.gpu
SENTINEL = -7.25          # what an output buffer holds before a launch (tests/test_layer_kernels_gpu.py's value)
FAR = 1.0e6               # what the channels around an input / residual slice hold
ERR_UNSUPPORTED = -2      # include/tsod.h
PAIR_IDS = [f"{R.PREC_NAMES[p]}-{R.TILES[t].name}" for p, t in R.PAIRS]


@pytest.fixture(scope="module")
def ops():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def ffi():
    from two_stage_object_detection_amd import _ffi
    return _ffi


def all_cases():
    seen = {}
    for t in R.TILES:
        for c in R.cases_for(t):
            seen.setdefault(c, None)
    return tuple(seen)


# ----------------------------------------------------------------------------- operands and references, once per case
class Operands:
    def __init__(self, c: R.Case):
        g = torch.Generator().manual_seed(zlib.crc32(repr(c).encode()))
        e = c.epi
        x = torch.full((c.N, c.H, c.W, c.in_pitch), FAR)
        img = torch.tensor([1000.0 ** n if c.border else 1.0 for n in range(c.N)]).view(-1, 1, 1, 1) * e.gain
        for off, ln in c.segs:
            x[..., off:off + ln] = torch.randn(c.N, c.H, c.W, ln, generator=g) * img
        self.x = x
        self.w = torch.randn(c.Cout, c.K, generator=g) / math.sqrt(c.K)
        self.x2 = None
        if c.src2:
            c2, p2, off2, _, H2, W2 = c.src2
            self.x2 = torch.full((c.N, H2, W2, p2), FAR)
            self.x2[..., off2:off2 + c2] = torch.randn(c.N, H2, W2, c2, generator=g)
        sign = torch.where(torch.rand(c.Cout, generator=g) < 0.5, -1.0, 1.0)
        self.scale = (0.5 + torch.rand(c.Cout, generator=g)) * sign if e.scale else None
        self.shift = torch.randn(c.Cout, generator=g) if e.shift else None
        self.res = None
        if e.res:
            self.res = torch.full((c.M, c.res_pitch), FAR)
            self.res[:, e.res_off:e.res_off + c.Cout] = torch.randn(c.M, c.Cout, generator=g) * \
                (img / e.gain).view(-1).repeat_interleave(c.OH * c.OW).view(-1, 1)       # (of its image's order)
        sel = [R.gather_segments(x, c.segs)] + ([self.x2[..., c.src2[2]:c.src2[2] + c.src2[0]]] if c.src2 else [])
        self.exps = R.fp16x2_exponents(max(float(s.abs().max()) for s in sel), float(self.w.abs().max()))
        self._ref = {}
        self._dev = {}

    def ref(self, c: R.Case, prec: int):
        """(pre-activation y, activated y, T) in f64 [M, Cout]; fp16x2's T is over the floored magnitudes"""
        key = prec == R.FP16X2
        if key not in self._ref:
            fx, fw = (R.FP16_FLOOR / 2.0 ** self.exps[0], R.FP16_FLOOR / 2.0 ** self.exps[1]) if key else (0.0, 0.0)
            s2 = c.src2 or (0, 0, 0, 1, 0, 0)
            pre, T = R.conv_ref(self.x, self.w, segs=c.segs, KH=c.KH, KW=c.KW, stride=c.stride, pad_h=c.pad_h, pad_w=c.pad_w,
                                x2=self.x2, c2=s2[0], in2_off=s2[2], stride2=s2[3], scale=self.scale, shift=self.shift,
                                residual=self.res, res_off=c.epi.res_off, floor_x=fx, floor_w=fw)
            pre, T = pre.reshape(c.M, c.Cout), T.reshape(c.M, c.Cout)
            self._ref[key] = (pre, R.activation(pre, c.epi.act, c.epi.slope), T)
        return self._ref[key]

    def on(self, dev, ops, c: R.Case, prec: int):
        """device operands: (x, x2, weight image of the arithmetic, scale, shift, residual at its base offset)"""
        if "x" not in self._dev:
            d = self._dev
            d["x"], d["x2"] = self.x.to(dev), None if self.x2 is None else self.x2.to(dev)
            d["w"] = self.w.to(dev)
            d["scale"], d["shift"] = (None if t is None else t.to(dev) for t in (self.scale, self.shift))
            d["res"] = None
            if self.res is not None:
                flat = torch.full((c.epi.res_shift + self.res.numel(),), FAR, device=dev)
                flat[c.epi.res_shift:] = self.res.to(dev).reshape(-1)
                d["res"] = flat[c.epi.res_shift:]
        d = self._dev
        if ("w", prec) not in d:
            d[("w", prec)] = (d["w"] if prec == R.F32 else ops.pack_conv_weight_bf16x3(d["w"]) if prec == R.BF16X3
                              else ops.pack_conv_weight_fp16x2(d["w"], self.exps[1]))
        return d["x"], d["x2"], d[("w", prec)], d["scale"], d["shift"], d["res"]


_OPERANDS = {}


def operands(c: R.Case) -> Operands:
    if c not in _OPERANDS:
        _OPERANDS[c] = Operands(c)
    return _OPERANDS[c]


def describe(ffi, c: R.Case, tile: int, prec: int, mode: int, exps=(0, 0)):
    d = ffi.make_conv_desc(N=c.N, H=c.H, W=c.W, in_pitch=c.in_pitch, segs=c.segs, Cout=c.Cout, out_pitch=c.out_pitch,
                           out_off=c.epi.out_off, KH=c.KH, KW=c.KW, stride=c.stride, pad_h=c.pad_h, pad_w=c.pad_w, act=c.epi.act,
                           slope=c.epi.slope, res_pitch=c.res_pitch if c.epi.res else 0, res_off=c.epi.res_off if c.epi.res else 0,
                           tile=tile, split_k=mode, precision=prec, src2=c.src2)
    assert (d.OH, d.OW) == (c.OH, c.OW)
    if prec == R.FP16X2:
        d.a_scale_exp, d.w_scale_exp = exps
    return d


# ----------------------------------------------------------------------------- CPU: the restatement itself
def test_restatement_matches_torch_conv2d_in_f64():
    for c in all_cases():
        o = operands(c)
        pre, y, T = o.ref(c, R.F32)

        def conv(x, x2, w):
            xg = R.gather_segments(x, c.segs).permute(0, 3, 1, 2)
            w1 = w[:, :c.K1].reshape(c.Cout, c.KH, c.KW, c.Cin).permute(0, 3, 1, 2)
            v = F.conv2d(xg, w1, None, c.stride, (c.pad_h, c.pad_w))
            if c.src2:
                c2, _, off2, s2, _, _ = c.src2
                v = v + F.conv2d(x2[..., off2:off2 + c2].permute(0, 3, 1, 2), w[:, c.K1:].reshape(c.Cout, c2, 1, 1), None, s2)[:, :, :c.OH, :c.OW]
            return v.permute(0, 2, 3, 1).reshape(c.M, c.Cout)

        x64, w64 = o.x.double(), o.w.double()
        x2_64 = None if o.x2 is None else o.x2.double()
        want, wantT = conv(x64, x2_64, w64), conv(x64.abs(), None if x2_64 is None else x2_64.abs(), w64.abs())
        if o.scale is not None:
            want, wantT = want * o.scale.double(), wantT * o.scale.double().abs()
        if o.shift is not None:
            want, wantT = want + o.shift.double(), wantT + o.shift.double().abs()
        if o.res is not None:
            r = o.res.double()[:, c.epi.res_off:c.epi.res_off + c.Cout]
            want, wantT = want + r, wantT + r.abs()
        e = c.epi
        want_y = {R.ACT_NONE: lambda v: v, R.ACT_PRELU: lambda v: F.prelu(v, torch.tensor([e.slope], dtype=torch.float64)),
                  R.ACT_RELU6: F.relu6, R.ACT_RELU: F.relu}[e.act](want)
        # (1e-13 is for operands of order one: a border case's rows are compared in units of their image's multiplier)
        unit = torch.tensor([1000.0 ** n if c.border else 1.0 for n in range(c.N)], dtype=torch.float64)
        unit = unit.repeat_interleave(c.OH * c.OW).view(-1, 1)
        torch.testing.assert_close(pre / unit, want / unit, rtol=1e-13, atol=1e-13, msg=c.name)
        torch.testing.assert_close(y / unit, want_y / unit, rtol=1e-13, atol=1e-13, msg=c.name)
        torch.testing.assert_close(T / unit, wantT / unit, rtol=1e-13, atol=1e-13, msg=c.name)
        # fp16x2: the floored T bounds the plain one
        assert bool((o.ref(c, R.FP16X2)[2] >= T * (1 - 1e-12)).all()), c.name


def test_relu6_cases_reach_both_clamps_on_the_reference():
    hit = 0
    for c in all_cases():
        if c.epi.act != R.ACT_RELU6:
            continue
        pre = operands(c).ref(c, R.F32)[0]
        assert float((pre > 6.0).double().mean()) >= 0.05 and float((pre < 0.0).double().mean()) >= 0.05, c.name
        hit += 1
    assert hit == 2


def test_reciprocal_split_is_exact_below_2_21():
    """The kernel comment "exact for k < 2^21" and the host check p.K < (1 << 21): (int)((k + 0.5f) * (1.0f / Cin)) == k / Cin at
    every chunk next to a multiple of Cin, for every Cin the library accepts up to 8192; the same split of the tap index by KW."""
    import numpy as np
    for cin in range(4, 8193, 4):
        assert R.reciprocal_split_mismatches(cin) == 0, cin
    seg = np.arange(0, (1 << 19) + 1, dtype=np.int64)
    for kw in range(1, 17):
        kh = ((seg.astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(kw))).astype(np.int32)
        assert int((kh != seg // kw).sum()) == 0, kw


def test_bars_follow_their_derivation():
    assert R.bar(R.F32, 288, 1) == 1.01 * (2 * 288 + 5) * R.U
    assert R.bar(R.BF16X3, 288, 3) == 1.01 * (12 * 288 + 3 + 7) * R.U
    assert R.bar(R.FP16X2, 288, 2) == 1.01 * (6 * 288 + 12 + 6) * R.U
    # fp16x2's split on torch's round-to-nearest-even fp16: |x - (hi + lo) / s| <= 2^-22 max(|x|, 2^-3 / s)
    x = torch.cat([torch.randn(1 << 16, generator=torch.Generator().manual_seed(1)) * 10.0 ** torch.arange(-6, 2).repeat(1 << 13),
                   torch.tensor([2.0 ** -3, 2.0 ** -14, 2.0 ** -24, 0.0])])
    for s in (1.0, 16.0, 2.0 ** -9):
        sx = x * s
        hi = sx.half().float()
        lo = (sx - hi).half().float()
        err = (x.double() - (hi.double() + lo.double()) / s).abs()
        assert bool((err <= 2.0 ** -22 * x.double().abs().clamp_min(R.FP16_FLOOR / s)).all())


# ----------------------------------------------------------------------------- CPU: the rules restated, and what the table reaches
def test_tile_table_matches_the_package():
    from two_stage_object_detection_amd import _ffi
    assert set(R.TILES) == set(_ffi.TILES)
    for t, row in R.TILES.items():
        assert (row.name, row.bm, row.dma, row.precs) == (_ffi.TILES[t].name, _ffi.TILES[t].rows, _ffi.TILES[t].dma, _ffi.TILES[t].precisions)
    assert len(R.PAIRS) == 42


def _reached(tile, prec, cus=R.FALLBACK_CUS):
    """{(gather path, epilogue path, body)} of the launches the table gives (tile, arithmetic)"""
    out = set()
    for c in R.cases_for(tile):
        for mode in R.schedules_for(tile):
            if not R.runs(c, tile, prec, mode):
                continue
            bodies = ("balanced",) if mode == -2 else R.make_sched(c, tile, prec, mode, cus).bodies
            for b in bodies:
                out.add((R.gather_path(c, tile, prec), R.epilogue_path(c), b))
    return out


@pytest.mark.parametrize("prec,tile", R.PAIRS, ids=PAIR_IDS)
def test_case_table_reaches_every_switch_of_every_pair(prec, tile):
    reached = _reached(tile, prec)
    row = R.TILES[tile]
    for body in ("whole", "combine"):
        for epi in ("vec", "scalar"):
            assert any(r[1:] == (epi, body) for r in reached), (epi, body)
        for path in (("dma",) if row.dma else ("uniform", "table", "generic")):
            assert any(r[0] == path and r[2] == body for r in reached), (path, body)
    if row.dma:
        assert any(r[2] == "balanced" for r in reached)
        border = [c for c in R.cases_for(tile) if c.border and c.KH * c.KW > 1 and c.N > 1 and R.gather_path(c, tile, prec) == "dma"]
        assert border, "no multi-tap filter across a batch border on the tap form"
        if prec == R.FP16X2:
            assert any(r[0] == "dma_chan" for r in reached)
    # every scalar trigger of epilogue_path's table is in the cases, and is scalar for its own reason alone
    for e in R.SCALAR_TRIGGERS:
        mended = e._replace(out_extra=4 if e.out_extra else 0, out_off=0, res_extra=4 if e.res_extra else 0, res_off=0,
                            out_shift=0, res_shift=0)
        assert R.epilogue_path(R.G1._replace(epi=e)) == "scalar" and R.epilogue_path(R.G1._replace(epi=mended)) == "vec", e.name
    # the launches the rules give this pair, pinned (the GPU test asserts that exactly these run): 38 cases (40 with 64-float steps) x 4
    # schedules on a register-staged tile, less G12-96 where 96 channels are no whole K-step; on an LDS-DMA tile 5 schedules of
    # the cases it accepts and, in fp16x2, 4 of G6-2048; d64x128k64 accepts G2, G12, its own two G10 cases and G6-2048
    want = 24 if row.bk == 64 and row.dma else 156 if row.bk == 64 else 152 if not row.dma else 110 + 4 * (prec == R.FP16X2)
    assert R.predicted_runs(tile, prec) == want


def test_gather_path_examples():
    """The switches the issue names, one line each."""
    assert R.gather_path(R.G1, 3) == "uniform" and R.gather_path(R.G1, 10) == "generic" and R.gather_path(R.G1, 17, R.BF16X3) == "dma"
    assert R.gather_path(R.G1, 24, R.FP16X2) == "unsupported"
    by = {c.name: c for c in R.FIXED_GEOMETRY}
    assert R.gather_path(by["G6-2048"], 8) == "table" and R.gather_path(by["G6-2052"], 8) == "generic"
    assert R.gather_path(by["G6-2048"], 17, R.FP16X2) == "dma_chan" and R.gather_path(by["G6-2052"], 17, R.FP16X2) == "unsupported"
    assert R.gather_path(by["G6-2048"], 17, R.BF16X3) == "unsupported"
    assert R.gather_path(by["G9"], 3) == "generic" and R.gather_path(by["G4"], 3) == "generic"
    assert R.gather_path(by["G12"], 10) == "uniform" and R.gather_path(by["G12"], 22, R.BF16X3) == "dma"
    assert R.epilogue_path(R.G1) == "vec" and R.epilogue_path(R.G3) == "scalar"


@pytest.mark.parametrize("prec,tile", R.PAIRS, ids=PAIR_IDS)
def test_restated_scheduler_matches_the_resolver(prec, tile):
    """tsod_conv2d_resolve and tsod_conv2d_workspace_bytes need no device (the CU count falls back to 256): the named tile comes
    back with the restated schedule and workspace, or TSOD_ERR_UNSUPPORTED exactly where gather_path says so."""
    from two_stage_object_detection_amd import _ffi
    lib = _ffi.lib()
    cus = lib.tsod_device_cu_count() if torch.cuda.is_available() else R.FALLBACK_CUS
    for c in R.FIXED_GEOMETRY + R.tile_geometry(*R.TILES[tile][1:4]) + (R.hybrid_case(tile, prec, cus),):
        for mode in R.SCHEDULES:
            d = describe(_ffi, c, tile, prec, mode)
            got_tile, got_split = ctypes.c_int32(-1), ctypes.c_int32(0)
            rc = lib.tsod_conv2d_resolve(ctypes.byref(d), ctypes.byref(got_tile), ctypes.byref(got_split))
            ws = lib.tsod_conv2d_workspace_bytes(ctypes.byref(d))
            if not R.runs(c, tile, prec, mode):
                assert (rc, ws) == (ERR_UNSUPPORTED, 0), (c.name, mode)
                continue
            s = R.make_sched(c, tile, prec, mode, cus)
            assert (rc, got_tile.value, got_split.value, ws) == (0, tile, s.reported_split_k, s.ws_bytes), (c.name, mode, s)
    h = R.make_sched(R.hybrid_case(tile, prec, cus), tile, prec, -1, cus)
    if R.TILES[tile].bk <= 32:        # (K = 128 in 64-float steps: a slice would be one K-step, the hybrid launch keeps whole tiles)
        assert 0 < h.dp_tiles < h.tiles and h.bodies == ("whole", "combine")


# ----------------------------------------------------------------------------- GPU: one launch, checked
_WORST = {}


def note(prec, tile, path, body, mode, ratio):
    key = (R.PREC_NAMES[prec], "dma" if R.TILES[tile].dma else "reg", path, body, mode)
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    path = os.environ.get("TSOD_CONV_KERNELS_JSONL")
    for (arith, family, gpath, body, mode), ratio in sorted(_WORST.items()):
        line = {"arithmetic": arith, "tile_family": family, "gather": gpath, "epilogue": body, "split_k": mode,
                "max_err_over_bar": round(ratio, 5), "commit": os.environ.get("TSOD_CONV_KERNELS_COMMIT", "unknown")}
        print("conv_kernels:", json.dumps(line))
        if path:
            with open(path, "a") as f:
                f.write(json.dumps(line) + "\n")


def launch(ffi, ops, dev, c, tile, prec, mode, words=None):
    """One call of tsod_conv2d_dual_f32 into a SENTINEL-filled buffer with a guard row -> (rc, flat buffer, [M + 1, pitch] view)"""
    o = operands(c)
    x, x2, w, scale, shift, res = o.on(dev, ops, c, prec)
    d = describe(ffi, c, tile, prec, mode, o.exps)
    if words is not None:
        d.amax_out = words.data_ptr()
    flat = torch.full((c.epi.out_shift + (c.M + 1) * c.out_pitch,), SENTINEL, device=dev)
    out = flat[c.epi.out_shift:]
    ws_bytes = ffi.lib().tsod_conv2d_workspace_bytes(ctypes.byref(d))
    ws = ops.CONV_ARENA.get(dev, ws_bytes) if ws_bytes else None
    rc = ffi.lib().tsod_conv2d_dual_f32(ctypes.byref(d), ffi.ptr(x), ffi.ptr(x2) or None, ffi.ptr(w), ffi.ptr(scale) or None,
                                        ffi.ptr(shift) or None, ffi.ptr(res) or None, ffi.ptr(out), ffi.ptr(ws) or None, ws_bytes,
                                        ffi.stream_ptr())
    return rc, flat, out.view(c.M + 1, c.out_pitch)


def slices_of(c, tile, prec, mode, cus):
    """[(epilogue body, S of its bar, mask [M, Cout] of the outputs that body stores)] of a launch"""
    everything = torch.ones((c.M, c.Cout), dtype=torch.bool)
    t = R.TILES[tile]
    if mode == -2:                    # balanced K ranges: a workgroup holds >= 4 K-steps, so a tile has at most ksteps / 4 + 2 holders
        return [("balanced", -(-c.K // t.bk) // 4 + 2, everything)]
    s = R.make_sched(c, tile, prec, mode, cus)
    if len(s.bodies) == 1:
        return [(s.bodies[0], s.split, everything)]
    # a mixed launch: tile_id = row tile * tiles_n + channel tile, the first dp_tiles of them whole (work_item)
    tile_id = (torch.arange(c.M) // t.bm).view(-1, 1) * s.tiles_n + (torch.arange(c.Cout) // t.bn).view(1, -1)
    whole = tile_id < s.dp_tiles
    return [("whole", 1, whole), ("combine", s.split, ~whole)]


def run_and_check(ffi, ops, dev, c, tile, prec, mode, cus, words=False):
    """Launch twice; every check of the module docstring.  Returns the stored slice (host, [M, Cout]) and the range words' value."""
    if not R.runs(c, tile, prec, mode):
        rc, flat, _ = launch(ffi, ops, dev, c, tile, prec, mode)
        assert rc == ERR_UNSUPPORTED, (c.name, mode, rc)
        assert bool((flat == SENTINEL).all())
        return None, None, ()
    w1 = ops.new_amax_words(dev, 1) if words else None
    rc, flat, rows = launch(ffi, ops, dev, c, tile, prec, mode, w1)
    assert rc == 0, (c.name, mode, rc)
    rc2, flat2, _ = launch(ffi, ops, dev, c, tile, prec, mode)
    assert rc2 == 0 and torch.equal(flat, flat2), (c.name, mode, "two launches differ")
    e = c.epi
    host = rows.cpu()
    got = host[:c.M, e.out_off:e.out_off + c.Cout].clone()
    assert bool((got != SENTINEL).all()), (c.name, mode, "an output was not written")
    host[:c.M, e.out_off:e.out_off + c.Cout] = SENTINEL
    assert bool((host == SENTINEL).all()) and bool((flat[:e.out_shift] == SENTINEL).all()), (c.name, mode, "a byte outside the slice changed")
    pre, y, T = operands(c).ref(c, prec)
    bodies = slices_of(c, tile, prec, mode, cus)
    lim = torch.zeros_like(T)
    for _, S, mask in bodies:         # (every output belongs to exactly one body)
        lim = torch.where(mask, R.bar(prec, c.K, S) * T, lim)
    err = (got.double() - y).abs()
    rel = err / lim.clamp_min(1e-300)
    assert bool((err <= lim).all()), (c.name, R.TILES[tile].name, mode, "err / (bar T) =", float(rel.max()))
    if e.act == R.ACT_RELU6:          # at the clamps the stored value is the clamp itself
        assert bool((got[pre > 6.0 + lim] == 6.0).all()) and bool((got[pre < -lim] == 0.0).all()), (c.name, mode)
    for b, _, mask in bodies:         # each body's figure is over the outputs it stored
        note(prec, tile, R.gather_path(c, tile, prec), f"{b}/{R.epilogue_path(c)}", mode, float(rel[mask].max()))
    return got, (ops.amax_value(w1) if words else None), tuple(b for b, _, _ in bodies)


@gpu
@pytest.mark.parametrize("prec,tile", R.PAIRS, ids=PAIR_IDS)
def test_conv_tile_at_every_switch(ffi, ops, dev, prec, tile):
    cus = ffi.lib().tsod_device_cu_count()
    ran = 0
    for c in R.cases_for(tile):
        for mode in R.schedules_for(tile):
            got, _, _ = run_and_check(ffi, ops, dev, c, tile, prec, mode, cus)
            ran += got is not None
    assert ran == R.predicted_runs(tile, prec)


FOUR_BODIES = {(b, e) for b in ("whole", "combine") for e in ("vec", "scalar")}


def range_word_tiles(prec):
    """one register-staged tile, and one LDS-DMA tile where the arithmetic has any"""
    return (8,) + ((17,) if prec != R.F32 else ())


def range_word_cases():
    """G1's geometry (32 channels: whole K-steps of both tiles) with vector stores (a plain slice at out_off 12; scale, shift,
    residual at res_off 8 and PReLU) and with scalar stores (out_off = 2; a residual at res_off = 2)"""
    triggers = {e.name: e for e in R.SCALAR_TRIGGERS}
    epis = (R.EPILOGUES[5], R.EPILOGUES[2], triggers["out_off=2"], triggers["res_off=2"])
    return tuple(R.G1._replace(name=f"G1/{e.name}/words", epi=e, border=False) for e in epis)


@pytest.mark.parametrize("prec", (R.F32, R.BF16X3, R.FP16X2), ids=("f32", "bf16x3", "fp16x2"))
def test_range_word_cases_reach_the_four_bodies_on_each_tile(prec):
    for tile in range_word_tiles(prec):
        seen = set()
        for c in range_word_cases():
            for mode in (1, 2):
                assert R.runs(c, tile, prec, mode)
                seen |= {(b, R.epilogue_path(c)) for b in R.make_sched(c, tile, prec, mode).bodies}
        assert seen == FOUR_BODIES, (tile, seen)
    assert [R.TILES[t].dma for t in range_word_tiles(R.FP16X2)] == [False, True]


@gpu
@pytest.mark.parametrize("prec", (R.F32, R.BF16X3, R.FP16X2), ids=("f32", "bf16x3", "fp16x2"))
def test_conv_range_words_hold_the_stored_abs_max(ffi, ops, dev, prec):
    """amax_out after a launch == the abs-max of the slice it stored, bit for bit, under each of the four epilogue bodies (the
    SENTINEL neighbours of the slice are not counted)."""
    cus = ffi.lib().tsod_device_cu_count()
    for tile in range_word_tiles(prec):
        seen = set()
        for c in range_word_cases():
            for mode in (1, 2):       # whole tile / last-arriver combine
                assert R.runs(c, tile, prec, mode), (c.name, tile, mode)
                got, amax, bodies = run_and_check(ffi, ops, dev, c, tile, prec, mode, cus, words=True)
                assert bodies == (("whole",) if mode == 1 else ("combine",))
                assert amax == float(got.abs().max()) > 0, (c.name, tile, mode)
                seen.add((bodies[0], R.epilogue_path(c)))
        assert seen == FOUR_BODIES, (tile, seen)


@gpu
@pytest.mark.parametrize("prec,tile", ((R.F32, 3), (R.BF16X3, 8), (R.FP16X2, 8)), ids=("f32-64x64", "bf16x3-64x64s1", "fp16x2-64x64s1"))
def test_conv_mixed_hybrid_launch(ffi, ops, dev, prec, tile):
    """split_k = -1 with more tiles than CU slots: whole tiles and K-sliced tiles in one grid (both branches of work_item, the
    ticket index tile_id - dp_tiles).  The shape comes from the restated scheduler at the device's CU count.  A tile written
    twice by different workgroups, or not at all, shows as a SENTINEL left in the slice, a run-to-run difference or an error."""
    cus = ffi.lib().tsod_device_cu_count()
    c = R.hybrid_case(tile, prec, cus)
    s = R.make_sched(c, tile, prec, -1, cus)
    assert 0 < s.dp_tiles < s.tiles and s.split == 2 and c.K == 128
    got, _, bodies = run_and_check(ffi, ops, dev, c, tile, prec, -1, cus)
    assert got is not None and bodies == ("whole", "combine")
    _OPERANDS.pop(c, None)            # (the one large case: its operands are not kept)
