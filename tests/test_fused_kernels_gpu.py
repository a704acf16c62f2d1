"""The one-launch stem (csrc/stem_fused.hip) and the one-launch bottleneck (csrc/bottleneck_fused.hip) against the float64
restatements of tests/fused_restated.py, per element:  |got - y| <= E  with E derived there - at every tile geometry, channel
count, pixel pitch, BatchNorm sign, slope and scale the kernels switch on, and for the stem at one, two and three rounds of its
persistent tile loop.  Sentinels, zero tiles, bit identities and the range words are checked for exact equality.

The unmarked tests run on any machine: the restatements against F.conv2d / F.max_pool2d chains, a CPU emulation of the kernels'
arithmetic inside E on every case (the reference alone meets the bar), the same emulation with three planted faults outside E
(the bar bites), the launchers' rules against the source text, and every case's claim about its tile height and round count.

With TSOD_FUSED_KERNELS_JSONL=<path> the largest err / E of every (kernel, form, case) is appended to that file, one JSON line
each (TSOD_FUSED_KERNELS_COMMIT names the commit in them)."""
import json
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_restated as R  # noqa: E402
import fused_restated as Z  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "two_stage_object_detection_amd", "csrc")
gpu = pytest.mark.gpu
SENTINEL = -7.25
CU_COUNTS = (256, 304)
B_NAMES = [c.name for c in Z.bottleneck_cases(256)]
S_NAMES = [c.name for c in Z.stem_cases(256)]


@pytest.fixture(scope="module")
def ops():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ----------------------------------------------------------------------------- operands and references, once per case
_CACHE = {}


def b_ref(c: Z.BCase):
    """(inputs, y, E) of a bottleneck case at the tile height its label claims"""
    if c not in _CACHE:
        i = Z.bottleneck_inputs(c)
        y, E = Z.bottleneck_ref(i["x"], i["w1"], i["w2"], i["w3"], i["bn"], c.slope, wd=i["wd"], bnd=i["bnd"], e_x=i["e_x"], TH=c.th)
        _CACHE[c] = (i, y, E)
    return _CACHE[c]


def b_emulate(c: Z.BCase, fault=None):
    i = b_ref(c)[0]
    return Z.bottleneck_emulate(i["x"], i["w1"], i["w2"], i["w3"], i["bn"], c.slope, wd=i["wd"], bnd=i["bnd"], e_x=i["e_x"], TH=c.th,
                                fault=fault)


def s_ref(c: Z.SCase):
    if c not in _CACHE:
        i = Z.stem_inputs(c)
        y, E = Z.stem_ref(i["x"], i["w"], i["scale"], i["shift"], c.slope)
        _CACHE[c] = (i, y, E)
    return _CACHE[c]


def s_emulate(c: Z.SCase, fault=None):
    i = s_ref(c)[0]
    return Z.stem_emulate(i["x"], i["w"], i["scale"], i["shift"], c.slope, fault=fault)


def ratio(got, y, E):
    return float(((got.double() - y).abs() / E.clamp_min(1e-300)).max())


def by_name(cases, name):
    return next(c for c in cases if c.name == name)


# ----------------------------------------------------------------------------- CPU: the restatements themselves
def _v4(v):
    return v.double().view(1, -1, 1, 1)


@pytest.mark.parametrize("proj", (False, True), ids=("identity", "projection"))
def test_bottleneck_restatement_matches_a_torch_chain_in_f64(proj):
    for N, H, W, Cin, Cout in ((2, 5, 7, 64, 128 if proj else 64), (1, 9, 17, 128, 64 if proj else 128)):
        c = Z.BCase("chain", N, H, W, Cin, Cout, proj, bn="mixed")
        i = Z.bottleneck_inputs(c)
        y, E = Z.bottleneck_ref(i["x"], i["w1"], i["w2"], i["w3"], i["bn"], c.slope, wd=i["wd"], bnd=i["bnd"], e_x=i["e_x"], TH=8)
        s1, b1, s2, b2, s3, b3 = i["bn"]
        act = lambda t: F.prelu(t, torch.tensor([c.slope], dtype=torch.float64))      # noqa: E731
        x = i["x"].double().permute(0, 3, 1, 2)
        v = act(F.conv2d(x, i["w1"].double().view(64, Cin, 1, 1)) * _v4(s1) + _v4(b1))
        v = act(F.conv2d(v, i["w2"].double().permute(0, 3, 1, 2), padding=1) * _v4(s2) + _v4(b2))
        if proj:
            ws, bs = Z.stack_projection(i["w3"], s3, i["wd"], i["bnd"][0], b3, i["bnd"][1])
            want = act(F.conv2d(torch.cat([v, x], dim=1), ws.double().view(Cout, 64 + Cin, 1, 1)) + _v4(bs))
        else:
            want = act(F.conv2d(v, i["w3"].double().view(Cout, 64, 1, 1)) * _v4(s3) + _v4(b3) + x)
        torch.testing.assert_close(y, want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
        assert bool((E > 0).all()) and bool(torch.isfinite(E).all())
        y10 = Z.bottleneck_ref(i["x"], i["w1"], i["w2"], i["w3"], i["bn"], c.slope, wd=i["wd"], bnd=i["bnd"], e_x=i["e_x"], TH=10)[0]
        torch.testing.assert_close(y10, y, rtol=1e-12, atol=1e-12)          # (the tile height only enters E)


def test_stem_restatement_matches_a_torch_chain_in_f64():
    for N, H, W in ((2, 9, 11), (1, 17, 65), (1, 18, 66), (1, 1, 1)):
        c = Z.SCase("chain", N, H, W, bn="mixed")
        i = Z.stem_inputs(c)
        y, E = Z.stem_ref(i["x"], i["w"], i["scale"], i["shift"], c.slope)
        v = F.conv2d(i["x"].double(), i["w"].double(), stride=2, padding=3) * _v4(i["scale"]) + _v4(i["shift"])
        want = F.max_pool2d(F.prelu(v, torch.tensor([c.slope], dtype=torch.float64)), 3, 2, 1)
        torch.testing.assert_close(y, want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
        assert tuple(y.shape[1:3]) == Z.stem_out_hw(H, W)[2:]
        # E is the pooled bound of the conv: F.max_pool2d of bar * T over the same windows, for a one-tile image with one exponent
        if Z.stem_launch(N, H, W, 256).tiles == N:
            f = R.FP16_FLOOR / 2.0 ** Z.exp_from_max(float(i["x"].abs().max()))
            mw = i["w"].double().abs().clamp_min(R.FP16_FLOOR / 2.0 ** Z.weight_exp(i["w"]))
            # (max(|x|, f) inside the image, 0 in the padding)
            T = F.conv2d(i["x"].double().abs().clamp_min(f), mw, stride=2, padding=3) * _v4(i["scale"]).abs() + _v4(i["shift"]).abs()
            if N == 1 or all(Z.exp_from_max(float(i["x"][n].abs().max())) == Z.exp_from_max(float(i["x"].abs().max())) for n in range(N)):
                torch.testing.assert_close(E, F.max_pool2d(R.bar(R.FP16X2, 147) * T, 3, 2, 1).permute(0, 2, 3, 1), rtol=1e-12, atol=0)


def test_exponent_rule_restates_the_kernels():
    with open(os.path.join(CSRC, "tsod_internal.h")) as f:
        src = f.read()
    assert re.search(r"const int e = 141 - \(int\)\(bits >> 23\);", src) and "return e < -24 ? -24 : (e > 24 ? 24 : e);" in src
    for m, e in ((1.0, 14), (1.999, 14), (2.0, 13), (16384.0, 0), (32767.0, 0), (32768.0, -1), (0.0, 24), (2.0 ** -30, 24),
                 (math.inf, -24), (2.0 ** 60, -24)):
        assert Z.exp_from_max(m) == e, m
        if 0.0 < m < math.inf:                          # the bits of the f32, as the kernel reads them
            bits = torch.tensor(m, dtype=torch.float32).view(torch.int32).item()
            assert max(-24, min(24, 141 - (bits >> 23))) == e


# ----------------------------------------------------------------------------- CPU: the launch rules, pinned to the source
def test_bottleneck_tile_height_rule_restates_the_launcher():
    with open(os.path.join(CSRC, "bottleneck_fused.hip")) as f:
        src = f.read()
    assert "constexpr int TW = 16, HW_ = TW + 2;" in src
    assert "return (double)((tiles + 2 * cus - 1) / (2 * cus)) * mfma_slowest;" in src
    assert "const int64_t tiles = (int64_t)d->N * ((d->W + TW - 1) / TW) * ((d->H + th - 1) / th);" in src
    assert "const int n1 = d->Cin / 32, nq = d->Cout / 64, c3 = proj ? 4 + 2 * n1 : 4;" in src
    m = re.search(r"const int TH = cost\(8, ([0-9n1c3q*+() ]+)\) < cost\(10, ([0-9n1c3q*+() ]+)\) \? 8 : 10;", src)
    assert m, "the tile height rule changed: restate it in fused_restated.bottleneck_tile_height"
    for Cin, Cout, proj in ((64, 64, False), (256, 256, False), (64, 256, True), (128, 64, True), (256, 128, True), (64, 192, True)):
        names = dict(n1=Cin // 32, nq=Cout // 64, c3=4 + 2 * (Cin // 32) if proj else 4)
        assert eval(m.group(1), {}, names) == Z.bottleneck_wave_mfmas(8, Cin, Cout, proj)
        assert eval(m.group(2), {}, names) == Z.bottleneck_wave_mfmas(10, Cin, Cout, proj)
    # the figures of the kernel's header comment: 456 MFMAs for 128 pixels, 660 for 160 (Cin = Cout = 256)
    assert (Z.bottleneck_wave_mfmas(8, 256, 256, False), Z.bottleneck_wave_mfmas(10, 256, 256, False)) == (456, 660)
    # the rule at its switch: 8 rows while both tilings take the same rounds, 10 once only the 8-row tiling needs a second
    assert Z.bottleneck_tile_height(1, 40, 16 * 102, 64, 64, False, 256) == 8          # 510 / 408 tiles on 512 slots
    assert Z.bottleneck_tile_height(1, 40, 16 * 103, 64, 64, False, 256) == 10         # 515 / 412
    assert Z.bottleneck_tile_height(1, 40, 16 * 128, 64, 64, False, 256) == 10         # 640 / 512
    assert Z.bottleneck_tile_height(1, 40, 16 * 129, 64, 64, False, 256) == 8          # 645 / 516: two rounds either way


def test_stem_launch_rule_restates_the_launcher():
    with open(os.path.join(CSRC, "stem_fused.hip")) as f:
        src = f.read()
    assert "constexpr int TPH = 4, TPW = 16;" in src
    assert "constexpr int IH = 2 * CH + 5, IW = 2 * CW + 5;" in src and "constexpr int CH = 2 * TPH + 1, CW = 2 * TPW + 1;" in src
    assert (2 * (2 * Z.TPH + 1) + 5, 2 * (2 * Z.TPW + 1) + 5) == (Z.PATCH_H, Z.PATCH_W)
    assert "const int i0y = 4 * tl.p0y - 5, i0x = 4 * tl.p0x - 5;" in src
    assert "p.tiles_x = (p.PW + TPW - 1) / TPW; p.tiles_y = (p.PH + TPH - 1) / TPH;" in src
    assert "const int64_t tiles = (int64_t)d->N * p.tiles_x * p.tiles_y;" in src
    assert "const int64_t slots = 2 * (int64_t)cus, rounds = (tiles + slots - 1) / slots;" in src
    assert "const int64_t grid = (tiles + rounds - 1) / rounds;" in src
    assert "for (; t < n_tiles; t += nwg) {" in src
    assert Z.stem_launch(1, 200, 336, 256) == Z.StemLaunch(6, 13, 78, 512, 1, 78)
    assert Z.stem_launch(513, 5, 6, 256) == Z.StemLaunch(1, 1, 513, 512, 2, 257)
    assert Z.stem_launch(1027, 5, 6, 256) == Z.StemLaunch(1, 1, 1027, 512, 3, 343)
    assert Z.stem_launch(1, 800, 1333, 256)[2:] == (1050, 512, 3, 350)


@pytest.mark.parametrize("n_cus", CU_COUNTS)
def test_every_case_reaches_the_path_its_label_claims(n_cus):
    heights, forms = set(), set()
    for c in Z.bottleneck_cases(n_cus):
        assert Z.bottleneck_tile_height(c.N, c.H, c.W, c.Cin, c.Cout, c.proj, n_cus) == c.th, c.name
        assert Z.bottleneck_rounds(c.th, c.N, c.H, c.W, n_cus) == c.rounds, c.name
        assert c.Cin % 64 == 0 and c.Cout % 64 == 0 and (c.proj or c.Cin == c.Cout)
        heights.add(c.th)
        forms.add((c.th, c.proj))
    assert forms == {(8, False), (8, True), (10, False), (10, True)}
    # the ten-row case: the 8-row tiling would need two rounds
    t = Z.ten_row_case(n_cus, False)
    assert Z.bottleneck_rounds(8, t.N, t.H, t.W, n_cus) == 2 and Z.bottleneck_rounds(10, t.N, t.H, t.W, n_cus) == 1
    # 8 and 9 workgroups: both sides of the XCD order's remainder; fewer workgroups than XCDs
    names = {c.name.split("/")[0]: c for c in Z.bottleneck_cases(n_cus)}
    assert [-(-names[k].W // 16) for k in ("geo-1x8x128", "geo-1x8x144")] == [8, 9] and names["geo-3x5x5"].N == 3
    rounds = set()
    for c in Z.stem_cases(n_cus):
        L = Z.stem_launch(c.N, c.H, c.W, n_cus)
        assert L.rounds == c.rounds, c.name
        rounds.add(L.rounds)
        if c.name == "rounds-2/images":
            assert L.tiles == 2 * n_cus + 1 and L.tiles - L.grid == L.grid - 1       # the last workgroup owns a single tile
        if c.name == "rounds-2/column":
            assert (L.tiles_x, L.tiles_y) == (1, 2 * n_cus + 2)
    assert rounds == {1, 2, 3}


# ----------------------------------------------------------------------------- CPU: the emulation inside E, the faults outside
@pytest.mark.parametrize("name", B_NAMES)
def test_bottleneck_emulation_stays_within_E(name):
    c = by_name(Z.bottleneck_cases(256), name)
    _, y, E = b_ref(c)
    r = ratio(b_emulate(c), y, E)
    print(f"bottleneck emulation {name}: max err / E = {r:.4f}")
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("name", S_NAMES)
def test_stem_emulation_stays_within_E(name):
    c = by_name(Z.stem_cases(256), name)
    _, y, E = s_ref(c)
    r = ratio(s_emulate(c), y, E)
    print(f"stem emulation {name}: max err / E = {r:.4f}")
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("fault", Z.FAULTS)
def test_a_planted_fault_exceeds_E(fault):
    """x zero-padded instead of y1, one cross product dropped, the low piece dropped on halo rows: each leaves E on some case"""
    caught = {}
    for c in Z.bottleneck_cases(256):
        if c.th == 8 and c.Cin == 64:                                    # (the small cases are enough)
            _, y, E = b_ref(c)
            r = ratio(b_emulate(c, fault), y, E)
            if r > 1.0:
                caught[c.name] = round(r, 2)
    print(f"fault {fault}: caught on {caught}")
    assert caught, fault
    assert any(n.startswith("aligned/") for n in caught) or fault == "pad_x"
    if fault == "pad_x":                                                 # every case with a non-zero b1 at an image border
        assert len(caught) >= 20


def test_a_dropped_cross_product_exceeds_E_on_the_stem():
    wide = by_name(Z.stem_cases(256), "geo-2x18x66")
    i = dict(s_ref(wide)[0])
    # aligned data: one positive constant with a full low piece for pixels and weights - every product's error has one sign
    i["x"] = torch.full_like(i["x"], Z.ALIGNED)
    i["w"] = torch.full_like(i["w"], Z.ALIGNED / 16.0)
    i["scale"], i["shift"] = i["scale"].abs(), torch.zeros(64)
    y, E = Z.stem_ref(i["x"], i["w"], i["scale"], i["shift"], wide.slope)
    ok = Z.stem_emulate(i["x"], i["w"], i["scale"], i["shift"], wide.slope)
    bad = Z.stem_emulate(i["x"], i["w"], i["scale"], i["shift"], wide.slope, fault="drop_cross")
    assert ratio(ok, y, E) <= 1.0 < ratio(bad, y, E)


# ----------------------------------------------------------------------------- GPU: recording
_WORST = {}


def note(kernel, form, case, path, r):
    _WORST[(kernel, form, case, path)] = max(_WORST.get((kernel, form, case, path), 0.0), float(r))


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    path = os.environ.get("TSOD_FUSED_KERNELS_JSONL")
    for (kernel, form, case, p), r in sorted(_WORST.items()):
        line = {"kernel": kernel, "form": form, "case": case, ("tile_rows" if kernel == "bottleneck" else "rounds"): p,
                "max_err_over_bar": float(f"{r:.3g}"), "commit": os.environ.get("TSOD_FUSED_KERNELS_COMMIT", "unknown")}
        print("fused_kernels:", json.dumps(line))
        if path:
            with open(path, "a") as f:
                f.write(json.dumps(line) + "\n")


# ----------------------------------------------------------------------------- GPU: the bottleneck
def set_words(ops, dev, value):
    """range words holding ``value`` in word 0 (the kernel takes the largest word)"""
    w = ops.new_amax_words(dev, 1)
    w.view(torch.float32)[0, 0] = value
    return w


class BLaunch:
    """device operands of a bottleneck case; ``run`` launches into a SENTINEL-filled buffer"""

    def __init__(self, ops, dev, c, i):
        self.ops, self.dev, self.c, self.i = ops, dev, c, i
        x = torch.full((c.N, c.H, c.W, c.Cin + c.in_extra), float("nan"))
        x[..., :c.Cin] = i["x"]
        self.x = x.to(dev)
        s1, b1, s2, b2, s3, b3 = i["bn"]
        if c.proj:
            w3, bs = Z.stack_projection(i["w3"], s3, i["wd"], i["bnd"][0], b3, i["bnd"][1])
            bn = [s1, b1, s2, b2, torch.ones(c.Cout), bs]
        else:
            w3, bn = i["w3"], i["bn"]
        self.stream, self.exps = ops.pack_bottleneck_wstream(i["w1"].to(dev), i["w2"].to(dev), w3.contiguous().to(dev), projection=c.proj)
        assert tuple(self.exps) == (Z.weight_exp(i["w1"]), Z.weight_exp(i["w2"]), Z.weight_exp(w3))
        self.bn = torch.cat(bn).float().to(dev)

    def run(self, x=None, *, words="case", static=None, seed_out=None, n=None):
        """-> (out [N, H, W, out_pitch] on the host, flag, the value amax_out holds).  ``words``: "case" (the case's own range
        words or static exponent), a float (range words holding it) or None with ``static``; ``n``: only the first n images"""
        c, ops, dev = self.c, self.ops, self.dev
        x = self.x if x is None else x
        if n is not None:
            x = x[:n].contiguous()
        out = torch.full((x.shape[0], c.H, c.W, c.Cout + c.out_extra), SENTINEL, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        wout = ops.new_amax_words(dev, 1) if seed_out is None else set_words(ops, dev, seed_out)
        kw = dict(cin=c.Cin) if c.proj else {}
        if words == "case":
            words, static = (None, c.static) if c.static is not None else (self.i["words_max"], None)
        if words is not None:
            kw["amax_in"] = set_words(ops, dev, words)
        else:
            kw["a_scale_exp"] = static
        ops.bottleneck_fused(x, self.stream, self.exps, self.bn, c.Cout, c.slope, out=out, amax_out=wout, range_flag=flag, **kw)
        return out.cpu(), int(flag.item()), ops.amax_value(wout)


def check_stored(c_out, extra, host):
    """-> the stored channels; every float of the pad channels must still hold SENTINEL's bits"""
    got = host[..., :c_out]
    assert bool((host[..., c_out:] == SENTINEL).all()), "a pad channel of the output was written"
    assert host.shape[-1] == c_out + extra and bool(torch.isfinite(got).all())
    return got


@gpu
@pytest.mark.parametrize("name", B_NAMES)
def test_bottleneck_case(ops, dev, cus, name):
    c = by_name(Z.bottleneck_cases(cus), name)
    assert Z.bottleneck_tile_height(c.N, c.H, c.W, c.Cin, c.Cout, c.proj, cus) == c.th, "the case does not reach its tile height here"
    i, y, E = b_ref(c)
    L = BLaunch(ops, dev, c, i)
    host, flag, amax = L.run()
    got = check_stored(c.Cout, c.out_extra, host)
    r = ratio(got, y, E)
    print(f"bottleneck {c.form} {name} (TH = {c.th}): max err / E = {r:.4f}")
    assert flag == 0, "NaN pad channels or in-range data raised the flag"
    assert r <= 1.0, (name, r)
    note("bottleneck", c.form, name, c.th, r)
    assert amax == float(got.abs().max()), "amax_out is not the largest stored magnitude"
    host2, flag2, amax2 = L.run()
    assert torch.equal(host, host2) and (flag2, amax2) == (flag, amax), "two runs differ"
    if c.x == "zero_tile" and not c.shifts:
        # tile (0, 1) and its halo are zeros and so are b1, b2: y1 = y2 = 0 and the tile's output is PReLU(b3 + x) = PReLU(b3) exactly
        b3 = L.bn[-c.Cout:].cpu()
        want = torch.clamp(b3, min=0) + torch.tensor(c.slope) * torch.clamp(b3, max=0)
        assert torch.equal(got[0, 0:8, 16:32], want.expand(8, 16, c.Cout))
    if c.static is not None:
        # tile-local and static scales only: an image's bits do not depend on the batch it is in
        assert Z.bottleneck_tile_height(1, c.H, c.W, c.Cin, c.Cout, c.proj, cus) == c.th
        one, _, _ = L.run(n=1)
        assert torch.equal(one[0], host[0])
        one, _, _ = L.run(x=L.x[1:2].contiguous())
        assert torch.equal(one[0], host[1])


@gpu
@pytest.mark.parametrize("proj", (False, True), ids=("identity", "projection"))
def test_bottleneck_flag_and_range_words(ops, dev, cus, proj):
    c = by_name(Z.bottleneck_cases(cus), "geo-1x16x32/" + ("proj64-256" if proj else "id64"))
    i, y, E = b_ref(c)
    L = BLaunch(ops, dev, c, i)
    host, flag, amax = L.run()
    assert flag == 0
    # a static exponent that overflows fp16: 2^16 x is beyond 65504 for most of the tensor - only the flag says so
    assert float(i["x"].abs().max()) * 2.0 ** 16 > 65504.0
    assert L.run(words=None, static=16)[1] == 1
    # a static exponent that fits gives the reference again (E for e_x = 8 differs only in its floors: checked by the static-exp case)
    assert L.run(words=None, static=8)[1] == 0
    # non-finite input: first pixel, last pixel, and column 16 of row 3 - tile (0, 1)'s own pixel and nothing but halo to tile (0, 0)
    for bad in (float("inf"), float("nan")):
        for h, w, ch in ((0, 0, 0), (c.H - 1, c.W - 1, c.Cin - 1), (3, 16, 5)):
            xb = L.x.clone()
            xb[0, h, w, ch] = bad
            assert L.run(x=xb)[1] == 1, (bad, h, w)
    # range words seeded with more than the launch stores keep their value; seeded with less they take the launch's
    assert L.run(seed_out=2.0 * amax)[2] == 2.0 * amax
    assert L.run(seed_out=0.5 * amax)[2] == amax


# ----------------------------------------------------------------------------- GPU: the stem
class SLaunch:
    def __init__(self, ops, dev, c, i):
        self.ops, self.dev, self.c = ops, dev, c
        self.x = i["x"].to(dev)
        self.wfrag, self.e = ops.pack_stem_wfrag(i["w"].to(dev))
        assert self.e == Z.weight_exp(i["w"])
        self.bn = torch.cat([i["scale"], i["shift"]]).float().to(dev)

    def run(self, x=None, *, nhwc4=False, seed_out=None):
        from two_stage_object_detection_amd._ffi import NHWC4Images
        c, ops, dev = self.c, self.ops, self.dev
        x = self.x if x is None else x
        _, _, ph, pw = Z.stem_out_hw(c.H, c.W)
        out = torch.full((x.shape[0], ph, pw, 64 + c.out_extra), SENTINEL, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        wout = ops.new_amax_words(dev, 1) if seed_out is None else set_words(ops, dev, seed_out)
        if nhwc4:                                          # whatever sits in channel 3 is never read: NaN
            x4 = torch.full((x.shape[0], c.H, c.W, 4), float("nan"), device=dev)
            x4[..., :3] = x.permute(0, 2, 3, 1)
            x = NHWC4Images(x4)
        ops.stem_fused(x, self.wfrag, self.e, self.bn, c.slope, out=out, amax_out=wout, range_flag=flag)
        return out.cpu(), int(flag.item()), ops.amax_value(wout)


@gpu
@pytest.mark.parametrize("name", S_NAMES)
def test_stem_case(ops, dev, cus, name):
    c = by_name(Z.stem_cases(cus), name)
    launch = Z.stem_launch(c.N, c.H, c.W, cus)
    assert launch.rounds == c.rounds, "the case does not reach its round count here"
    i, y, E = s_ref(c)
    L = SLaunch(ops, dev, c, i)
    host, flag, amax = L.run()
    got = check_stored(64, c.out_extra, host)
    r = ratio(got, y, E)
    print(f"stem {name} ({launch.rounds} round(s), grid {launch.grid}): max err / E = {r:.4f}")
    assert flag == 0
    assert r <= 1.0, (name, r)
    note("stem", "nchw+nhwc4", name, launch.rounds, r)
    assert amax == float(got.abs().max()), "amax_out is not the largest stored magnitude"
    host2, flag2, amax2 = L.run()
    assert torch.equal(host, host2) and (flag2, amax2) == (flag, amax), "two runs differ"
    host4, flag4, amax4 = L.run(nhwc4=True)
    assert torch.equal(host, host4) and (flag4, amax4) == (flag, amax), "NHWC4 input (NaN in channel 3) differs from NCHW"
    if c.x == "zero_image":                                # acc = 0: the pooled maximum of the constant PReLU(shift), exactly
        b = i["shift"]
        want = torch.clamp(b, min=0) + torch.tensor(c.slope) * torch.clamp(b, max=0)
        assert torch.equal(got[1], want.expand_as(got[1]))
    if c.x == "copies":                                    # the scale is tile-local: a tile's bits do not depend on its round
        same = list(range(0, c.N, 3))
        assert same[-1] >= (c.rounds - 1) * launch.grid and sum(s >= launch.grid for s in same) > 10
        assert bool((got[same] == got[0]).all())
    if c.x == "periodic":                                  # rows repeat every 16: every interior tile sees tile 1's patch
        rows = got[0].view(launch.tiles_y, Z.TPH, *got.shape[2:])
        assert launch.tiles_y - 2 > launch.grid and bool((rows[1:-1] == rows[1]).all())
    if c.rounds > 1:                                       # a NaN met in a later round of the tile loop still reaches the flag
        xb = L.x.clone()
        xb[-1, 1, c.H - 1, c.W - 1] = float("nan")
        assert launch.tiles - 1 >= launch.grid                # (the last tile holds the last pixel)
        assert L.run(x=xb)[1] == 1


@gpu
def test_stem_flag_and_range_words(ops, dev, cus):
    c = by_name(Z.stem_cases(cus), "geo-2x18x66")
    i, y, E = s_ref(c)
    L = SLaunch(ops, dev, c, i)
    host, flag, amax = L.run()
    assert flag == 0
    for bad in (float("inf"), float("nan")):
        for n, ch, h, w in ((0, 0, 0, 0), (c.N - 1, 2, c.H - 1, c.W - 1)):
            xb = L.x.clone()
            xb[n, ch, h, w] = bad
            assert L.run(x=xb)[1] == 1, (bad, n, h, w)
            assert L.run(x=xb, nhwc4=True)[1] == 1, (bad, n, h, w)
    assert L.run(seed_out=2.0 * amax)[2] == 2.0 * amax
    assert L.run(seed_out=0.5 * amax)[2] == amax
