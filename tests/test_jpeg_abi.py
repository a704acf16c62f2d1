"""The JPEG decoder without a device: header, binding and library agree; both structs' layouts against the
C compiler's; every refusal of the host parser and of the two launch entries (on the host, before any launch); truncated and
damaged files end in a status, inside their buffers, also under AddressSanitizer in a stand-alone program; dataset.image_io's
host logic with the upload and the launches stubbed out."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_jpeg_restated import fixtures, restated  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _lib():
    from two_stage_object_detection_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi, _ffi.lib()


def _status(L, rc):
    return L.tsod_status_str(rc).decode().upper() if rc else "OK"


def _fixture(name):
    for n, data, pixels in fixtures()[0]:
        if n == name:
            return data, pixels
    raise KeyError(name)


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    raw_text = open(os.path.join(ROOT, "include", "tsod.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_jpeg_parse", 3), ("tsod_jpeg_entropy_decode", 4), ("tsod_jpeg_idct_u8", 13), ("tsod_jpeg_to_rgb_u8", 11)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name) and name in _ffi.EXPORTED_SYMBOLS, name
    for macro, value in (("TSOD_JPEG_IDCT_BLOCKS", _ffi.JPEG_IDCT_BLOCKS), ("TSOD_JPEG_RGB_TILE_W", _ffi.JPEG_RGB_TILE_W),
                         ("TSOD_JPEG_RGB_TILE_H", _ffi.JPEG_RGB_TILE_H)):
        assert int(re.search(r"#define " + macro + r" (\d+)", raw_text).group(1)) == value, macro
    assert L.tsod_version() == 242                                   # the change only adds exports
    statuses = re.search(r"TSOD_ERR_INVALID_ARG = (-\d+),.*?TSOD_ERR_UNSUPPORTED = (-\d+),", raw_text, flags=re.S)
    assert tuple(int(v) for v in statuses.groups()) == (-1, -2)
    makefile = open(os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "Makefile")).read()
    assert "plot.hip jpeg.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    # the host pass is plain C++ with no HIP in it
    entropy = open(os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "jpeg_entropy.h")).read()
    assert "#include <hip" not in entropy and "__global__" not in entropy and "__device__" not in entropy
    assert "static " not in entropy and "malloc" not in entropy and "new " not in entropy


@pytest.mark.parametrize("struct,mirror", [("tsod_jpeg_info", "JpegInfo"), ("tsod_jpeg_image", "JpegImage")])
def test_struct_layouts_match_header(tmp_path, struct, mirror):
    """The ctypes mirrors against the C compiler's own layout of include/tsod.h: the size and every field."""
    _ffi, _ = _lib()
    S = getattr(_ffi, mirror)
    names = [f[0] for f in S._fields_]
    fmt = " ".join(["%zu"] * (len(names) + 1))
    args = ", ".join([f"sizeof({struct})"] + [f"offsetof({struct}, {n})" for n in names])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsod.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in names]
    header = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", open(os.path.join(ROOT, "include", "tsod.h")).read(),
                       flags=re.S).group(1)
    declared = re.findall(r"(\w+)(?:\[\d+\])*\s*[,;]", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert declared == names                                         # no field of the header is missing from the mirror


def _parse(L, _ffi, data):
    info = _ffi.JpegInfo()
    return L.tsod_jpeg_parse(data, len(data), ctypes.byref(info)), info


def _refusal_cases():
    """(what, file bytes, status): files made by patching bytes of a fixture's frame header, and two files Pillow wrote."""
    data, _ = _fixture("17x33_s2_q75")
    sof = data.index(b"\xff\xc0")                                    # FF C0, length (2), precision, H (2), W (2), components, (id, hv, tq) ...
    assert data[sof + 4] == 8 and data[sof + 5:sof + 7] == b"\x00\x11" and data[sof + 9] == 3 and data[sof + 11] == 0x22

    def patched(offset, value):
        b = bytearray(data)
        b[offset] = value
        return bytes(b)

    _, refused = fixtures()
    return [("progressive SOF", patched(sof + 1, 0xC2), -2), ("arithmetic SOF", patched(sof + 1, 0xC9), -2),
            ("12-bit", patched(sof + 4, 12), -2), ("4x1 luma", patched(sof + 11, 0x41), -2), ("four components", patched(sof + 9, 4), -2),
            ("a progressive file", refused["progressive"], -2), ("a CMYK file", refused["cmyk"], -2),
            ("zero height", patched(sof + 6, 0), -1),
            ("no SOI", b"\x00" + data[1:], -1), ("empty", b"", -1), ("segment past the end", data[:sof + 2] + b"\xff\xff" + data[sof + 4:], -1)]


def test_refusals_on_the_host():
    _ffi, L = _lib()
    for what, data, want in _refusal_cases():
        rc, _ = _parse(L, _ffi, data)
        assert rc == want, what
        buf = np.zeros(1 << 16, dtype=np.int16)
        assert L.tsod_jpeg_entropy_decode(data, len(data), buf.ctypes.data, buf.size) == want, what
    data, _ = _fixture("17x33_s2_q75")
    # an Adobe APP14 segment with transform 0 says the three components are R G B
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    assert _parse(L, _ffi, data[:2] + adobe + data[2:])[0] == -2
    assert _parse(L, _ffi, data[:2] + adobe[:-1] + b"\x01" + data[2:])[0] == 0          # transform 1: YCbCr
    # a missing table: drop the first DHT segment
    dht = data.index(b"\xff\xc4")
    length = int.from_bytes(data[dht + 2:dht + 4], "big")
    assert _parse(L, _ffi, data[:dht] + data[dht + 2 + length:])[0] == -1
    # a scan that starts before any frame header
    sof = data.index(b"\xff\xc0")
    sof_len = int.from_bytes(data[sof + 2:sof + 4], "big")
    assert _parse(L, _ffi, data[:sof] + data[sof + 2 + sof_len:])[0] == -1
    # null pointers
    info = _ffi.JpegInfo()
    assert L.tsod_jpeg_parse(None, 10, ctypes.byref(info)) == -1 and L.tsod_jpeg_parse(data, len(data), None) == -1
    assert L.tsod_jpeg_entropy_decode(data, len(data), None, 1 << 20) == -1
    # a hand-made 8x8 grey file whose code tables are short enough to write the bits out: DC '0' -> category 0; AC '00' -> ZRL,
    # '01' -> EOB, '10' -> run 14 size 1, '110' -> run 0 size 1, and no code that starts '111'
    def tiny(scan):
        seg = lambda marker, body: b"\xff" + bytes([marker]) + (len(body) + 2).to_bytes(2, "big") + body  # noqa: E731
        return (b"\xff\xd8" + seg(0xDB, b"\x00" + b"\x01" * 64) + seg(0xC0, b"\x08\x00\x08\x00\x08\x01\x01\x11\x00")
                + seg(0xC4, b"\x00" + bytes([1] + [0] * 15) + b"\x00")
                + seg(0xC4, b"\x10" + bytes([0, 3, 1] + [0] * 13) + b"\xf0\x00\xe1\x01")
                + seg(0xDA, b"\x01\x01\x00\x00\x3f\x00") + scan + b"\xff\xd9")

    def tiny_decode(scan):
        buf = np.full(64, 99, dtype=np.int16)
        data = tiny(scan)
        return L.tsod_jpeg_entropy_decode(data, len(data), buf.ctypes.data, 64), buf

    rc, buf = tiny_decode(b"\x3f")                                   # 0 01 + pad: an empty block
    assert rc == 0 and not buf.any()
    rc, buf = tiny_decode(b"\x01\x7f")                               # 0 00 00 00 10 1 + pad: three ZRL, then +1 at coefficient 63
    assert rc == 0 and buf[63] == 1 and int(np.abs(buf).sum()) == 1
    assert tiny_decode(b"\x00\x7f")[0] == -1                         # 0 00 00 00 00: the fourth ZRL runs past coefficient 63
    assert tiny_decode(b"\x01\xb7")[0] == -1                         # 0 00 00 00 110 1 10: run 14 from coefficient 50
    assert tiny_decode(b"\x7f")[0] == -1                             # 0 111...: a code the table does not hold
    assert tiny_decode(b"")[0] == -1                                 # no entropy-coded bits at all
    # a wrong restart marker
    rst, _ = _fixture("17x33_s2_rstb")
    at = rst.index(b"\xff\xd0", rst.index(b"\xff\xda"))
    bad = rst[:at + 1] + b"\xd3" + rst[at + 2:]
    buf = np.zeros(1 << 16, dtype=np.int16)
    assert L.tsod_jpeg_entropy_decode(rst, len(rst), buf.ctypes.data, buf.size) == 0
    assert L.tsod_jpeg_entropy_decode(bad, len(bad), buf.ctypes.data, buf.size) == -1


def _guarded_decode(L, data, n_coef):
    """(status, coefficients): the decode into a buffer with GUARD sentinel bytes on both sides, which must survive."""
    raw = np.full(2 * n_coef + 2 * GUARD, 0xC3, dtype=np.uint8)
    rc = L.tsod_jpeg_entropy_decode(data, len(data), raw.ctypes.data + GUARD, n_coef)
    assert (raw[:GUARD] == 0xC3).all() and (raw[GUARD + 2 * n_coef:] == 0xC3).all()
    return rc, raw[GUARD:GUARD + 2 * n_coef].view(np.int16)


def _corruptions(data, count=2000, seed=99):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        b = bytearray(data)
        at = int(rng.integers(0, len(b)))
        b[at] ^= int(rng.integers(1, 256))
        yield bytes(b)


PREFIX_FIXTURES = ("17x33_s2_rstb", "17x9_grey_opt")
CORRUPT_FIXTURE = "37x53_s1_q75"


def test_truncated_files_end_in_a_status():
    """Every proper prefix is refused - except the two that only lack the EOI marker's bytes, which decode as the whole file does:
    the entry point accepts a missing EOI (include/tsod.h), and every entropy-coded bit is still there."""
    _ffi, L = _lib()
    for name in PREFIX_FIXTURES:
        data, _ = _fixture(name)
        assert data[-2:] == b"\xff\xd9"
        rc, info = _parse(L, _ffi, data)
        assert rc == 0
        rc, whole = _guarded_decode(L, data, info.coef_total)
        assert rc == 0
        for n in range(len(data)):
            head = bytes(data[:n])                                    # (a copy of exactly n bytes)
            rc_p, _ = _parse(L, _ffi, head)
            rc, coef = _guarded_decode(L, head, info.coef_total)
            if n >= len(data) - 2:
                assert rc_p == 0 and rc == 0 and np.array_equal(coef, whole), (name, n)
            else:
                assert rc < 0 and rc_p in (0, -1) and (rc_p == 0 or rc == rc_p), (name, n)


def test_damaged_files_end_in_a_status():
    """2000 single-byte corruptions: each ends in TSOD_OK (a byte that only changes values, or one no decoder reads) or in a
    negative status - never in a crash or a write outside the buffer the parse of the same bytes asked for."""
    _ffi, L = _lib()
    data, _ = _fixture(CORRUPT_FIXTURE)
    seen = set()
    for bad in _corruptions(data):
        rc_p, info = _parse(L, _ffi, bad)
        assert rc_p in (0, -1, -2)
        if rc_p:
            buf = np.zeros(16, dtype=np.int16)
            assert L.tsod_jpeg_entropy_decode(bad, len(bad), buf.ctypes.data, buf.size) == rc_p
        else:
            assert 0 < info.coef_total == sum(info.coef_count) and info.coef_total % 64 == 0
            rc, _ = _guarded_decode(L, bad, info.coef_total)
            assert rc in (0, -1)
            seen.add(rc)
        seen.add(rc_p)
    assert seen == {0, -1, -2}                                       # the sweep reaches all three outcomes


def test_host_decoder_under_address_sanitizer(tmp_path):
    """tests/jpeg_entropy_main.cpp - its own main, only csrc/jpeg_entropy.h - built with ASan and UBSan and run over the
    fixtures, the prefixes and the corruptions above with exact-size buffers: exit 0, empty stderr, the library's statuses."""
    _ffi, L = _lib()
    exe = tmp_path / "jpeg_entropy_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "jpeg_entropy_main.cpp"), "-o", str(exe)])
    files = [data for _, data, _ in fixtures()[0]] + [d for _, d, _ in _refusal_cases()]
    for name in PREFIX_FIXTURES:
        data, _ = _fixture(name)
        files += [data[:n] for n in range(len(data))]
    files += list(_corruptions(_fixture(CORRUPT_FIXTURE)[0]))
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / f"f{i}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    want = []
    for data in files:
        rc, info = _parse(L, _ffi, data)
        if rc == 0:
            buf = np.zeros(info.coef_total, dtype=np.int16)
            rc = L.tsod_jpeg_entropy_decode(data, len(data), buf.ctypes.data, buf.size)
        want.append(rc)
    got = []
    for first in range(0, len(paths), 400):
        run = subprocess.run(["timeout", "-k", "5", "120", str(exe)] + paths[first:first + 400], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
        got += [int(line.split()[0]) for line in run.stdout.splitlines()]
    assert got == want


def test_launch_entries_refuse_bad_tables_on_the_host():
    """Every record and every work item is checked against the buffer sizes before anything is launched (the device pointers
    are never dereferenced)."""
    _ffi, L = _lib()
    from two_stage_object_detection_amd import hip_ops
    A = 0x100000

    def record(**kw):
        rec = dict(H=20, W=30, n_comp=3, hs=2, vs=2, blocks_w=(4, 2, 2), blocks_h=(4, 2, 2), coef_offset=(0, 1024, 1280),
                   plane_offset=(0, 1024, 1280), quant_offset=0, out_offset=0)
        rec.update(kw)
        t = (_ffi.JpegImage * 1)()
        for k, v in rec.items():
            if isinstance(v, tuple):
                for c, x in enumerate(v):
                    getattr(t[0], k)[c] = x
            else:
                setattr(t[0], k, v)
        return t

    def idct(table=None, work=((0, 0, 0, 0),), coef=A, coef_count=1536, quant=A, quant_count=192, planes=A, plane_bytes=1536,
             table_dev=A, work_dev=A, n_images=1):
        w = np.array(work, dtype=np.int32).reshape(-1, 4)
        return _status(L, L.tsod_jpeg_idct_u8(table if table is not None else record(), table_dev, n_images, w.ctypes.data, work_dev,
                                              len(w), coef, coef_count, quant, quant_count, planes, plane_bytes, None))

    def rgb(table=None, work=((0, 0, 0, 0),), planes=A, plane_bytes=1536, out=A, out_bytes=1800, table_dev=A, work_dev=A, n_images=1):
        w = np.array(work, dtype=np.int32).reshape(-1, 4)
        return _status(L, L.tsod_jpeg_to_rgb_u8(table if table is not None else record(), table_dev, n_images, w.ctypes.data, work_dev,
                                                len(w), planes, plane_bytes, out, out_bytes, None))

    bad_records = (dict(n_comp=2), dict(n_comp=4), dict(H=0), dict(W=-1), dict(hs=4, vs=1), dict(hs=1, vs=2), dict(hs=3),
                   dict(n_comp=1, hs=2, vs=2), dict(blocks_w=(3, 2, 2)), dict(blocks_h=(2, 2, 2)), dict(blocks_w=(4, 1, 1)),
                   dict(blocks_w=(4, 2, 3)), dict(blocks_w=(0, 2, 2)), dict(plane_offset=(4, 1024, 1280)),
                   dict(plane_offset=(-8, 1024, 1280)), dict(plane_offset=(0, 1024, 1288)), dict(plane_offset=(0, 1024, 1 << 40)))
    for kw in bad_records:
        assert "INVALID" in idct(record(**kw)) and "INVALID" in rgb(record(**kw)), kw
    for kw in (dict(coef_offset=(32, 1024, 1280)), dict(coef_offset=(0, 1024, 1344)), dict(coef_offset=(0, -64, 1280)),
               dict(quant_offset=64), dict(quant_offset=8), dict(quant_offset=-64)):
        assert "INVALID" in idct(record(**kw)), kw
    for kw in (dict(out_offset=1), dict(out_offset=-1)):
        assert "INVALID" in rgb(record(**kw)), kw
    # buffers one unit short
    assert "INVALID" in idct(coef_count=1535) and "INVALID" in idct(quant_count=191) and "INVALID" in idct(plane_bytes=1535)
    assert "INVALID" in rgb(plane_bytes=1535) and "INVALID" in rgb(out_bytes=1799)
    # work items outside the table, the component list, the block grid, the image
    for w in ((1, 0, 0, 0), (-1, 0, 0, 0), (0, 3, 0, 0), (0, -1, 0, 0), (0, 0, 16, 0), (0, 0, 1, 0), (0, 0, -32, 0), (0, 1, 32, 0)):
        assert "INVALID" in idct(work=(w,)), w
    for w in ((1, 0, 0, 0), (-1, 0, 0, 0), (0, 5, 0, 0), (0, -1, 0, 0), (0, 0, 1, 0), (0, 0, -1, 0)):
        assert "INVALID" in rgb(work=(w,)), w
    # null pointers, negative counts, misaligned buffers
    for kw in (dict(coef=None), dict(quant=None), dict(planes=None), dict(table_dev=None), dict(work_dev=None), dict(n_images=0),
               dict(n_images=-1), dict(coef_count=-1)):
        assert "INVALID" in idct(**kw), kw
    for kw in (dict(planes=None), dict(out=None), dict(table_dev=None), dict(work_dev=None), dict(out_bytes=-1)):
        assert "INVALID" in rgb(**kw), kw
    for kw in (dict(coef=A + 8), dict(quant=A + 2), dict(planes=A + 4), dict(table_dev=A + 8), dict(work_dev=A + 4)):
        assert "ALIGN" in idct(**kw), kw
    for kw in (dict(planes=A + 4), dict(table_dev=A + 8), dict(work_dev=A + 4)):
        assert "ALIGN" in rgb(**kw), kw
    # nothing to do: TSOD_OK without a launch, so without a device
    assert idct(work=()) == "OK" and rgb(work=()) == "OK" and idct(work=(), coef=None, table_dev=None) == "OK"
    # the wrappers refuse host tensors
    plan = hip_ops.jpeg_plan([])
    with pytest.raises(_ffi.TsodError, match="no CPU fallback"):
        hip_ops.jpeg_idct(plan["table"], torch.zeros(256, dtype=torch.uint8), plan["idct_work"], torch.zeros(4, dtype=torch.int32),
                          torch.zeros(64, dtype=torch.int16), torch.zeros(64, dtype=torch.int16), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(_ffi.TsodError, match="no CPU fallback"):
        hip_ops.jpeg_to_rgb(plan["table"], torch.zeros(256, dtype=torch.uint8), plan["rgb_work"], torch.zeros(4, dtype=torch.int32),
                            torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))


def test_plan_covers_every_block_and_pixel_once():
    _ffi, L = _lib()
    from two_stage_object_detection_amd import hip_ops
    cases, _ = fixtures()
    infos = [_parse(L, _ffi, data)[1] for _, data, _ in cases[::7]]
    plan = hip_ops.jpeg_plan(infos)
    table = plan["table"]
    assert plan["coef_count"] == sum(i.coef_total for i in infos) == plan["plane_bytes"]
    assert plan["quant_count"] == 64 * sum(i.n_comp for i in infos)
    blocks = {}
    for img, comp, first, zero in plan["idct_work"].tolist():
        n = infos[img].blocks_w[comp] * infos[img].blocks_h[comp]
        assert zero == 0 and first % _ffi.JPEG_IDCT_BLOCKS == 0 and first < n
        blocks[(img, comp)] = blocks.get((img, comp), 0) + min(_ffi.JPEG_IDCT_BLOCKS, n - first)
    assert blocks == {(i, c): info.blocks_w[c] * info.blocks_h[c] for i, info in enumerate(infos) for c in range(info.n_comp)}
    tiles = {}
    for img, ty, tx, zero in plan["rgb_work"].tolist():
        assert zero == 0 and ty * _ffi.JPEG_RGB_TILE_H < infos[img].H and tx * _ffi.JPEG_RGB_TILE_W < infos[img].W
        tiles[img] = tiles.get(img, 0) + 1
    assert tiles == {i: -(-info.H // _ffi.JPEG_RGB_TILE_H) * -(-info.W // _ffi.JPEG_RGB_TILE_W) for i, info in enumerate(infos)}
    end = 0
    for i, info in enumerate(infos):
        assert table[i].out_offset % 256 == 0 and table[i].out_offset >= end
        end = table[i].out_offset + 3 * info.H * info.W
        assert (table[i].hs, table[i].vs) == (info.hmax, info.vmax)
        assert list(table[i].coef_offset)[:info.n_comp] == list(table[i].plane_offset)[:info.n_comp]
    assert plan["out_bytes"] >= end


@pytest.fixture()
def stub(monkeypatch):
    """dataset.image_io without a device: host staging, an upload that stays on the host, launches that record their calls."""
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.dataset import image_io
    calls = []
    monkeypatch.setattr(image_io, "_staging", lambda n: torch.zeros(n, dtype=torch.uint8))
    monkeypatch.setattr(image_io, "_upload", lambda staging, device: calls.append(("upload", staging.numel())) or staging.clone())
    monkeypatch.setattr(image_io, "_empty", lambda n, device: torch.zeros(n, dtype=torch.uint8))
    monkeypatch.setattr(hip_ops, "jpeg_idct", lambda *a: calls.append(("idct",) + a))
    monkeypatch.setattr(hip_ops, "jpeg_to_rgb", lambda *a: calls.append(("to_rgb",) + a))
    return image_io, calls


def test_image_io_batch_host_logic(stub, tmp_path):
    image_io, calls = stub
    _ffi, L = _lib()
    cases, _ = fixtures()
    idx = (0, 20, 41, 60, 86)
    picks = [cases[i] for i in idx]
    path = tmp_path / "a.jpg"
    path.write_bytes(picks[4][1])
    items = [picks[0][1], bytearray(picks[1][1]), memoryview(picks[2][1]), np.frombuffer(picks[3][1], dtype=np.uint8), str(path)]
    dec = image_io.JPEGDecoder("cuda", threads=3)
    out = dec.batch(items)
    assert [c[0] for c in calls] == ["upload", "idct", "to_rgb"]      # one upload, one launch each, in this order
    assert len(out) == 5
    base = out[0].untyped_storage().data_ptr()
    for t, (name, _, pixels) in zip(out, picks):
        assert t.shape == pixels.shape and t.dtype == torch.uint8 and t.is_contiguous(), name
        assert t.untyped_storage().data_ptr() == base and (t.data_ptr() - base) % 256 == 0, name
    offsets = [t.data_ptr() - base for t in out]
    assert offsets == sorted(offsets) and len(set(offsets)) == 5
    # what went up: the table, both work lists, the quantisers and the coefficients of every image, where the table says
    _, table, table_dev, work, work_dev, coef, quant, planes = calls[1]
    assert bytes(table_dev.numpy()) == bytes(table)[:table_dev.numel()] and len(table) == 5
    assert np.array_equal(work_dev.numpy().view(np.int32).reshape(-1, 4), work)
    for i, (name, data, _) in enumerate(picks):
        want_info, want = restated(idx[i])
        flat = np.concatenate([c.reshape(-1) for c in want])
        first = table[i].coef_offset[0]
        assert np.array_equal(coef.numpy()[first:first + flat.size], flat), name
        q = np.concatenate(want_info["quant"]).astype(np.uint16)
        assert np.array_equal(quant.numpy().view(np.uint16)[table[i].quant_offset:table[i].quant_offset + q.size], q), name
    assert calls[2][1] is table and calls[2][2] is table_dev and calls[2][5] is planes
    assert np.array_equal(calls[2][4].numpy().view(np.int32).reshape(-1, 4), calls[2][3])
    # decode / read / the conveniences are batches of one; an empty batch launches nothing
    calls.clear()
    assert dec.decode(picks[1][1]).shape == picks[1][2].shape and dec.read(path).shape == picks[4][2].shape
    assert dec.read(tmp_path / "a.jpg").shape == picks[4][2].shape
    assert [c[0] for c in calls] == ["upload", "idct", "to_rgb"] * 3
    calls.clear()
    assert dec.batch([]) == [] and calls == []
    assert dec._pool is not None                                     # three threads shared the five files above
    dec.close()
    assert dec._pool is None and dec.decode(picks[0][1]).shape == (1, 1, 3)
    assert image_io.decode_jpeg(picks[0][1]).shape == (1, 1, 3) and image_io.read_image(str(path)).shape == picks[4][2].shape
    assert picks[3][0] == "16x16_s0_rstb" and image_io.jpeg_info(picks[3][1]) == image_io.JPEGInfo(16, 16, 3, (1, 1), 1)
    assert image_io.jpeg_info(str(path)).components == 1 and image_io.jpeg_info(_fixture("17x33_s2_rstb")[0]).sampling == (2, 2)
    with pytest.raises(TypeError):
        dec.batch([12])
    with pytest.raises(ValueError):
        dec.batch([np.zeros(4, dtype=np.int32)])


def test_image_io_threads_and_device():
    from two_stage_object_detection_amd import _ffi
    from two_stage_object_detection_amd.dataset import image_io
    assert image_io.JPEGDecoder("cuda").threads == 4
    assert image_io.JPEGDecoder("cuda", threads=64).threads == 16 and image_io.JPEGDecoder("cuda", threads=0).threads == 1
    assert image_io.JPEGDecoder("cuda:1", threads=16).threads == 16
    source = open(os.path.join(ROOT, "two_stage_object_detection_amd", "dataset", "image_io.py")).read()
    assert source.count("cpu_count") == 1                            # only the comment that says it is not used
    with pytest.raises(_ffi.TsodError, match="no CPU fallback"):
        image_io.JPEGDecoder("cpu")
    assert issubclass(image_io.UnsupportedJPEG, _ffi.TsodError) and issubclass(image_io.CorruptJPEG, _ffi.TsodError)


def test_image_io_refuses_before_anything_is_uploaded_or_launched(stub, tmp_path):
    image_io, calls = stub
    good, _ = _fixture("9x5_s2_q100")
    dec = image_io.JPEGDecoder("cuda", threads=2)
    for what, data, want in _refusal_cases():
        exc = image_io.UnsupportedJPEG if want == -2 else image_io.CorruptJPEG
        with pytest.raises(exc, match="item 2"):
            dec.batch([good, good, data, good])
        with pytest.raises(exc, match="item 0"):
            image_io.jpeg_info(data)
    # damage that only the Huffman pass finds: a truncated scan, in a thread of the pool
    cut, _ = _fixture("17x33_s2_rstb")
    with pytest.raises(image_io.CorruptJPEG, match=r"item 1.*entropy"):
        dec.batch([good, cut[:-20], good])
    path = tmp_path / "p.jpg"
    path.write_bytes(fixtures()[1]["progressive"])
    with pytest.raises(image_io.UnsupportedJPEG, match=r"item 1 \(.*p\.jpg\).*no CPU fallback"):
        dec.batch([good, str(path)])
    assert calls == []
