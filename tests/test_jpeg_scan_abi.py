"""The device Huffman pass without a device: header, binding and library agree; the new structs' layouts
against the C compiler's; tsod_jpeg_scan_prepare against tests/jpeg_scan_restated.py on every fixture and every one of its
refusals, inside guarded buffers; the launch entry's refusals (on the host, before any launch); the kernel's algorithm run lane by
lane on the CPU under AddressSanitizer and UBSan (tests/jpeg_huffman_main.cpp) against the host pass on every fixture and on 2000
damaged files; dataset.image_io's entropy="device" host logic with the upload and the launches stubbed out."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_scan_restated as S  # noqa: E402
from test_jpeg_restated import fixtures, rounds  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "two_stage_object_detection_amd", "csrc")
GUARD = 64
SENTINEL = 0xC3
RESTART_FIXTURE = "17x33_s2_rstb"
CORRUPT_FIXTURES = ("37x53_s2_q100", "24x130_s1_rstr", "37x53_s0_opt", "37x53_grey_rstb")


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
            return data
    raise KeyError(name)


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    raw_text = open(os.path.join(ROOT, "include", "tsod.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_jpeg_scan_sizes", 4), ("tsod_jpeg_scan_prepare", 9), ("tsod_jpeg_huffman_i16", 18)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name) and name in _ffi.EXPORTED_SYMBOLS, name
    for macro, value in (("TSOD_JPEG_HUFF_TABLES", _ffi.JPEG_HUFF_TABLES), ("TSOD_JPEG_MAX_SEGMENT_BITS", _ffi.JPEG_MAX_SEGMENT_BITS),
                         ("TSOD_JPEG_STATUS_ERROR", _ffi.JPEG_STATUS_ERROR), ("TSOD_JPEG_STATUS_BLOCKS", _ffi.JPEG_STATUS_BLOCKS),
                         ("TSOD_JPEG_STATUS_LEFTOVER", _ffi.JPEG_STATUS_LEFTOVER)):
        assert int(re.search(r"#define " + macro + r" (\w+)", raw_text).group(1), 0) == value, macro
    assert L.tsod_version() == 242                                   # the change only adds exports
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "jpeg_huffman.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    # the host sweep and the shared core are plain C++: no HIP header, no statics, no allocation
    for header in ("jpeg_scan.h", "jpeg_huffman_core.h"):
        src = open(os.path.join(CSRC, header)).read()
        assert "#include <hip" not in src and "__global__" not in src and "__shared__" not in src, header
        assert "static " not in src and "malloc" not in src and "new " not in src, header
    main = open(os.path.join(ROOT, "tests", "jpeg_huffman_main.cpp")).read()
    assert set(re.findall(r'#include "([^"]+)"', main)) == {"../two_stage_object_detection_amd/csrc/jpeg_huffman_core.h",
                                                            "../two_stage_object_detection_amd/csrc/jpeg_scan.h"}
    from two_stage_object_detection_amd import hip_ops
    assert hip_ops.jpeg_segment_dtype().itemsize == ctypes.sizeof(_ffi.JpegSegment) == 32
    assert hip_ops.JPEG_HUFF_BYTES == 6 * ctypes.sizeof(_ffi.JpegHuff) == 6 * 1416


@pytest.mark.parametrize("struct,mirror", [("tsod_jpeg_huff", "JpegHuff"), ("tsod_jpeg_segment", "JpegSegment")])
def test_struct_layouts_match_header(tmp_path, struct, mirror):
    """The ctypes mirrors (and the NumPy record dtype) against the C compiler's own layout of include/tsod.h."""
    _ffi, _ = _lib()
    from two_stage_object_detection_amd import hip_ops
    T = getattr(_ffi, mirror)
    names = [f[0] for f in T._fields_]
    fmt = " ".join(["%zu"] * (len(names) + 1))
    args = ", ".join([f"sizeof({struct})"] + [f"offsetof({struct}, {n})" for n in names])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsod.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(T)] + [getattr(T, n).offset for n in names]
    header = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", open(os.path.join(ROOT, "include", "tsod.h")).read(),
                       flags=re.S).group(1)
    declared = re.findall(r"(\w+)(?:\[\d+\])*\s*[,;]", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert declared == names
    if mirror == "JpegSegment":
        dt = hip_ops.jpeg_segment_dtype()
        assert list(dt.names) == names and [dt.fields[n][1] for n in names] == got[1:] and dt.itemsize == got[0]


def _prepare(L, _ffi, data, stream_capacity=None, segment_capacity=None):
    """(status, stream bytes, records, tables) of one file, every buffer between sentinel guards that must survive."""
    from two_stage_object_detection_amd import hip_ops
    info = _ffi.JpegInfo()
    cap_b, cap_s = ctypes.c_int64(0), ctypes.c_int32(0)
    if L.tsod_jpeg_parse(data, len(data), ctypes.byref(info)) == 0:
        assert L.tsod_jpeg_scan_sizes(ctypes.byref(info), len(data), ctypes.byref(cap_b), ctypes.byref(cap_s)) == 0
    cap_b = cap_b.value if stream_capacity is None else stream_capacity
    cap_s = cap_s.value if segment_capacity is None else segment_capacity
    sizes = (cap_b, 32 * cap_s, hip_ops.JPEG_HUFF_BYTES)
    bufs = [np.full(n + 2 * GUARD, SENTINEL, dtype=np.uint8) for n in sizes]
    n_b, n_s = ctypes.c_int64(-7), ctypes.c_int32(-7)
    rc = L.tsod_jpeg_scan_prepare(data, len(data), bufs[0].ctypes.data + GUARD, cap_b, ctypes.byref(n_b), bufs[1].ctypes.data + GUARD,
                                  cap_s, ctypes.byref(n_s), bufs[2].ctypes.data + GUARD)
    for b, n in zip(bufs, sizes):
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all()
    if rc:
        return rc, None, None, None
    assert 0 <= n_b.value <= cap_b and 0 < n_s.value <= cap_s
    records = bufs[1][GUARD:GUARD + 32 * n_s.value].view(hip_ops.jpeg_segment_dtype())
    return rc, bufs[0][GUARD:GUARD + n_b.value], records, bufs[2][GUARD:GUARD + sizes[2]]


def test_scan_prepare_equals_restatement_on_every_fixture():
    _ffi, L = _lib()
    cases, _ = fixtures()
    assert len(cases) == 87
    intervals = set()
    for name, data, _ in cases:
        info, want_stream, want_records = S.scan(data)
        rc, stream, records, tables = _prepare(L, _ffi, data)
        assert rc == 0, name
        assert np.array_equal(stream, want_stream), name
        got = [(int(r["first_mcu"]), int(r["n_mcu"]), int(r["stream_offset"]), int(r["bit_length"]), int(r["flags"])) for r in records]
        assert got == want_records and not records["image"].any(), name
        assert all(r[2] % 4 == 0 and r[3] % 8 == 0 for r in got) and sum(r[1] for r in got) == info["mcus_x"] * info["mcus_y"], name
        intervals.add(len(got))
        t = tables.view(np.uint8).reshape(6, 1416)
        for c in range(3):
            for k, key in enumerate(("dc", "ac")):
                row = t[2 * c + k]
                if c >= info["n_comp"]:
                    assert not row.any(), (name, c, key)
                    continue
                look, maxcode, valoff, vals = S.table_layout(info[key][c])
                assert np.array_equal(row[:1024].view(np.uint16), look), (name, c, key)
                assert np.array_equal(row[1024:1092].view(np.int32), maxcode), (name, c, key)
                assert np.array_equal(row[1092:1160].view(np.int32), valoff), (name, c, key)
                assert np.array_equal(row[1160:], vals), (name, c, key)
    assert 1 in intervals and max(intervals) > 8                     # files without restarts, one-block and one-row intervals


def test_scan_prepare_refusals():
    _ffi, L = _lib()
    rst = _fixture(RESTART_FIXTURE)
    info, want_stream, want_records = S.scan(rst)
    assert len(want_records) > 2
    assert _prepare(L, _ffi, rst)[0] == 0
    sos = rst.index(b"\xff\xda")
    at = rst.index(b"\xff\xd0", sos)
    assert _prepare(L, _ffi, rst[:at + 1] + b"\xd3" + rst[at + 2:])[0] == -1             # a wrong RSTn
    assert _prepare(L, _ffi, rst[:at] + rst[at + 2:])[0] == -1                           # the marker is missing
    at1 = rst.index(b"\xff\xd1", sos)
    assert _prepare(L, _ffi, rst[:at1] + b"\xff\xd2" + rst[at1 + 2:])[0] == -1           # the second one out of order
    assert _prepare(L, _ffi, rst[:at] + b"\xff\xff" + rst[at:])[0] == 0                  # fill bytes before a marker are allowed
    assert _prepare(L, _ffi, rst[:-2])[0] == 0                                           # a missing EOI is accepted
    # capacities one short
    assert _prepare(L, _ffi, rst, stream_capacity=want_stream.size)[0] == 0
    assert _prepare(L, _ffi, rst, stream_capacity=want_stream.size - 1)[0] == -1
    assert _prepare(L, _ffi, rst, stream_capacity=0)[0] == -1
    assert _prepare(L, _ffi, rst, segment_capacity=len(want_records))[0] == 0
    assert _prepare(L, _ffi, rst, segment_capacity=len(want_records) - 1)[0] == -1
    assert _prepare(L, _ffi, rst, segment_capacity=0)[0] == -1
    # what the parser refuses is refused alike
    _, refused = fixtures()
    assert _prepare(L, _ffi, refused["progressive"])[0] == -2 and _prepare(L, _ffi, b"")[0] == -1
    # null pointers
    A = np.zeros(1 << 16, dtype=np.uint8)
    p, n_b, n_s = A.ctypes.data, ctypes.c_int64(0), ctypes.c_int32(0)
    good = (rst, len(rst), p, 4096, ctypes.byref(n_b), p + 8192, 64, ctypes.byref(n_s), p + 16384)
    assert L.tsod_jpeg_scan_prepare(*good) == 0
    for k in (0, 2, 4, 5, 7, 8):
        args = list(good)
        args[k] = None
        assert L.tsod_jpeg_scan_prepare(*args) == -1, k
    jinfo = _ffi.JpegInfo()
    assert L.tsod_jpeg_parse(rst, len(rst), ctypes.byref(jinfo)) == 0
    assert L.tsod_jpeg_scan_sizes(None, len(rst), ctypes.byref(n_b), ctypes.byref(n_s)) == -1
    assert L.tsod_jpeg_scan_sizes(ctypes.byref(jinfo), len(rst), None, ctypes.byref(n_s)) == -1
    assert L.tsod_jpeg_scan_sizes(ctypes.byref(jinfo), len(rst), ctypes.byref(n_b), None) == -1
    assert L.tsod_jpeg_scan_sizes(ctypes.byref(jinfo), len(rst), ctypes.byref(n_b), ctypes.byref(n_s)) == 0
    assert n_s.value == len(want_records) and n_b.value >= want_stream.size and n_b.value % 4 == 0


def test_every_prefix_ends_in_a_status():
    """Every strict prefix of a restart file: a status, the guard bytes intact (checked inside _prepare).  The prefixes that
    only lack EOI bytes are accepted; one that ends inside the last interval is accepted by the sweep too - the missing bits
    are the device pass's to find - and every shorter one lacks a restart marker."""
    _ffi, L = _lib()
    rst = _fixture(RESTART_FIXTURE)
    last_marker = max(rst.rindex(bytes([0xFF, 0xD0 + k])) for k in range(8) if bytes([0xFF, 0xD0 + k]) in rst[rst.index(b"\xff\xda"):])
    info = _ffi.JpegInfo()
    seen = set()
    for n in range(len(rst)):
        head = bytes(rst[:n])
        rc_p = L.tsod_jpeg_parse(head, len(head), ctypes.byref(info))
        rc = _prepare(L, _ffi, head)[0]
        seen.add(rc)
        if rc_p:
            assert rc == rc_p, n
        elif n >= last_marker + 2:
            assert rc == 0, n
        else:
            assert rc == -1, n
    assert seen == {0, -1}


def test_launch_entry_refuses_bad_records_on_the_host():
    """Every record and work item is checked before anything is launched (the device pointers are never dereferenced)."""
    _ffi, L = _lib()
    from two_stage_object_detection_amd import hip_ops
    A = 0x100000

    def record(**kw):
        rec = dict(H=20, W=30, n_comp=3, hs=2, vs=2, blocks_w=(4, 2, 2), blocks_h=(4, 2, 2), coef_offset=(0, 1024, 1280))
        rec.update(kw)
        t = (_ffi.JpegImage * 1)()
        for k, v in rec.items():
            if isinstance(v, tuple):
                for c, x in enumerate(v):
                    getattr(t[0], k)[c] = x
            else:
                setattr(t[0], k, v)
        return t

    def segs(*rows):
        a = np.zeros(len(rows), dtype=hip_ops.jpeg_segment_dtype())
        for r, row in zip(a, rows):
            for k, v in dict(dict(stream_offset=0, bit_length=64, image=0, first_mcu=0, n_mcu=4, flags=0), **row).items():
                r[k] = v
        return a

    two = (dict(n_mcu=3, flags=1), dict(first_mcu=3, n_mcu=1, stream_offset=8))

    def run(table=None, segments=None, work=((0, 0, 0, 0),), stream=A, stream_bytes=16, huff=A, n_huff=6, coef=A, coef_count=1536,
            status=A, words=32, table_dev=A, segs_dev=A, work_dev=A, n_images=1):
        sg = segs(dict()) if segments is None else segments
        w = np.array(work, dtype=np.int32).reshape(-1, 4)
        return _status(L, L.tsod_jpeg_huffman_i16(table if table is not None else record(), table_dev, n_images, sg.ctypes.data, segs_dev,
                                                  len(sg), w.ctypes.data, work_dev, len(w), stream, stream_bytes, huff, n_huff, coef,
                                                  coef_count, status, words, None))

    # nothing to do: TSOD_OK without a launch, so without a device
    assert run(work=()) == "OK" and run(segments=segs(*two), work=()) == "OK"
    # subseq_words outside [1, 64], even with nothing to do
    for words in (0, 65, -1):
        assert "INVALID" in run(words=words) and "INVALID" in run(words=words, work=()), words
    for kw in (dict(n_comp=2), dict(hs=4, vs=1), dict(hs=1, vs=2), dict(n_comp=1), dict(blocks_w=(3, 2, 2)), dict(blocks_w=(4, 1, 1)),
               dict(blocks_h=(4, 2, 3)), dict(blocks_w=(0, 2, 2)), dict(coef_offset=(32, 1024, 1280)), dict(coef_offset=(0, 1024, 1344)),
               dict(coef_offset=(0, -64, 1280)), dict(coef_offset=(0, 1024, 1 << 40))):
        assert "INVALID" in run(record(**kw)), kw
    assert "INVALID" in run(coef_count=1535) and "INVALID" in run(n_huff=5)
    # an offset outside its buffer, a misaligned offset, lengths that are not whole bytes or too long
    for row in (dict(stream_offset=16), dict(stream_offset=12), dict(stream_offset=-4), dict(stream_offset=2), dict(bit_length=136),
                dict(bit_length=60), dict(bit_length=-8), dict(bit_length=0x7FF00008), dict(flags=2), dict(flags=-1)):
        assert "INVALID" in run(segments=segs(row)), row
    assert "INVALID" in run(stream_bytes=7)
    # segments that do not tile the MCUs: short, long, a gap, an overlap, out of order, an image without segments, unsorted
    for rows in ((dict(n_mcu=3),), (dict(n_mcu=5),), (dict(n_mcu=0),), (dict(first_mcu=1, n_mcu=3),),
                 (dict(n_mcu=2), dict(first_mcu=3, n_mcu=1)), (dict(n_mcu=3), dict(first_mcu=2, n_mcu=2)),
                 (dict(first_mcu=3, n_mcu=1), dict(n_mcu=3)), (dict(image=1),), (dict(image=-1),), (dict(), dict(image=1))):
        assert "INVALID" in run(segments=segs(*rows)), rows
    two_images = (_ffi.JpegImage * 2)()
    two_images[0] = record()[0]
    two_images[1] = record()[0]
    assert "INVALID" in run(two_images, segs(dict()), n_images=2, n_huff=12)             # the second image has no segment
    assert "INVALID" in run(two_images, segs(dict(image=1), dict()), n_images=2, n_huff=12)
    assert "INVALID" in run(two_images, segs(dict(), dict(image=1)), n_images=2, n_huff=11)
    # a work item outside the table
    for w in ((1, 0, 0, 0), (-1, 0, 0, 0)):
        assert "INVALID" in run(work=(w,)), w
    assert "INVALID" in run(segments=segs(*two), work=((0, 0, 0, 0), (2, 0, 0, 0)))
    # null pointers, negative counts, misaligned buffers
    for kw in (dict(stream=None), dict(huff=None), dict(coef=None), dict(status=None), dict(table_dev=None), dict(segs_dev=None),
               dict(work_dev=None), dict(n_images=0), dict(n_images=-1), dict(coef_count=-1), dict(stream_bytes=-1), dict(n_huff=-1)):
        assert "INVALID" in run(**kw), kw
    for kw in (dict(coef=A + 8), dict(stream=A + 2), dict(huff=A + 2), dict(status=A + 2), dict(table_dev=A + 8), dict(segs_dev=A + 8),
               dict(work_dev=A + 4)):
        assert "ALIGN" in run(**kw), kw
    # the wrapper refuses host tensors
    plan = hip_ops.jpeg_plan([])
    with pytest.raises(_ffi.TsodError, match="no CPU fallback"):
        hip_ops.jpeg_huffman(plan["table"], torch.zeros(256, dtype=torch.uint8), segs(dict()), torch.zeros(32, dtype=torch.uint8),
                             np.zeros((1, 4), dtype=np.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8),
                             torch.zeros(8496, dtype=torch.uint8), torch.zeros(64, dtype=torch.int16), torch.zeros(1, dtype=torch.int32), 32)


@pytest.fixture(scope="module")
def cpu_program(tmp_path_factory):
    """tests/jpeg_huffman_main.cpp - its own main, only the new headers - built with ASan and UBSan."""
    exe = tmp_path_factory.mktemp("huffman") / "jpeg_huffman_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "jpeg_huffman_main.cpp"), "-o", str(exe)])
    return str(exe)


def _sweep(exe, tmp_path, files, words):
    """The program's lines for `files`: exit 0 (device status 0 exactly where the host pass accepts, equal coefficients where
    both accept) and an empty stderr (no sanitizer report)."""
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / f"f{i}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    lines = []
    for first in range(0, len(paths), 400):
        run = subprocess.run(["timeout", "-k", "5", "300", exe, words] + paths[first:first + 400], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-500:], run.stderr[-2000:])
        lines += [line.split() for line in run.stdout.splitlines()]
    assert len(lines) == len(files)
    return lines


def test_device_pass_on_the_cpu_under_sanitizers_every_fixture(cpu_program, tmp_path):
    """Every fixture at subseq_words 1, 2, 3 and 32, lane by lane with exact-size buffers: the host pass's coefficients."""
    cases, _ = fixtures()
    lines = _sweep(cpu_program, tmp_path, [data for _, data, _ in cases], "1,2,3,32")
    most = 0
    for (name, _, _), line in zip(cases, lines):
        assert line[:2] == ["0", "0"] and len(line) == 18, name
        for k in range(4):
            assert line[2 + 4 * k:4 + 4 * k] == ["0", "1"], (name, k)
        most = max(most, int(line[4]))
    assert 1 < most < 256                                            # 32-bit subsequences do need the fixpoint, and it ends early


def test_device_pass_on_the_cpu_under_sanitizers_round_boundaries(cpu_program, tmp_path):
    """tests/golden/jpeg_rounds.npz: one segment each of 256, 257, 512 and 513 one-word subsequences - a full last round, and a
    last round of one lane from the carried state - and of 256 and 257 again at two words: the host pass's coefficients."""
    cases = rounds()
    assert [n for _, _, _, n in cases] == [256, 257, 512, 513]
    for name, data, _, n in cases:
        records = S.scan(data)[2]
        assert len(records) == 1 and -(-records[0][3] // 32) == n, name
        assert n < 512 or -(-records[0][3] // 64) == n - 256, name
    lines = _sweep(cpu_program, tmp_path, [data for _, data, _, _ in cases], "1,2")
    for (name, _, _, _), line in zip(cases, lines):
        assert line[:2] == ["0", "0"] and len(line) == 10, name
        for k in range(2):
            assert line[2 + 4 * k:4 + 4 * k] == ["0", "1"], (name, k)


def test_device_pass_on_the_cpu_under_sanitizers_damaged_files(cpu_program, tmp_path):
    """2000 seeded single-byte corruptions of the entropy-coded segments of four fixtures (4:2:0 and 4:4:4 without restart
    markers, 4:2:2 and grey with), at subseq_words 1 and 32: status 0 exactly where the host pass returns TSOD_OK, equal coefficients where
    both succeed (the program exits 1 otherwise), no sanitizer report, and both outcomes are reached."""
    files = []
    for k, name in enumerate(CORRUPT_FIXTURES):
        files += S.corruptions(_fixture(name), 500, 1000 + k)
    lines = _sweep(cpu_program, tmp_path, files, "1,32")
    accepted = sum(line[0] == "0" for line in lines)
    assert 50 < accepted < 1950
    assert any(line[1] != "0" for line in lines)                     # a damaged restart marker: refused by the sweep itself
    bits = set()
    for line in lines:
        if line[0] != "0" and line[1] == "0":
            assert int(line[2]) != 0 and int(line[6]) != 0
            bits.add(int(line[2]))
    assert len(bits) > 1                                             # more than one kind of damage


def test_status_corruptions_of_the_gpu_test_on_the_cpu_first(cpu_program, tmp_path):
    """The 3 x 200 damaged files tests/test_jpeg_huffman_gpu.py decodes on the device, first here: lane by lane under the
    sanitizers at the default subsequence length and at one word."""
    from two_stage_object_detection_amd.dataset import image_io
    default = image_io.JPEGDecoder("cuda", entropy="device").subseq_bits // 32
    files = []
    for name in S.STATUS_FIXTURES:
        files += S.status_corruptions(name, _fixture(name))
    lines = _sweep(cpu_program, tmp_path, files, f"{default},1")
    for first in range(0, 600, 200):
        accepted = sum(line[0] == "0" for line in lines[first:first + 200])
        assert 5 < accepted < 195, first                             # every group has both outcomes


@pytest.fixture()
def stub(monkeypatch):
    """dataset.image_io without a device: host staging, an upload that stays on the host, launches that record their calls."""
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.dataset import image_io
    calls = []
    monkeypatch.setattr(image_io, "_staging", lambda n: torch.zeros(n, dtype=torch.uint8))
    monkeypatch.setattr(image_io, "_upload", lambda staging, device: calls.append(("upload", staging.numel())) or staging.clone())
    monkeypatch.setattr(image_io, "_empty", lambda n, device: torch.zeros(n, dtype=torch.uint8))
    monkeypatch.setattr(hip_ops, "jpeg_huffman", lambda *a: calls.append(("huffman",) + a))
    monkeypatch.setattr(hip_ops, "jpeg_idct", lambda *a: calls.append(("idct",) + a))
    monkeypatch.setattr(hip_ops, "jpeg_to_rgb", lambda *a: calls.append(("to_rgb",) + a))
    return image_io, calls


def test_image_io_device_entropy_host_logic(stub):
    image_io, calls = stub
    _ffi, L = _lib()
    cases, _ = fixtures()
    picks = [cases[i] for i in (0, 20, 41, 60, 86)]
    dec = image_io.JPEGDecoder("cuda", threads=3, entropy="device", subseq_bits=96)
    assert (dec.entropy, dec.subseq_bits, dec.status) == ("device", 96, None)
    out = dec.batch([data for _, data, _ in picks])
    assert [c[0] for c in calls] == ["upload", "huffman", "idct", "to_rgb"]       # one upload, then the launches in this order
    assert [t.shape for t in out] == [p[2].shape for p in picks]
    _, table, table_dev, segments, segments_dev, work, work_dev, stream, huff, coef, status, words = calls[1]
    assert words == 3 and status is dec.status and status.dtype == torch.int32 and status.numel() == 5
    assert coef.dtype == torch.int16 and coef is calls[2][5] and table is calls[2][1]
    assert bytes(segments_dev.numpy()) == segments.tobytes() and np.array_equal(work_dev.numpy().view(np.int32).reshape(-1, 4), work)
    assert np.array_equal(work[:, 0], np.arange(len(segments))) and not work[:, 1:].any()
    # what went up is what the restatement says, image after image, the offsets moved to the image's place
    at = 0
    for i, (name, data, _) in enumerate(picks):
        _, want_stream, want_records = S.scan(data)
        mine = segments[segments["image"] == i]
        assert len(mine) == len(want_records) and np.array_equal(mine, segments[at:at + len(mine)]), name
        base = int(mine["stream_offset"][0])
        assert base % 4 == 0 and [int(r["stream_offset"]) - base for r in mine] == [r[2] for r in want_records], name
        assert np.array_equal(stream.numpy()[base:base + want_stream.size], want_stream), name
        got, _, _, tables = _prepare(L, _ffi, data)
        assert got == 0 and np.array_equal(huff.numpy()[8496 * i:8496 * (i + 1)], tables), name
        at += len(mine)
    assert at == len(segments)
    # damage the host can see is raised before anything is uploaded; host mode is untouched by the keyword's existence
    calls.clear()
    rst = _fixture(RESTART_FIXTURE)
    at = rst.index(b"\xff\xd0", rst.index(b"\xff\xda"))
    with pytest.raises(image_io.CorruptJPEG, match=r"item 1.*restart"):
        dec.batch([picks[0][1], rst[:at + 1] + b"\xd3" + rst[at + 2:]])
    with pytest.raises(image_io.UnsupportedJPEG, match="item 0"):
        dec.batch([fixtures()[1]["progressive"]])
    assert calls == []
    dec.raise_if_corrupt()                                           # (all zero in the stub)
    dec.status[3] = 2
    with pytest.raises(image_io.CorruptJPEG, match="item 3"):
        dec.raise_if_corrupt()
    host = image_io.JPEGDecoder("cuda")
    assert (host.entropy, host.subseq_bits) == ("host", image_io.JPEGDecoder("cuda", entropy="device").subseq_bits)
    host.batch([picks[1][1]])
    assert [c[0] for c in calls] == ["upload", "idct", "to_rgb"] and host.status is None
    host.raise_if_corrupt()
    calls.clear()
    assert image_io.decode_jpeg(picks[1][1], entropy="device").shape == picks[1][2].shape
    assert [c[0] for c in calls] == ["upload", "huffman", "idct", "to_rgb"]
    for kw in (dict(entropy="gpu"), dict(subseq_bits=0), dict(subseq_bits=48), dict(subseq_bits=2080), dict(subseq_bits=64.5)):
        with pytest.raises(ValueError):
            image_io.JPEGDecoder("cuda", **kw)
