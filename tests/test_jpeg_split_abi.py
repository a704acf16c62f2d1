"""The split mode of the device Huffman pass ("split over workgroups") without a device: header, binding
and library agree; the workspace size; hip_ops.jpeg_split_chunks against a restatement; the launch entry's refusals (on the host,
before any launch); JPEGDecoder(split=...) with the upload and the launches stubbed out; and the three launches run lane by lane
on the CPU under AddressSanitizer and UBSan (tests/jpeg_huffman_split_main.cpp) against the host pass on every fixture at every
parameter triple, on the two large files and on the 3 x 200 damaged files the GPU test decodes."""
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
# (subseq_words, chunk_subseqs, overlap)
ROUND_TRIPLES = ((1, 256, 0), (1, 255, 1), (1, 128, 0))             # for tests/golden/jpeg_rounds.npz: whole, warmed and half rounds
TRIPLES = ((1, 1, 0), (1, 3, 0), (1, 3, 2), (1, 5, 251), (1, 256, 0), (2, 64, 16), (3, 224, 32), (32, 256, 0), (32, 2, 1))


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


def _large():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_large.npz"))
    return [z[f"file_{i}"].tobytes() for i in range(len(z["names"]))]


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_jpeg_huffman_split_workspace_bytes", 3), ("tsod_jpeg_huffman_split_i16", 23)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name) and name in _ffi.EXPORTED_SYMBOLS, name
    # the chunk arithmetic is plain C++ beside the shared core, and the CPU program uses nothing else
    src = open(os.path.join(CSRC, "jpeg_huffman_split.h")).read()
    assert "#include <hip" not in src and "__global__" not in src and "__shared__" not in src
    assert "static " not in src and "malloc" not in src and "new " not in src
    main = open(os.path.join(ROOT, "tests", "jpeg_huffman_split_main.cpp")).read()
    assert set(re.findall(r'#include "([^"]+)"', main)) == {"../two_stage_object_detection_amd/csrc/jpeg_huffman_core.h",
                                                            "../two_stage_object_detection_amd/csrc/jpeg_huffman_split.h",
                                                            "../two_stage_object_detection_amd/csrc/jpeg_scan.h"}
    assert "LD_PRELOAD" not in main


def test_workspace_bytes():
    """48 bytes per chunk, 32 per subsequence and per lane slot a segment's last chunk may leave unused (at most 256)."""
    _, L = _lib()
    from two_stage_object_detection_amd import hip_ops
    f = L.tsod_jpeg_huffman_split_workspace_bytes
    assert f(0, 0, 0) == 0 and f(0, 1, 1) == 48 + 32 * 256
    assert f(1000, 7, 2) == 48 * 7 + 32 * (1000 + 512)
    assert f(1 << 26, 1 << 26, 1) == 48 * (1 << 26) + 32 * ((1 << 26) + 256)
    assert f(-1, 1, 1) == 0 and f(1, -1, 1) == 0 and f(1, 1, -1) == 0
    assert hip_ops.jpeg_huffman_split_workspace_bytes(1000, 7, 2) == f(1000, 7, 2)
    # enough for chunk_subseqs lane records per chunk, whatever the lengths are
    for bits in ((0,), (8,), (32 * 256,), (32 * 256 + 8, 0, 32 * 255), (8222 * 8, 40)):
        for words, chunk in ((1, 1), (1, 3), (1, 256), (2, 64), (64, 255)):
            n = [-(-b // (32 * words)) for b in bits]
            chunks = [max(1, -(-k // chunk)) for k in n]
            assert f(sum(n), sum(chunks), len(bits)) >= 48 * sum(chunks) + 32 * chunk * sum(chunks), (bits, words, chunk)


def _segments(bit_lengths):
    from two_stage_object_detection_amd import hip_ops
    a = np.zeros(len(bit_lengths), dtype=hip_ops.jpeg_segment_dtype())
    a["bit_length"] = bit_lengths
    return a


def _chunks_restated(bit_lengths, words, chunk):
    """The chunk list, item by item."""
    items, n_subseqs = [], 0
    for k, bits in enumerate(bit_lengths):
        n = (bits + 32 * words - 1) // (32 * words)
        count = max(1, (n + chunk - 1) // chunk)
        first = len(items)
        items += [(k, c, first, count) for c in range(count)]
        n_subseqs += n
    return np.array(items, dtype=np.int32).reshape(-1, 4), n_subseqs


def test_split_chunks_equals_restatement():
    from two_stage_object_detection_amd import hip_ops
    rng = np.random.default_rng(7)
    cases = [[0], [8], [32], [40], [32 * 256], [32 * 256 + 8], [0, 8, 0], [8222 * 8, 16, 32 * 3, 32 * 3 + 8]]
    cases += [list(8 * rng.integers(0, 5000, size=int(rng.integers(1, 40)))) for _ in range(20)]
    for bit_lengths in cases:
        for words, chunk in ((1, 1), (1, 3), (1, 5), (1, 256), (2, 64), (3, 224), (32, 256), (32, 2), (64, 7)):
            got, n = hip_ops.jpeg_split_chunks(_segments(bit_lengths), words, chunk)
            want, want_n = _chunks_restated([int(b) for b in bit_lengths], words, chunk)
            assert got.dtype == np.int32 and got.flags.c_contiguous and np.array_equal(got, want) and n == want_n, (bit_lengths, words, chunk)
    for words, chunk in ((0, 1), (65, 1), (1, 0), (1, 257)):
        with pytest.raises(ValueError):
            hip_ops.jpeg_split_chunks(_segments([8]), words, chunk)


def test_launch_entry_refuses_bad_arguments_on_the_host():
    """Every record, the chunk list and the workspace are checked before anything is launched (the device pointers are never
    dereferenced): each case differs from a list the entry would launch in the one thing named."""
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

    # two segments of image 0: 2400 bits (75 words) and 64 bits
    sg = np.zeros(2, dtype=hip_ops.jpeg_segment_dtype())
    sg[0] = (0, 2400, 0, 0, 3, 1)
    sg[1] = (300, 64, 0, 3, 1, 0)
    WORDS, CHUNK = 2, 5                                              # 38 and 1 subsequences: 8 chunks and 1
    good, n_subseqs = _chunks_restated([2400, 64], WORDS, CHUNK)
    assert len(good) == 9 and n_subseqs == 39
    need = L.tsod_jpeg_huffman_split_workspace_bytes(n_subseqs, len(good), 2)

    def run(chunks=good, segments=sg, table=None, words=WORDS, chunk=CHUNK, overlap=3, workspace=A, workspace_bytes=need, repaired=A,
            stream=A, stream_bytes=308, huff=A, n_huff=6, coef=A, coef_count=1536, status=A, table_dev=A, segs_dev=A, chunks_dev=A,
            n_images=1):
        w = np.ascontiguousarray(np.array(chunks, dtype=np.int32).reshape(-1, 4))
        return _status(L, L.tsod_jpeg_huffman_split_i16(table if table is not None else record(), table_dev, n_images, segments.ctypes.data,
                                                        segs_dev, len(segments), w.ctypes.data, chunks_dev, len(w), stream, stream_bytes,
                                                        huff, n_huff, coef, coef_count, status, words, chunk, overlap, workspace,
                                                        workspace_bytes, repaired, None))

    # an empty list: TSOD_OK without a launch, so without a device
    assert run(chunks=()) == "OK" and run(chunks=(), workspace=None, workspace_bytes=0, repaired=None) == "OK"
    # the three lengths out of range, even with nothing to do
    for kw in (dict(words=0), dict(words=65), dict(chunk=0), dict(chunk=257), dict(chunk=-1), dict(overlap=-1), dict(overlap=252),
               dict(chunk=256, overlap=1), dict(chunk=1, overlap=256)):
        assert "INVALID" in run(**kw) and "INVALID" in run(chunks=(), **kw), kw
    # a chunk list that is not every segment's chunks in order with the implied count
    def changed(row, col, value):
        c = good.copy()
        c[row, col] = value
        return c

    swapped = good.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    by_segment = np.concatenate([good[8:], good[:8]])                # segment 1 before segment 0
    for what, chunks in (("a chunk missing", good[:-1]), ("the last segment missing", good[:8]), ("one too many", np.concatenate([good, good[-1:]])),
                         ("a chunk twice", np.concatenate([good[:3], good[2:]])), ("chunks out of order", swapped),
                         ("not sorted by segment", by_segment), ("another count", changed(0, 3, 7)), ("another first index", changed(8, 2, 7)),
                         ("a segment outside", changed(8, 0, 2)), ("a negative segment", changed(0, 0, -1)), ("a chunk index outside", changed(7, 1, 8)),
                         ("the counts of another chunk length", _chunks_restated([2400, 64], WORDS, 4)[0]),
                         ("the counts of another subsequence length", _chunks_restated([2400, 64], 1, CHUNK)[0])):
        assert "INVALID" in run(chunks=chunks), what
    # the workspace: too small by one byte, missing, misaligned
    assert "INVALID" in run(workspace_bytes=need - 1) and "INVALID" in run(workspace_bytes=0) and "INVALID" in run(workspace=None)
    assert "ALIGN" in run(workspace=A + 8) and "ALIGN" in run(repaired=A + 2)
    # what tsod_jpeg_huffman_i16 refuses is refused alike: records, buffers, pointers
    for kw in (dict(table=record(n_comp=2)), dict(table=record(coef_offset=(32, 1024, 1280))), dict(coef_count=1535), dict(n_huff=5),
               dict(stream_bytes=307), dict(stream=None), dict(huff=None), dict(coef=None), dict(status=None), dict(table_dev=None),
               dict(segs_dev=None), dict(chunks_dev=None), dict(n_images=0), dict(coef_count=-1)):
        assert "INVALID" in run(**kw), kw
    bad = sg.copy()
    bad["n_mcu"][1] = 2                                              # the segments do not tile the image's four MCUs
    assert "INVALID" in run(segments=bad)
    for kw in (dict(coef=A + 8), dict(stream=A + 2), dict(huff=A + 2), dict(status=A + 2), dict(table_dev=A + 8), dict(segs_dev=A + 8),
               dict(chunks_dev=A + 4)):
        assert "ALIGN" in run(**kw), kw
    # the wrapper refuses host tensors
    plan = hip_ops.jpeg_plan([])
    with pytest.raises(_ffi.TsodError, match="no CPU fallback"):
        hip_ops.jpeg_huffman_split(plan["table"], torch.zeros(256, dtype=torch.uint8), sg, torch.zeros(64, dtype=torch.uint8), good,
                                   torch.zeros(36, dtype=torch.int32), torch.zeros(308, dtype=torch.uint8), torch.zeros(8496, dtype=torch.uint8),
                                   torch.zeros(1536, dtype=torch.int16), torch.zeros(1, dtype=torch.int32), WORDS, CHUNK, 3,
                                   torch.zeros(need, dtype=torch.uint8))


def test_decoder_split_argument():
    from two_stage_object_detection_amd.dataset import image_io
    D = image_io.JPEGDecoder
    assert D("cuda").split is None and D("cuda", entropy="device").split is None and D("cuda", entropy="device").repaired is None
    assert D("cuda", entropy="device", split=True).split == (224, 32) == D("cuda", entropy="device", split=(224, 32)).split
    assert D("cuda", entropy="device", split=[1, 255]).split == (1, 255) and D("cuda", entropy="device", split=(256, 0)).split == (256, 0)
    for kw in (dict(split=True), dict(split=(64, 16)), dict(entropy="host", split=(64, 16))):
        with pytest.raises(ValueError, match="split"):
            D("cuda", **kw)
    for split in ((0, 0), (257, 0), (1, 256), (224, 33), (64, -1), (64,), (64, 16, 1), 64, (64.5, 16), "ab", False):
        with pytest.raises(ValueError, match="split"):
            D("cuda", entropy="device", split=split)
    assert D("cuda", entropy="device", subseq_bits=64, split=(3, 2)).subseq_bits == 64


@pytest.fixture()
def stub(monkeypatch):
    """dataset.image_io without a device: host staging, an upload that stays on the host, launches that record their calls."""
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.dataset import image_io
    calls = []
    monkeypatch.setattr(image_io, "_staging", lambda n: torch.zeros(n, dtype=torch.uint8))
    monkeypatch.setattr(image_io, "_upload", lambda staging, device: calls.append(("upload", staging.numel())) or staging.clone())
    monkeypatch.setattr(image_io, "_empty", lambda n, device: torch.zeros(n, dtype=torch.uint8))
    monkeypatch.setattr(image_io, "_DECODERS", {})
    monkeypatch.setattr(hip_ops, "jpeg_huffman", lambda *a: calls.append(("huffman",) + a))
    monkeypatch.setattr(hip_ops, "jpeg_huffman_split", lambda *a: calls.append(("split",) + a))
    monkeypatch.setattr(hip_ops, "jpeg_idct", lambda *a: calls.append(("idct",) + a))
    monkeypatch.setattr(hip_ops, "jpeg_to_rgb", lambda *a: calls.append(("to_rgb",) + a))
    return image_io, calls


def test_image_io_split_host_logic(stub):
    """One upload that holds the chunk list, then the split entry instead of jpeg_huffman, with a workspace of the stated size."""
    image_io, calls = stub
    from two_stage_object_detection_amd import hip_ops
    cases, _ = fixtures()
    picks = [cases[i] for i in (0, 20, 41, 60, 86)] + [("large", _large()[0], None)]
    dec = image_io.JPEGDecoder("cuda", threads=3, entropy="device", subseq_bits=64, split=(5, 3))
    out = dec.batch([p[1] for p in picks])
    assert [c[0] for c in calls] == ["upload", "split", "idct", "to_rgb"]
    assert [t.shape for t in out[:5]] == [p[2].shape for p in picks[:5]]
    (_, table, table_dev, segments, segments_dev, chunks, chunks_dev, stream, huff, coef, status, words, chunk, overlap, workspace,
     repaired) = calls[1]
    assert (words, chunk, overlap) == (2, 5, 3) and status is dec.status and repaired is dec.repaired
    assert repaired.dtype == torch.int32 and repaired.numel() == len(segments) and status.numel() == len(picks)
    want, n_subseqs = _chunks_restated([int(b) for b in segments["bit_length"]], 2, 5)
    assert np.array_equal(chunks, want) and len(chunks) > len(segments) + 1000
    assert np.array_equal(chunks_dev.numpy().view(np.int32).reshape(-1, 4), want)          # it went up with the one upload
    assert workspace.dtype == torch.uint8 and workspace.numel() == hip_ops.jpeg_huffman_split_workspace_bytes(n_subseqs, len(want), len(segments))
    assert coef is calls[2][5] and bytes(segments_dev.numpy()) == segments.tobytes()
    # the same decoder in host mode forgets the tensor; the conveniences pass the keyword through, on a decoder of their own
    dec.entropy = "host"
    dec.batch([picks[0][1]])
    assert dec.repaired is None and dec.status is None
    calls.clear()
    assert image_io.decode_jpeg(picks[1][1], entropy="device", split=True).shape == picks[1][2].shape
    assert [c[0] for c in calls] == ["upload", "split", "idct", "to_rgb"] and calls[1][12:14] == (224, 32)
    assert image_io._decoder("cuda", "device", True) is image_io._decoder("cuda", "device", (224, 32))
    assert image_io._decoder("cuda", "device", True) is not image_io._decoder("cuda", "device")
    calls.clear()
    image_io.decode_jpeg(picks[1][1], entropy="device")
    assert [c[0] for c in calls] == ["upload", "huffman", "idct", "to_rgb"]
    with pytest.raises(ValueError, match="split"):
        image_io.decode_jpeg(picks[1][1], split=True)


@pytest.fixture(scope="module")
def cpu_program(tmp_path_factory):
    """tests/jpeg_huffman_split_main.cpp - its own main, only the csrc headers - built with ASan and UBSan."""
    exe = tmp_path_factory.mktemp("split") / "jpeg_huffman_split_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "jpeg_huffman_split_main.cpp"), "-o", str(exe)])
    return str(exe)


def _sweep(exe, tmp_path, files, triples):
    """The program's lines for `files`, per triple (status, equal, chunks, accepted, repaired, most passes): exit 0 (device status
    0 exactly where the host pass accepts, equal coefficients where both accept) and an empty stderr (no sanitizer report)."""
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / f"f{i}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    arg = ":".join(",".join(str(v) for v in t) for t in triples)
    run = subprocess.run(["timeout", "-k", "5", "300", exe, arg] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    lines = [line.split() for line in run.stdout.splitlines()]
    assert len(lines) == len(files) and all(len(line) in (2, 2 + 6 * len(triples)) for line in lines)
    return [(line[:2], [line[2 + 6 * k:8 + 6 * k] for k in range(len(triples))] if len(line) > 2 else None) for line in lines]


def _totals(lines, k):
    """(chunks, accepted, repaired, most passes) of triple k over the files"""
    rows = [per[k] for _, per in lines]
    return tuple(sum(int(r[c]) for r in rows) for c in (2, 3, 4)) + (max(int(r[5]) for r in rows),)


def test_split_pass_on_the_cpu_under_sanitizers_every_fixture(cpu_program, tmp_path):
    """Every fixture at every triple, lane by lane with exact-size buffers and a workspace that starts as 0xA5: the host pass's
    coefficients; both outcomes of a boundary - accepted and repaired - are reached."""
    cases, _ = fixtures()
    lines = _sweep(cpu_program, tmp_path, [data for _, data, _ in cases], TRIPLES)
    for (name, _, _), (head, per) in zip(cases, lines):
        assert head == ["0", "0"], name
        for t, got in zip(TRIPLES, per):
            assert got[:2] == ["0", "1"], (name, t)
    totals = {t: _totals(lines, k) for k, t in enumerate(TRIPLES)}
    segments = totals[(32, 256, 0)][0]
    assert totals[(32, 256, 0)][:3] == (segments, 0, 0) and segments > 200          # no file is longer than 256 x 1024 bits
    for t, (chunks, accepted, repaired, most) in totals.items():
        assert accepted + repaired == chunks - segments, t                           # no true error: every boundary is looked at
        assert 1 <= most <= t[1] + t[2] + 1, t
    assert totals[(1, 3, 0)][2] > 0
    assert totals[(1, 5, 251)][1] > 0 and totals[(1, 5, 251)][2] > 0
    words32 = sum(max(1, -(-record[3] // 32)) for _, data, _ in cases for record in S.scan(data)[2])
    assert totals[(1, 1, 0)][0] == words32 > 9000                    # one chunk per 32-bit subsequence


def test_split_pass_on_the_cpu_under_sanitizers_large_files(cpu_program, tmp_path):
    triples = ((32, 224, 32), (4, 224, 32), (32, 2, 0))
    lines = _sweep(cpu_program, tmp_path, _large(), triples)
    assert len(lines) == 2
    for head, per in lines:
        assert head == ["0", "0"] and all(got[:2] == ["0", "1"] for got in per)
    chunks, accepted, repaired, _ = _totals(lines, 0)
    assert chunks > 2 and accepted == chunks - 2 and repaired == 0   # 32 x 1024 bits of overlap: every entry is the true one
    _, accepted, repaired, _ = _totals(lines, 1)
    assert accepted > 0 and repaired > 0
    assert _totals(lines, 2)[2] > 500


def test_split_pass_on_the_cpu_under_sanitizers_round_boundaries(cpu_program, tmp_path):
    """tests/golden/jpeg_rounds.npz - 256, 257, 512 and 513 one-word subsequences - in chunks of a whole round, of a round less
    one lane after one lane of warm-up, and of half a round: the last chunk is full, or is one lane."""
    cases = rounds()
    lines = _sweep(cpu_program, tmp_path, [data for _, data, _, _ in cases], ROUND_TRIPLES)
    for (name, _, _, n), (head, per) in zip(cases, lines):
        assert head == ["0", "0"], name
        for (_, chunk, _), got in zip(ROUND_TRIPLES, per):
            assert got[:2] == ["0", "1"] and int(got[2]) == -(-n // chunk), (name, chunk)


def test_split_pass_on_the_cpu_under_sanitizers_damaged_files(cpu_program, tmp_path):
    """The 3 x 200 damaged files tests/test_jpeg_split_gpu.py decodes on the device, first here: the program exits 0 - status 0
    exactly where the host pass accepts, equal coefficients there - and every group has both outcomes."""
    files = []
    for name in S.STATUS_FIXTURES:
        files += S.status_corruptions(name, _fixture(name))
    lines = _sweep(cpu_program, tmp_path, files, ((1, 3, 2), (32, 2, 1), (1, 64, 16)))
    for first in range(0, 600, 200):
        accepted = sum(head[0] == "0" for head, _ in lines[first:first + 200])
        assert 5 < accepted < 195, first
    for head, per in lines:
        if per is not None and head[1] == "0":
            assert all((got[0] == "0") == (head[0] == "0") for got in per)
