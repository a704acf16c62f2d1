"""The split mode of the JPEG Huffman pass on the GPU ("split over workgroups"), bit for bit against the
host pass tsod_jpeg_entropy_decode: the kernel entry alone on every fixture at nine (subseq_words, chunk_subseqs, overlap) triples
inside sentinel-padded buffers, with the chunks the stitch launch repaired counted; two calls and two workspace fills with the
same bits; one mixed batch through JPEGDecoder(split=...) against the pixels Pillow decoded, with the launches counted; the two
large files with and without repairs; the status word on 3 x 200 damaged files (run on the CPU first,
tests/test_jpeg_split_abi.py); and entropy="device" without split unchanged.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_scan_restated as S  # noqa: E402
from test_jpeg_huffman_gpu import _device_copy, _fixture, _guarded, _guards_intact, _large, _prepare  # noqa: E402
from test_jpeg_restated import fixtures, rounds  # noqa: E402
from test_jpeg_split_abi import ROUND_TRIPLES, TRIPLES  # noqa: E402

pytestmark = pytest.mark.gpu

# chunks repaired over all 87 fixtures, counted lane by lane on the CPU (tests/jpeg_huffman_split_main.cpp): the scheme fixes them
REPAIRED = {(1, 3, 0): 2990, (1, 5, 251): 76, (2, 64, 16): 22, (32, 256, 0): 0}


def _launch(dev, prep, triple, fill=0xA5):
    """The split entry alone: (coefficients int16, status int32, repaired int32 ndarrays, chunk count), the guards of the
    coefficients, the status words, the workspace and `repaired` checked."""
    from two_stage_object_detection_amd import hip_ops
    words, chunk, overlap = triple
    plan, segments = prep["plan"], prep["segments"]
    chunks, n_subseqs = hip_ops.jpeg_split_chunks(segments, words, chunk)
    coef_whole, coef = _guarded(dev, 2 * plan["coef_count"])
    status_whole, status = _guarded(dev, 4 * len(prep["infos"]))
    work_whole, workspace = _guarded(dev, hip_ops.jpeg_huffman_split_workspace_bytes(n_subseqs, len(chunks), len(segments)))
    repaired_whole, repaired = _guarded(dev, 4 * len(segments))
    workspace.fill_(fill)
    hip_ops.jpeg_huffman_split(plan["table"], _device_copy(plan["table"], dev), segments, _device_copy(segments, dev), chunks,
                               _device_copy(chunks, dev), _device_copy(prep["stream"], dev), _device_copy(prep["huff"], dev),
                               coef.view(torch.int16), status.view(torch.int32), words, chunk, overlap, workspace, repaired.view(torch.int32))
    torch.cuda.synchronize()
    assert all(_guards_intact(w) for w in (coef_whole, status_whole, work_whole, repaired_whole))
    return coef.view(torch.int16).cpu().numpy(), status.view(torch.int32).cpu().numpy(), repaired.view(torch.int32).cpu().numpy(), len(chunks)


@pytest.fixture(scope="module")
def every_fixture():
    return _prepare([data for _, data, _ in fixtures()[0]])


def _equals_host_pass(prep, coef):
    table = prep["plan"]["table"]
    for i, info in enumerate(prep["infos"]):
        first = table[i].coef_offset[0]
        assert np.array_equal(coef[first:first + info.coef_total], prep["want"][i]), i
    assert coef.size == sum(info.coef_total for info in prep["infos"])


@pytest.mark.parametrize("triple", TRIPLES)
def test_split_entry_equals_host_pass_on_every_fixture(dev, every_fixture, triple):
    """All 87 fixtures - grey, 1x1, 2x1, 2x2, with and without restart markers - in ONE call: from one chunk per 32-bit
    subsequence, every one of them repaired in turn, to one chunk per segment, which is the unsplit pass in three launches."""
    prep = every_fixture
    coef, status, repaired, n_chunks = _launch(dev, prep, triple)
    assert not status.any()
    _equals_host_pass(prep, coef)
    n_segments = len(prep["segments"])
    assert repaired.shape == (n_segments,) and (repaired >= 0).all()
    accepted = n_chunks - n_segments - int(repaired.sum())           # without a true error every boundary is looked at
    assert accepted >= 0
    if triple in REPAIRED:
        assert int(repaired.sum()) == REPAIRED[triple]
    if triple == (1, 3, 0):
        assert repaired.sum() > 0
    if triple == (1, 5, 251):
        assert accepted > 0 and repaired.sum() > 0
    if triple == (32, 256, 0):
        assert n_chunks == n_segments


@pytest.mark.parametrize("triple", ROUND_TRIPLES)
def test_split_entry_at_the_round_boundaries(dev, triple):
    """tests/golden/jpeg_rounds.npz - segments of 256, 257, 512 and 513 one-word subsequences - in chunks of a whole round, of a
    round less one lane after one lane of warm-up, and of half a round: the host pass's coefficients, status 0, the guards
    intact, and Pillow's pixels through the decoder."""
    from two_stage_object_detection_amd.dataset import image_io
    cases = rounds()
    files = [data for _, data, _, _ in cases]
    prep = _prepare(files)
    coef, status, repaired, n_chunks = _launch(dev, prep, triple)
    assert not status.any()
    _equals_host_pass(prep, coef)
    assert n_chunks == sum(-(-n // triple[1]) for _, _, _, n in cases) and repaired.shape == (len(cases),)
    decoder = image_io.JPEGDecoder(dev, threads=2, entropy="device", subseq_bits=32 * triple[0], split=triple[1:])
    for t, (name, _, pixels, _) in zip(decoder.batch(files), cases):
        assert np.array_equal(t.cpu().numpy(), pixels), (name, triple)
    decoder.raise_if_corrupt()


def test_same_bits_from_two_calls_and_from_any_workspace_fill(dev, every_fixture):
    first = _launch(dev, every_fixture, (1, 3, 2), fill=0xA5)
    again = _launch(dev, every_fixture, (1, 3, 2), fill=0xA5)
    zeros = _launch(dev, every_fixture, (1, 3, 2), fill=0)
    assert first[2].sum() > 0
    for other in (again, zeros):
        assert all(np.array_equal(a, b) for a, b in zip(first[:3], other[:3]))


def _counted(monkeypatch):
    from two_stage_object_detection_amd import hip_ops
    counts = {"huffman": 0, "split": 0, "idct": 0, "to_rgb": 0}
    captured = {}
    huffman, split, idct, to_rgb = hip_ops.jpeg_huffman, hip_ops.jpeg_huffman_split, hip_ops.jpeg_idct, hip_ops.jpeg_to_rgb

    def counted_split(*a):
        counts["split"] += 1
        captured["table"], captured["coef"], captured["chunks"] = a[0], a[8], a[4]
        return split(*a)

    monkeypatch.setattr(hip_ops, "jpeg_huffman", lambda *a: counts.__setitem__("huffman", counts["huffman"] + 1) or huffman(*a))
    monkeypatch.setattr(hip_ops, "jpeg_huffman_split", counted_split)
    monkeypatch.setattr(hip_ops, "jpeg_idct", lambda *a: counts.__setitem__("idct", counts["idct"] + 1) or idct(*a))
    monkeypatch.setattr(hip_ops, "jpeg_to_rgb", lambda *a: counts.__setitem__("to_rgb", counts["to_rgb"] + 1) or to_rgb(*a))
    return counts, captured


def test_mixed_batch_is_one_split_call_and_equals_pillow(dev, monkeypatch):
    from two_stage_object_detection_amd.dataset import image_io
    counts, captured = _counted(monkeypatch)
    decoder = image_io.JPEGDecoder(dev, threads=4, entropy="device", subseq_bits=64, split=(64, 16))
    cases = fixtures()[0]
    out = decoder.batch([data for _, data, _ in cases])
    assert counts == {"huffman": 0, "split": 1, "idct": 1, "to_rgb": 1}
    n_segments = int(captured["chunks"][-1, 0]) + 1
    assert decoder.repaired.dtype == torch.int32 and decoder.repaired.shape == (n_segments,) and decoder.repaired.device == out[0].device
    assert n_segments > len(cases) + 100 and len(captured["chunks"]) > n_segments
    assert decoder.status.dtype == torch.int32 and decoder.status.shape == (len(cases),)
    for t, (name, _, pixels) in zip(out, cases):
        assert t.data_ptr() % 256 == 0 and t.is_contiguous(), name
        assert np.array_equal(t.cpu().numpy(), pixels), name
    assert not decoder.status.cpu().numpy().any()
    assert int(decoder.repaired.sum()) == REPAIRED[(2, 64, 16)]
    decoder.raise_if_corrupt()
    # the conveniences pass the keyword through
    one = image_io.decode_jpeg(cases[40][1], dev, entropy="device", split=(3, 2))
    assert np.array_equal(one.cpu().numpy(), cases[40][2]) and counts["split"] == 2 and counts["huffman"] == 0


def test_large_files_with_and_without_repairs(dev):
    """tests/golden/jpeg_large.npz at the default subsequence length: three chunks per file whose entries, after 32 x 1024 bits of
    warm-up, are the true ones; and chunks of two subsequences without warm-up, every one repaired in turn."""
    from two_stage_object_detection_amd.dataset import image_io
    files = [data for _, data in _large()]
    host = [t.cpu().numpy() for t in image_io.JPEGDecoder(dev, threads=2, entropy="host").batch(files)]
    default = image_io.JPEGDecoder(dev, threads=2, entropy="device", split=True)
    assert default.split == (224, 32) and default.subseq_bits == image_io.JPEGDecoder(dev).subseq_bits
    got = default.batch(files)
    assert default.repaired.shape == (2,) and int(default.repaired.sum()) == 0
    assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(host, got))
    default.raise_if_corrupt()
    serial = image_io.JPEGDecoder(dev, threads=2, entropy="device", split=(2, 0))
    got = serial.batch(files)
    assert int(serial.repaired.sum()) > 500
    assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(host, got))
    serial.raise_if_corrupt()


@pytest.mark.parametrize("name", S.STATUS_FIXTURES)
def test_status_is_nonzero_exactly_where_the_host_pass_refuses(dev, monkeypatch, name):
    """200 seeded single-byte corruptions of one fixture's entropy-coded segment as ONE split batch of 32-bit subsequences in
    chunks of three (those the sweep refuses itself stay on the host): status nonzero exactly where the host pass refuses, equal
    coefficients where it accepts, the sentinels around every device buffer the decoder allocates intact."""
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.dataset import image_io
    files = []
    for data in S.status_corruptions(name, _fixture(name)):
        status, info = hip_ops.jpeg_parse(data)
        assert status == 0
        cap_bytes, cap_segs = hip_ops.jpeg_scan_sizes(info, len(data))
        rc, _, _ = hip_ops.jpeg_scan_prepare(data, np.zeros(cap_bytes, dtype=np.uint8), np.zeros(cap_segs, dtype=hip_ops.jpeg_segment_dtype()),
                                             np.zeros(hip_ops.JPEG_HUFF_BYTES, dtype=np.uint8))
        if rc == 0:
            files.append(data)
    assert len(files) > 150
    want = []
    for data in files:
        _, info = hip_ops.jpeg_parse(data)
        coef = np.zeros(info.coef_total, dtype=np.int16)
        want.append(coef if hip_ops.jpeg_entropy_decode(data, coef) == 0 else None)
    bad = [i for i, w in enumerate(want) if w is None]
    assert 5 < len(bad) < len(files) - 5
    counts, captured = _counted(monkeypatch)
    wholes = []

    def guarded_empty(nbytes, device):
        whole, inner = _guarded(device, nbytes)
        wholes.append(whole)
        return inner

    monkeypatch.setattr(image_io, "_empty", guarded_empty)
    decoder = image_io.JPEGDecoder(dev, threads=4, entropy="device", subseq_bits=32, split=(3, 2))
    out = decoder.batch(files)
    torch.cuda.synchronize()
    assert counts == {"huffman": 0, "split": 1, "idct": 1, "to_rgb": 1}
    assert len(wholes) == 6                                          # coef, planes, out, status, workspace, repaired
    assert all(_guards_intact(w) for w in wholes)
    status = decoder.status.cpu().numpy()
    assert [i for i in range(len(files)) if status[i] != 0] == bad
    assert all(t.shape == out[0].shape for t in out)
    coef, table = captured["coef"].cpu().numpy(), captured["table"]
    for i, w in enumerate(want):
        if w is not None:
            first = table[i].coef_offset[0]
            assert np.array_equal(coef[first:first + w.size], w), i
    with pytest.raises(image_io.CorruptJPEG, match=rf"item {bad[0]}\b"):
        decoder.raise_if_corrupt()


def test_device_mode_without_split_is_unchanged(dev, monkeypatch):
    from two_stage_object_detection_amd.dataset import image_io
    counts, _ = _counted(monkeypatch)
    cases = fixtures()[0][::5]
    decoder = image_io.JPEGDecoder(dev, threads=4, entropy="device")
    assert decoder.split is None
    out = decoder.batch([data for _, data, _ in cases])
    assert counts == {"huffman": 1, "split": 0, "idct": 1, "to_rgb": 1} and decoder.repaired is None
    for t, (name, _, pixels) in zip(out, cases):
        assert np.array_equal(t.cpu().numpy(), pixels), name
