"""The JPEG Huffman pass on the GPU (entropy="device"), bit for bit against the host pass
tsod_jpeg_entropy_decode: the kernel entry alone on every fixture at subsequences of 1, 2, 3 and 32 words inside sentinel-padded
buffers; one mixed batch through JPEGDecoder(entropy="device") against the pixels Pillow decoded, with the launches counted; files
long enough for three rounds at the default subsequence length; the status word on 3 x 200 damaged files (swept on the CPU first,
tests/test_jpeg_scan_abi.py); and entropy="host" unchanged.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_scan_restated as S  # noqa: E402
from test_jpeg_restated import fixtures, rounds  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 256                                                            # sentinel bytes on both sides of a device buffer
SENTINEL = 0xA5


def _fixture(name):
    for n, data, pixels in fixtures()[0]:
        if n == name:
            return data
    raise KeyError(name)


def _large():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_large.npz"))
    return [(str(n), z[f"file_{i}"].tobytes()) for i, n in enumerate(z["names"])]


def _prepare(files):
    """What one Huffman launch over `files` needs, made on the host with the library's own sweep, and the host pass's
    coefficients of every file (None where it refuses)."""
    from two_stage_object_detection_amd import hip_ops
    infos = []
    for data in files:
        status, info = hip_ops.jpeg_parse(data)
        assert status == 0
        infos.append(info)
    plan = hip_ops.jpeg_plan(infos)
    segments, streams, tables, want, at = [], [], [], [], 0
    for i, (data, info) in enumerate(zip(files, infos)):
        cap_bytes, cap_segs = hip_ops.jpeg_scan_sizes(info, len(data))
        stream, segs = np.zeros(cap_bytes, dtype=np.uint8), np.zeros(cap_segs, dtype=hip_ops.jpeg_segment_dtype())
        huff = np.zeros(hip_ops.JPEG_HUFF_BYTES, dtype=np.uint8)
        status, n_bytes, n_segs = hip_ops.jpeg_scan_prepare(data, stream, segs, huff)
        assert status == 0 and n_bytes % 4 == 0
        segs = segs[:n_segs]
        segs["image"] = i
        segs["stream_offset"] += at
        at += n_bytes
        segments.append(segs), streams.append(stream[:n_bytes]), tables.append(huff)
        coef = np.zeros(info.coef_total, dtype=np.int16)
        want.append(coef if hip_ops.jpeg_entropy_decode(data, coef) == 0 else None)
    segments = np.ascontiguousarray(np.concatenate(segments))
    work = np.zeros((len(segments), 4), dtype=np.int32)
    work[:, 0] = np.arange(len(segments))
    return dict(infos=infos, plan=plan, segments=segments, work=work, stream=np.concatenate(streams), huff=np.concatenate(tables), want=want)


def _guarded(dev, nbytes):
    """(whole, inner): a sentinel-filled u8 device buffer and the `nbytes` in its middle."""
    whole = torch.full((nbytes + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    return whole, whole[PAD:PAD + nbytes]


def _guards_intact(whole):
    host = whole.cpu().numpy()
    return bool((host[:PAD] == SENTINEL).all() and (host[-PAD:] == SENTINEL).all())


def _device_copy(obj, dev):
    raw = np.frombuffer(bytes(obj), dtype=np.uint8) if not isinstance(obj, np.ndarray) else obj.reshape(-1).view(np.uint8)
    return torch.from_numpy(raw.copy()).to(dev)


def _launch(dev, prep, words):
    """The kernel entry alone: (coefficients int16 ndarray, status int32 ndarray), the guards of both buffers checked."""
    from two_stage_object_detection_amd import hip_ops
    plan = prep["plan"]
    coef_whole, coef = _guarded(dev, 2 * plan["coef_count"])
    status_whole, status = _guarded(dev, 4 * len(prep["infos"]))
    hip_ops.jpeg_huffman(plan["table"], _device_copy(plan["table"], dev), prep["segments"], _device_copy(prep["segments"], dev),
                         prep["work"], _device_copy(prep["work"], dev), _device_copy(prep["stream"], dev), _device_copy(prep["huff"], dev),
                         coef.view(torch.int16), status.view(torch.int32), words)
    torch.cuda.synchronize()
    assert _guards_intact(coef_whole) and _guards_intact(status_whole)
    return coef.view(torch.int16).cpu().numpy(), status.view(torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def every_fixture():
    return _prepare([data for _, data, _ in fixtures()[0]])


@pytest.mark.parametrize("words", [1, 2, 3, 32])
def test_kernel_entry_equals_host_pass_on_every_fixture(dev, every_fixture, words):
    """All 87 fixtures - grey, 1x1, 2x1, 2x2, with and without restart markers, one-block and one-row intervals - in ONE launch.
    At one word per subsequence the 8222-byte file is close to 1900 subsequences (eight rounds with carries), and symbols
    longer than a subsequence leave lanes without a symbol start."""
    prep = every_fixture
    longest = int(prep["segments"]["bit_length"].max())
    assert longest > 7 * 256 * 32 and len(prep["segments"]) > len(prep["infos"]) + 100
    coef, status = _launch(dev, prep, words)
    assert not status.any()
    table = prep["plan"]["table"]
    for i, ((name, _, _), info) in enumerate(zip(fixtures()[0], prep["infos"])):
        first = table[i].coef_offset[0]
        assert np.array_equal(coef[first:first + info.coef_total], prep["want"][i]), (name, words)
    assert coef.size == sum(info.coef_total for info in prep["infos"])


def _counted(monkeypatch):
    from two_stage_object_detection_amd import hip_ops
    counts = {"huffman": 0, "idct": 0, "to_rgb": 0}
    captured = {}
    huffman, idct, to_rgb = hip_ops.jpeg_huffman, hip_ops.jpeg_idct, hip_ops.jpeg_to_rgb

    def counted_huffman(*a):
        counts["huffman"] += 1
        captured["table"], captured["coef"] = a[0], a[8]
        return huffman(*a)

    monkeypatch.setattr(hip_ops, "jpeg_huffman", counted_huffman)
    monkeypatch.setattr(hip_ops, "jpeg_idct", lambda *a: counts.__setitem__("idct", counts["idct"] + 1) or idct(*a))
    monkeypatch.setattr(hip_ops, "jpeg_to_rgb", lambda *a: counts.__setitem__("to_rgb", counts["to_rgb"] + 1) or to_rgb(*a))
    return counts, captured


def test_mixed_batch_is_one_huffman_launch_and_equals_pillow(dev, monkeypatch):
    from two_stage_object_detection_amd.dataset import image_io
    counts, _ = _counted(monkeypatch)
    decoder = image_io.JPEGDecoder(dev, threads=4, entropy="device")
    cases = fixtures()[0]
    out = decoder.batch([data for _, data, _ in cases])
    assert counts == {"huffman": 1, "idct": 1, "to_rgb": 1}
    assert decoder.status.dtype == torch.int32 and decoder.status.shape == (len(cases),) and decoder.status.device == out[0].device
    base = out[0].untyped_storage().data_ptr()
    for t, (name, _, pixels) in zip(out, cases):
        assert t.untyped_storage().data_ptr() == base and t.data_ptr() % 256 == 0 and t.is_contiguous(), name
        assert np.array_equal(t.cpu().numpy(), pixels), name
    assert not decoder.status.cpu().numpy().any()
    decoder.raise_if_corrupt()
    # the conveniences pass the keyword through
    one = image_io.decode_jpeg(cases[40][1], dev, entropy="device")
    assert np.array_equal(one.cpu().numpy(), cases[40][2]) and counts["huffman"] == 2


def test_three_rounds_at_the_default_subsequence_length(dev):
    """tests/golden/jpeg_large.npz: a 4:2:0 and a 4:4:4 noise-textured file without restart markers, each one workgroup that
    walks at least three rounds of 256 default-length subsequences, carrying state, block count and DC sums between them."""
    from two_stage_object_detection_amd.dataset import image_io
    decoder = image_io.JPEGDecoder(dev, threads=2, entropy="device")
    files = [data for _, data in _large()]
    prep = _prepare(files)
    assert len(prep["segments"]) == 2 and {(i.hmax, i.vmax) for i in prep["infos"]} == {(2, 2), (1, 1)}
    assert int(prep["segments"]["bit_length"].min()) > 2 * 256 * decoder.subseq_bits
    coef, status = _launch(dev, prep, decoder.subseq_bits // 32)
    assert not status.any()
    table = prep["plan"]["table"]
    for i, info in enumerate(prep["infos"]):
        first = table[i].coef_offset[0]
        assert np.array_equal(coef[first:first + info.coef_total], prep["want"][i]), i
    got = [t.cpu().numpy() for t in decoder.batch(files)]
    decoder.raise_if_corrupt()
    decoder.entropy = "host"                                         # the same decoder, the host pass
    for a, t in zip(got, decoder.batch(files)):
        assert np.array_equal(a, t.cpu().numpy())
    assert decoder.status is None
    try:
        import io
        from PIL import Image
    except ImportError:
        return
    for a, data in zip(got, files):
        assert np.array_equal(a, np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


@pytest.mark.parametrize("words", [1, 2])
def test_round_boundaries(dev, words):
    """tests/golden/jpeg_rounds.npz: one workgroup each for a segment of 256, 257, 512 and 513 one-word subsequences, and of
    256 and 257 two-word ones - a last round that is full, and a last round of one lane that starts from the carried state.
    The host pass's coefficients, status 0, the guards intact, and Pillow's pixels through the decoder."""
    from two_stage_object_detection_amd.dataset import image_io
    cases = [c for c in rounds() if words == 1 or c[3] >= 512]
    files = [data for _, data, _, _ in cases]
    prep = _prepare(files)
    assert len(prep["segments"]) == len(cases)
    assert [int(-(-b // (32 * words))) for b in prep["segments"]["bit_length"]] == ([256, 257, 512, 513] if words == 1 else [256, 257])
    coef, status = _launch(dev, prep, words)
    assert not status.any()
    table = prep["plan"]["table"]
    for i, ((name, _, _, _), info) in enumerate(zip(cases, prep["infos"])):
        first = table[i].coef_offset[0]
        assert np.array_equal(coef[first:first + info.coef_total], prep["want"][i]), (name, words)
    decoder = image_io.JPEGDecoder(dev, threads=2, entropy="device", subseq_bits=32 * words)
    for t, (name, _, pixels, _) in zip(decoder.batch(files), cases):
        assert np.array_equal(t.cpu().numpy(), pixels), (name, words)
    decoder.raise_if_corrupt()


@pytest.mark.parametrize("name", S.STATUS_FIXTURES)
def test_status_is_nonzero_exactly_where_the_host_pass_refuses(dev, monkeypatch, name):
    """200 seeded single-byte corruptions of one fixture's entropy-coded segment as ONE batch (those that damage a restart marker
    are refused on the host, before anything is uploaded, and are checked to be): status nonzero exactly where the host pass
    refuses, equal coefficients where it accepts, the sentinels around the coefficient buffer and around the pixels intact."""
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.dataset import image_io
    files, refused_early = [], 0
    for data in S.status_corruptions(name, _fixture(name)):
        status, info = hip_ops.jpeg_parse(data)
        assert status == 0                                           # (the draws lie behind the markers)
        cap_bytes, cap_segs = hip_ops.jpeg_scan_sizes(info, len(data))
        rc, _, _ = hip_ops.jpeg_scan_prepare(data, np.zeros(cap_bytes, dtype=np.uint8), np.zeros(cap_segs, dtype=hip_ops.jpeg_segment_dtype()),
                                             np.zeros(hip_ops.JPEG_HUFF_BYTES, dtype=np.uint8))
        if rc:
            refused_early += 1
            assert hip_ops.jpeg_entropy_decode(data, np.zeros(info.coef_total, dtype=np.int16)) == -1
            with pytest.raises(image_io.CorruptJPEG, match="item 1"):
                image_io.JPEGDecoder(dev, entropy="device").batch([_fixture(name), data])
        else:
            files.append(data)
    assert len(files) + refused_early == 200 and len(files) > 150
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
    decoder = image_io.JPEGDecoder(dev, threads=4, entropy="device")
    out = decoder.batch(files)
    torch.cuda.synchronize()
    assert counts == {"huffman": 1, "idct": 1, "to_rgb": 1} and len(wholes) == 4          # coef, planes, out, status
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


def test_host_mode_is_unchanged(dev, monkeypatch):
    from two_stage_object_detection_amd.dataset import image_io
    counts, _ = _counted(monkeypatch)
    cases = fixtures()[0][::5]
    files = [data for _, data, _ in cases]
    default = image_io.JPEGDecoder(dev, threads=4).batch(files)
    assert counts == {"huffman": 0, "idct": 1, "to_rgb": 1}
    named = image_io.JPEGDecoder(dev, threads=4, entropy="host")
    host = named.batch(files)
    assert counts == {"huffman": 0, "idct": 2, "to_rgb": 2} and named.status is None
    for a, b, (name, _, pixels) in zip(default, host, cases):
        assert torch.equal(a, b) and np.array_equal(b.cpu().numpy(), pixels), name
