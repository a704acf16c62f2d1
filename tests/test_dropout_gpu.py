"""tsod_dropout_segs_f32 on the GPU against tests/dropout_restated.py, bit for bit: slices and padding,
the ends of the probability range, a counter beyond 32 bits, the ordinal, the grid cap, short quads and quads that straddle two
counters, and run-to-run equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_restated as D  # noqa: E402

KEY = (0x1234, 0x5678)
SENTINEL = -777.25
GRID_CAP, THREADS = 4096, 256                  # csrc/dropout.hip: kDropMaxBlocks, kDropThreads


def same_bits(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), np.asarray(want, dtype=np.float32).view(np.uint32))


def buffers(pixels, pitch, seed, dev):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(pixels, pitch, generator=g)
    return src.to(dev), torch.full((pixels, pitch), SENTINEL).to(dev)


def run(src, dst, segs, C, p, dev, shape=None, **kw):
    """One launch on [pixels, pitch] buffers seen as NHWC ``shape`` -> (result, the restatement's)."""
    from two_stage_object_detection_amd import hip_ops
    want = D.dropout_segs(src.cpu().numpy(), dst.cpu().numpy(), segs, C, p, KEY, kw.get("ordinal", 0), kw.get("e0", 0))
    view = (lambda t: t if shape is None else t.view(*shape, t.shape[-1]))
    out = hip_ops.dropout(view(src), p, KEY, segs=segs, C=C, out=view(dst), **kw)
    assert out.data_ptr() == dst.data_ptr()
    return dst, want


SEGS = [(4, 6, 0), (16, 10, 6), (32, 2, 16)]   # real widths 6, 10, 2 at padded offsets of a pitch-40 pixel; C = 18


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", (False, True))
def test_slices_padding_and_untouched_channels(dev, in_place):
    """N=1, H=3, W=5: 270 elements, the last counter is partial.  Pad lanes come out 0, channels outside the slices keep the
    sentinel (out of place) or their values (in place)."""
    src, dst = buffers(15, 40, 1, dev)
    before = src.clone()
    got, want = run(src, src if in_place else dst, SEGS, 18, 0.5, dev, shape=(1, 3, 5))
    assert same_bits(got, want)
    host = got.cpu().numpy()
    touched = np.zeros(40, dtype=bool)
    for off, real, _ in SEGS:
        touched[off:off + (real + 3) // 4 * 4] = True
        assert not host[:, off + real:off + (real + 3) // 4 * 4].any()
    outside = before.cpu().numpy() if in_place else np.full((15, 40), SENTINEL, dtype=np.float32)
    assert np.array_equal(host[:, ~touched], outside[:, ~touched]) and (~touched).sum() == 16
    if not in_place:
        assert torch.equal(src, before)
    kept = host[:, [c for off, real, _ in SEGS for c in range(off, off + real)]] != 0
    assert 0 < kept.sum() < kept.size                                     # p = 0.5: some of both


@pytest.mark.gpu
@pytest.mark.parametrize("p", (0.0, 1.0, 0.1, 0.5))
def test_probabilities(dev, p):
    src, dst = buffers(64, 40, 2, dev)
    got, want = run(src, dst, SEGS, 18, p, dev, shape=(2, 4, 8))
    assert same_bits(got, want)
    if p in (0.0, 1.0):                                                   # p = 0 copies, p = 1 gives zeros
        for off, real, _ in SEGS:
            assert torch.equal(got[:, off:off + real], src[:, off:off + real] if p == 0.0 else torch.zeros_like(src[:, off:off + real]))
    # a plain contiguous NHWC tensor is one slice
    from two_stage_object_detection_amd import hip_ops
    x = torch.randn(2, 3, 5, 8, generator=torch.Generator().manual_seed(3)).to(dev)
    assert same_bits(hip_ops.dropout(x, p, KEY).view(-1, 8), D.dropout(x.cpu().numpy().reshape(-1, 8), p, KEY))


@pytest.mark.gpu
def test_counter_beyond_32_bits(dev):
    """e0 = 2^34 - 6: the counter's high word is 0 for the first 6 elements and 1 after them."""
    src, dst = buffers(15, 40, 4, dev)
    e0 = (1 << 34) - 6
    got, want = run(src, dst, SEGS, 18, 0.5, dev, e0=e0)
    assert same_bits(got, want)
    low = D.dropout_segs(src.cpu().numpy(), np.full((15, 40), SENTINEL, dtype=np.float32), SEGS, 18, 0.5, KEY, e0=e0 & 0xFFFFFFFF)
    assert not np.array_equal(want, low)                                  # (the high word matters)


@pytest.mark.gpu
def test_ordinals_give_different_masks(dev):
    src, dst = buffers(15, 40, 5, dev)
    got0, want0 = run(src, dst.clone(), SEGS, 18, 0.5, dev, ordinal=0)
    got1, want1 = run(src, dst.clone(), SEGS, 18, 0.5, dev, ordinal=1)
    assert same_bits(got0, want0) and same_bits(got1, want1) and not torch.equal(got0, got1)


@pytest.mark.gpu
def test_one_row_block_past_the_grid_cap(dev):
    """8 quads per pixel -> 32 rows per workgroup: one pixel more than 4096 workgroups take in one round."""
    rows = THREADS // 8
    pixels = GRID_CAP * rows + 1
    src, dst = buffers(pixels, 32, 6, dev)
    got, want = run(src, dst, [(0, 32, 0)], 32, 0.1, dev)
    assert same_bits(got, want)
    assert same_bits(got[-1:], want[-1:]) and bool((got[-1] != SENTINEL).all())


@pytest.mark.gpu
def test_short_quads_and_quads_across_two_counters(dev):
    """Widths 5 and 3 with C = 9 (odd): a slice's last quad is short (lane-by-lane loads), the element index of a quad's first
    lane takes every residue mod 4, so quads straddle two counters; then the table's 16 slices, every quad short; then 71 quads
    in one slice: more than one 64-quad sweep of a wave."""
    segs = [(0, 5, 0), (8, 3, 5), (12, 1, 8)]
    src, dst = buffers(77, 16, 7, dev)
    got, want = run(src, dst, segs, 9, 0.3, dev)
    assert same_bits(got, want)
    wide = [(4 * i, 3, 3 * i) for i in range(16)]
    src, dst = buffers(33, 64, 8, dev)
    got, want = run(src, dst, wide, 48, 0.3, dev)
    assert same_bits(got, want)
    big = [(0, 281, 0)]                                                   # 71 quads: a thread takes two, the last one short
    src, dst = buffers(9, 284, 9, dev)
    got, want = run(src, dst, big, 281, 0.3, dev)
    assert same_bits(got, want)


@pytest.mark.gpu
def test_same_call_twice_same_bits(dev):
    src, dst = buffers(15, 40, 10, dev)
    a, _ = run(src, dst.clone(), SEGS, 18, 0.1, dev)
    b, _ = run(src, dst.clone(), SEGS, 18, 0.1, dev)
    assert torch.equal(a, b)
    from two_stage_object_detection_amd import hip_ops
    key = hip_ops.dropout_key(dev, *KEY)
    assert key.cpu().tolist() == list(KEY)
    c = hip_ops.dropout(src, 0.1, key, segs=SEGS, C=18, out=dst.clone())
    assert torch.equal(a, c)
    hi = hip_ops.dropout_key(dev, 0xFFFFFFFF, 0x80000000)                 # (words beyond int32's positive range)
    assert [v & 0xFFFFFFFF for v in hi.cpu().tolist()] == [0xFFFFFFFF, 0x80000000]
