"""Active dropout restated in NumPy: Philox4x32-10, the mask of a logical tensor [pixels, C] and the
masked multiply - what csrc/philox.h and csrc/dropout.hip are tested against, bit for bit.

    e    = e0 + pixel * C + c                                      (uint64)
    word = lane (e & 3) of philox((lo32(e >> 2), hi32(e >> 2), ordinal, 0), key)
    thr  = llround(double(float32(p)) * 2^32)                      keep iff word >= thr (in 64 bits)
    y    = keep ? x * scale : 0                                    scale = float32(1 / (1 - double(float32(p)))), 0 for p = 1
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0 = np.uint64(M0) * c[0]                              # (32 x 32 bits: exact in uint64)
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
    return [v.astype(np.uint32) for v in c]


def params(p, as_float32=True):
    """(thr, scale) of a probability; ``p`` arrives as a C float unless ``as_float32`` is off (thr of the double itself)."""
    pd = float(np.float32(p)) if as_float32 else float(p)
    if not 0.0 <= pd <= 1.0:
        raise ValueError(p)
    thr = int(np.floor(pd * 4294967296.0 + 0.5))              # llround: halves away from zero (pd >= 0)
    scale = np.float32(1.0 / (1.0 - pd)) if pd < 1.0 else np.float32(0.0)
    return thr, scale


def words(n, key, ordinal=0, e0=0):
    """The random words of elements e0 .. e0 + n - 1 (uint32 [n])."""
    first, last = e0 >> 2, (e0 + n - 1) >> 2
    ctr = np.arange(first, last + 1, dtype=np.uint64) if n else np.zeros(0, dtype=np.uint64)
    out = philox4x32_10((ctr & MASK32, ctr >> np.uint64(32), ordinal, 0), key)
    flat = np.stack(out, axis=1).reshape(-1)
    lo = e0 - 4 * first
    return flat[lo:lo + n]


def keep_mask(pixels, C, p, key, ordinal=0, e0=0, thr=None):
    """bool [pixels, C]: the elements kept."""
    thr = params(p)[0] if thr is None else thr
    return (words(pixels * C, key, ordinal, e0).astype(np.uint64) >= np.uint64(thr)).reshape(pixels, C)


def dropout(x, p, key, ordinal=0, e0=0):
    """x float32 [pixels, C] (logical channels) -> keep ? x * scale : 0 in float32."""
    x = np.asarray(x, dtype=np.float32)
    keep = keep_mask(x.shape[0], x.shape[1], p, key, ordinal, e0)
    return np.where(keep, x * params(p)[1], np.float32(0.0)).astype(np.float32)


def dropout_segs(src, dst, segs, C, p, key, ordinal=0, e0=0):
    """The kernel's contract on buffers [pixels, pitch]: slice (off, real, first) of ``dst`` gets the dropped logical channels
    [first, first + real) read from the same lanes of ``src``, its pad lanes 0, everything else of ``dst`` stays -> a new array."""
    src, out = np.asarray(src, dtype=np.float32), np.array(dst, dtype=np.float32, copy=True)
    logical = np.zeros((src.shape[0], C), dtype=np.float32)
    for off, real, first in segs:
        logical[:, first:first + real] = src[:, off:off + real]
    y = dropout(logical, p, key, ordinal, e0)
    for off, real, first in segs:
        out[:, off:off + real] = y[:, first:first + real]
        out[:, off + real:off + (real + 3) // 4 * 4] = 0.0
    return out
