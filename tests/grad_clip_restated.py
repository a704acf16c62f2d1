"""Shared by tests/test_grad_clip.py and tests/test_grad_clip_gpu.py: the gradient norm of DESIGN.md section 4.16 restated in
numpy in the order include/tsod.h states (chunks of 2048 elements, thread t of 256 owns quads t, t + 256, ... of its chunk,
exact float64 squares added in ascending element order, a binary tree over the 256 threads, the partials thread-strided and
the same tree again), the float64 definition sqrt(sum(g.double() ** 2)), and seeded gradients in the style of
adamw_restated.draw_grads."""
import numpy as np
import torch

CHUNK, THREADS = 2048, 256
SIZES = (1, 3, 18, 2047, 2048, 2049, 4100)


def draw_grads(sizes=SIZES, seed=5, scale=1.0):
    """One gradient per size: magnitudes scale * 10^U(-6, 1), random signs, about 5 % exact zeros, every seventh element zero."""
    g = torch.Generator().manual_seed(seed)
    row = []
    for n in sizes:
        mag = 10.0 ** (torch.rand(n, generator=g) * 7 - 6)
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        x = (mag * sign * scale).float()
        x[torch.rand(n, generator=g) < 0.05] = 0
        x[3::7] = 0
        row.append(x)
    return row


def tree_sum_256(v):
    """t += t + 128, then + 64, ... + 1 over 256 float64 values; element 0 is the sum."""
    v = np.array(v, dtype=np.float64)
    assert v.shape == (THREADS,)
    st = THREADS // 2
    while st >= 1:
        v[:st] = v[:st] + v[st:2 * st]
        st //= 2
    return v[0]


def chunk_partial(g):
    """One chunk (at most 2048 float32 values) -> its float64 partial.  A thread that owns no element of a quad adds nothing;
    adding the +0.0 of a zero pad instead leaves every sum as it is (the squares are >= +0 or NaN)."""
    assert g.dtype == np.float32 and 0 < g.size <= CHUNK
    sq = np.zeros(CHUNK, dtype=np.float64)
    d = g.astype(np.float64)
    sq[:g.size] = d * d                                     # exact: 24-bit significands
    sq = sq.reshape(CHUNK // (4 * THREADS), THREADS, 4)     # [round][thread][element of the quad]
    acc = np.zeros(THREADS, dtype=np.float64)
    for r in range(sq.shape[0]):
        for k in range(4):
            acc = acc + sq[r, :, k]
    return tree_sum_256(acc)


def restated(grads, max_norm):
    """-> (sum_sq float64, norm float32, coef float32) over a list of float32 arrays / tensors, tensor by tensor."""
    with np.errstate(all="ignore"):
        partials = []
        for g in grads:
            g = np.ascontiguousarray(g.numpy() if isinstance(g, torch.Tensor) else g).reshape(-1)
            for first in range(0, g.size, CHUNK):
                partials.append(chunk_partial(g[first:first + CHUNK]))
        if not partials:
            return np.float64(0.0), np.float32(0.0), np.float32(1.0)
        acc = np.zeros(THREADS, dtype=np.float64)
        for k, p in enumerate(partials):                     # thread k % 256 adds its partials in ascending order
            acc[k % THREADS] = acc[k % THREADS] + p
        sum_sq = np.float64(tree_sum_256(acc))
        norm = np.float32(np.sqrt(sum_sq))
        return sum_sq, norm, coef_of(norm, max_norm)


def coef_of(norm, max_norm):
    """np.float32(max_norm) / (norm + np.float32(1e-6)), clamped as c > 1 ? 1 : c (a NaN stays a NaN)."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    assert c.dtype == np.float32
    return np.float32(1.0) if c > np.float32(1.0) else c


def exact_norm(grads):
    """The float64 definition: sqrt(sum(g.double() ** 2))."""
    total = torch.zeros((), dtype=torch.float64)
    for g in grads:
        g = torch.as_tensor(g)
        total = total + (g.double() ** 2).sum()
    return float(total.sqrt())


def bits(x):
    """The bit pattern of a float32 / float64 scalar, so that NaNs compare too."""
    x = np.asarray(x)
    return int(x.view(np.uint32 if x.dtype == np.float32 else np.uint64))


def same_bits(a, b):
    """Equal bit patterns, or both NaN (a NaN's sign and payload are not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype, (a.dtype, b.dtype)
    return bool(np.isnan(a) and np.isnan(b)) or bits(a) == bits(b)


def same_record(got, want):
    return all(same_bits(g, w) for g, w in zip(got, want))


def ulp_distance_f32(got, exact):
    """|got - exact| in units of float32(exact)'s ulp."""
    ref = np.float32(exact)
    return abs(float(got) - exact) / float(np.spacing(np.abs(ref)))
