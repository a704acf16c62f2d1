"""The training-curve kernels on the GPU.  Every comparison is bit for bit against the NumPy restatement
(tests/plot_restated.py) - the EMA has the reference's own roundings, the painters are integer arithmetic beyond a handful of
f32 operations with one rounding each, so there is no tolerance - and on the WHOLE buffer, the bytes between 3 W and the row
pitch included.  A painted comparison also asserts that something was painted: an empty image must not pass on both sides."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plot_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
UNIT = (0.0, 1.0)


@pytest.fixture(scope="module")
def font():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops.draw_font5x7()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------- K1
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 4097])
def test_ema_scan_is_bit_identical(dev, n, rows):
    from two_stage_object_detection_amd import hip_ops
    pitch = n + 5
    buf = np.random.default_rng(n * 10 + rows).standard_normal((rows, pitch)).astype(np.float32)
    x = torch.from_numpy(buf).to(dev)[:, :n]                         # pitched rows
    for alpha in (0.0, 0.01, 0.5, 1.0):
        want = R.ema(buf[:, :n], alpha)
        got = hip_ops.ema_scan(x, alpha)
        assert got.shape == (rows, n) and np.array_equal(bits(got.cpu().numpy()), bits(want)), alpha
    out = torch.full((rows, pitch), 7.0, device=dev)                 # a pitched output: the padding stays
    hip_ops.ema_scan(x, 0.01, out=out[:, :n])
    assert np.array_equal(bits(out[:, :n].cpu().numpy()), bits(R.ema(buf[:, :n], 0.01))) and bool((out[:, n:] == 7.0).all())
    if rows == 1:
        assert np.array_equal(bits(hip_ops.ema_scan(x[0], 0.5).cpu().numpy()), bits(R.ema(buf[0, :n], 0.5)))


def test_ema_scan_non_finite_samples_and_repeats(dev):
    from two_stage_object_detection_amd import hip_ops
    x = np.random.default_rng(3).standard_normal((2, 200)).astype(np.float32)
    x[0, 70], x[1, 64], x[1, 130] = NAN, INF, -INF
    t = torch.from_numpy(x).to(dev)
    for alpha in (0.01, 0.5):
        want = R.ema(x, alpha)
        assert np.isnan(want[0, 70:]).all() and np.isfinite(want[0, :70]).all() and np.isinf(want[1, 64]) and np.isnan(want[1, 130:]).all()
        got = hip_ops.ema_scan(t, alpha).cpu().numpy()
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(hip_ops.ema_scan(t, alpha).cpu().numpy()), bits(got))             # two runs, the same bits


def test_ema_curve_and_training_log(dev, golden_dir):
    from two_stage_object_detection_amd.utils.utils import TrainingLog, ema_curve
    z = np.load(os.path.join(golden_dir, "ema_ref.npz"))
    x = torch.from_numpy(z["x"]).to(dev)
    log = TrainingLog(dev, capacity=4)
    for i in range(37):                                              # across three doublings: 4 -> 8 -> 16 -> 32 -> 64
        log.append(x[i] if i % 3 else float(z["x"][i]))
        assert len(log) == i + 1
    assert log.capacity == 64 and np.array_equal(bits(log.values.cpu().numpy()), bits(z["x"][:37]))
    for k, alpha in enumerate(z["alphas"]):
        want = bits(z[f"ema_{k}"])                                   # the reference's own values
        assert np.array_equal(bits(ema_curve(x, float(alpha)).cpu().numpy()), want)
        assert np.array_equal(bits(ema_curve(list(x[:50]), float(alpha)).cpu().numpy()), want[:50])              # 0-d tensors
        assert np.array_equal(bits(ema_curve([float(v) for v in z["x"][:50]], float(alpha), dev).cpu().numpy()), want[:50])
        assert np.array_equal(bits(log.ema(float(alpha)).cpu().numpy()), want[:37])
    assert ema_curve([], 0.01, dev).shape == (0,)


# --------------------------------------------------------------------------------------------------------------------- K2
@pytest.mark.parametrize("case", ["finite", "some_non_finite", "none_finite", "constant", "huge_pair", "empty", "long"])
def test_plot_limits(dev, case):
    from two_stage_object_detection_amd import hip_ops
    rng = np.random.default_rng(5)
    series = {
        "finite": [rng.standard_normal(300), rng.standard_normal(7) * 3 + 1],
        "some_non_finite": [np.array([1.5, NAN, -2.0, INF]), np.array([-INF, 9.25, NAN])],
        "none_finite": [np.array([NAN, INF, -INF])],
        "constant": [np.full(100, 2.75), np.array([2.75, NAN])],
        "huge_pair": [np.array([3e38, -3e38, 0.0])],
        "empty": [],
        "long": [rng.standard_normal(70001), rng.standard_normal(3), np.zeros(0), rng.standard_normal(5000) - 9],
    }[case]
    series = [np.asarray(s, dtype=np.float32) for s in series]
    want = R.limits(series)
    assert np.isfinite(want).all() and want[0] < want[1]
    got = hip_ops.plot_limits([torch.from_numpy(s).to(dev) for s in series], device=dev)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (got, want)
    if case in ("none_finite", "empty"):
        assert want.tolist() == [0.0, 1.0]
    if case == "constant":
        assert want.tolist() == [2.25, 3.25]


# --------------------------------------------------------------------------------------------------------------------- K3
H0, W0, RECT0 = 50, 40, (5, 8, 32, 37)                               # a 32 x 37 rectangle in a 40 x 50 image


def run_series(dev, series, x_range, lim=UNIT, H=H0, W=W0, rect=RECT0, row_pad=7, seed=0, repeat=1, expect_empty=False, fill=None):
    """Paint a pitched buffer (random bytes, or ``fill``) on the device and in NumPy; every byte must agree.  -> the painted
    [H, W, 3] view of the expected buffer, and the buffer as it was."""
    from two_stage_object_detection_amd import hip_ops
    row = 3 * W + row_pad
    buf = np.random.default_rng(seed).integers(0, 256, size=(H, row), dtype=np.uint8)
    if fill is not None:
        buf[:] = fill
    want = buf.copy()
    view = np.lib.stride_tricks.as_strided(want, shape=(H, W, 3), strides=(row, 3, 1))
    lim32 = np.asarray(lim, dtype=np.float32)
    painted = R.plot_series(view, rect, series, x_range, lim32)
    assert (painted == 0) == expect_empty, painted
    on_dev = [dict(s, y=torch.from_numpy(np.asarray(s["y"], dtype=np.float32)).to(dev)) for s in series]
    limits = torch.from_numpy(lim32).to(dev)
    for _ in range(repeat):
        t = torch.from_numpy(buf.copy()).to(dev)
        hip_ops.plot_series(t.as_strided((H, W, 3), (row, 3, 1)), rect, on_dev, x_range, limits)
        got = t.cpu().numpy()
        diff = np.argwhere(got != want)
        assert diff.size == 0, f"{len(diff)} bytes differ, first at (y, byte) = {diff[0].tolist()}"
    outside = np.ones((H, row), dtype=bool)
    px0, py0, pw, ph = rect
    outside[py0:py0 + ph, 3 * px0:3 * (px0 + pw)] = False
    assert np.array_equal(want[outside], buf[outside])               # nothing outside the rectangle, nothing beyond 3 W
    return view, buf


def wave(n, seed=1):
    rng = np.random.default_rng(seed)
    return (0.5 + 0.45 * np.sin(np.arange(n) * 0.37) * rng.random(n)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 8 * 32 + 3])
def test_series_lengths_around_the_rectangle_width(dev, n):
    pw = RECT0[2]
    assert n in (1, 2, pw - 1, pw, pw + 1, 8 * pw + 3)
    for w in (0, 1, 3):
        s = dict(y=wave(n, n), color=(200, 30, 40), alpha=255, width=w, marker="s" if w == 0 else None, marker_size=1)
        run_series(dev, [s], (0, max(n - 1, 0)), seed=n + w)
    run_series(dev, [dict(y=wave(n, n), width=2, alpha=90)], (-3, n + 4), seed=n)       # an abscissa range wider than the data


@pytest.mark.parametrize("marker", ["o", "s", "^"])
@pytest.mark.parametrize("size", [1, 5])
def test_markers_and_clipping_at_the_corners(dev, marker, size):
    corners = np.array([0, 1, 0.5, 1, 0], dtype=np.float32)          # the first and last column, the top and bottom row
    for w in (0, 1):
        s = dict(y=corners, color=(10, 200, 90), alpha=200, width=w, marker=marker, marker_size=size)
        run_series(dev, [s], (0, 4), seed=size)
    view, buf = run_series(dev, [dict(y=np.array([0.5], dtype=np.float32), width=0, marker=marker, marker_size=size, color=(1, 2, 3))],
                           (0, 0), seed=2)
    changed = (view != np.lib.stride_tricks.as_strided(buf, shape=view.shape, strides=view.strides)).any(axis=-1)
    assert int(changed.sum()) <= len(R.marker_pixels(R.MARKERS[marker], size))          # clipped at the left edge: column px0


def test_widths_and_a_rectangle_that_is_no_multiple_of_the_block(dev):
    from two_stage_object_detection_amd import _ffi
    rect = (3, 2, 45, 41)                                            # 45 columns: one full block of 32 and one of 13
    assert rect[2] % _ffi.PLOT_BLOCK_COLUMNS != 0
    for w in (0, 1, 2, 3, 15):
        for n in (7, 45, 500):
            s = dict(y=wave(n, w), color=(90, 60, 250), alpha=170, width=w, marker="^", marker_size=5 if n == 7 else 1)
            run_series(dev, [s], (0, n - 1), H=46, W=52, rect=rect, row_pad=1, seed=w)
    run_series(dev, [dict(y=wave(64), width=1)], (0, 63), H=37, W=32, rect=(0, 0, 32, 37), row_pad=0)        # the whole image


def test_dense_series(dev):
    n, rect = 200003, (11, 6, 701, 300)
    rng = np.random.default_rng(9)
    y = (np.exp(-np.arange(n) / 60000.0) + 0.08 * rng.standard_normal(n)).astype(np.float32)
    lim = R.limits([y])
    view, _ = run_series(dev, [dict(y=y, color=(0x1f, 0x77, 0xb4), alpha=128, width=1)], (0, n - 1), lim=lim, H=310, W=720, rect=rect,
                         row_pad=3, seed=4, repeat=2, fill=255)
    # independent of the restatement's segment code: with every column holding samples, column c's painted rows are exactly
    # min .. max of its samples' rows and of the boundary rows it shares with its neighbours (for two adjacent columns the
    # segment rule gives r_a + floor((r_b - r_a + 1) / 2), from the last sample of one to the first of the next)
    px0, py0, pw, ph = rect
    cols = np.array(R.columns(n, 0, 1, 0, n - 1, px0, pw))
    rows = R.rows_of(y, lim, py0, ph)
    assert len(np.unique(cols)) == pw
    first = np.searchsorted(cols, np.arange(px0, px0 + pw))
    last = np.append(first[1:], n) - 1
    boundary = [int(rows[last[k]]) + (int(rows[first[k + 1]]) - int(rows[last[k]]) + 1) // 2 for k in range(pw - 1)]
    painted = (view[py0:py0 + ph, px0:px0 + pw] != 255).any(axis=-1)          # (the buffer was white; the device's bytes equal these)
    for k in range(pw):
        rs = [int(rows[first[k]:last[k] + 1].min()), int(rows[first[k]:last[k] + 1].max())]
        rs += [boundary[k - 1]] if k > 0 else []
        rs += [boundary[k]] if k < pw - 1 else []
        want = np.zeros(ph, dtype=bool)
        want[min(rs) - py0:max(rs) - py0 + 1] = True
        assert np.array_equal(painted[:, k], want), k


def test_constant_series_paints_one_row(dev):
    from two_stage_object_detection_amd import hip_ops
    n = 20
    img = torch.zeros((H0, W0, 3), dtype=torch.uint8, device=dev)
    hip_ops.plot_series(img, RECT0, [dict(y=torch.full((n,), 0.25, device=dev), color=(255, 255, 255))], (0, 39),
                        torch.tensor(UNIT, device=dev))
    on = img.cpu().numpy()[..., 0] == 255
    px0, py0, pw, ph = RECT0
    row = py0 + (ph - 1) - 9                                         # rint(0.25 * 36) = 9
    c_last = px0 + (19 * (pw - 1)) // 39
    want = np.zeros((H0, W0), dtype=bool)
    want[row, px0:c_last + 1] = True
    assert np.array_equal(on, want) and int(on.sum()) == c_last - px0 + 1


def test_crossing_series_order_and_single_blend(dev):
    from two_stage_object_detection_amd import hip_ops
    up = dict(y=np.linspace(0, 1, 64, dtype=np.float32), color=(255, 0, 0), alpha=255, width=3)
    down = dict(y=np.linspace(1, 0, 64, dtype=np.float32), color=(0, 0, 255), alpha=128, width=3)
    view, buf = run_series(dev, [up, down], (0, 63), seed=6, repeat=2)
    before = np.lib.stride_tricks.as_strided(buf, shape=view.shape, strides=view.strides)
    lim = np.asarray(UNIT, dtype=np.float32)
    cov_up, cov_down = (R.series_coverage(s, RECT0, (0, 63), lim) for s in (up, down))
    both = cov_up & cov_down
    assert both.any() and (cov_up & ~cov_down).any()
    px0, py0, pw, ph = RECT0
    inner, src = view[py0:py0 + ph, px0:px0 + pw].astype(np.int64), before[py0:py0 + ph, px0:px0 + pw].astype(np.int64)
    # the later series wins where they cross: blue at alpha 128 over the red already there, blended exactly once
    assert np.array_equal(inner[both], np.broadcast_to((128 * np.array([0, 0, 255]) + 127 * np.array([255, 0, 0]) + 127) // 255, inner[both].shape))
    # a dense overlap of the series with itself (width 3: every pixel is covered by several segments) is still one blend
    only_down = cov_down & ~cov_up
    assert np.array_equal(inner[only_down], (128 * np.array([0, 0, 255]) + 127 * src[only_down] + 127) // 255)
    assert np.array_equal(inner[~(cov_up | cov_down)], src[~(cov_up | cov_down)])
    # the other order gives another image
    other, _ = run_series(dev, [down, up], (0, 63), seed=6)
    assert not np.array_equal(other, view)
    # alpha 0 leaves the series out
    run_series(dev, [dict(up, alpha=0)], (0, 63), expect_empty=True)
    t = torch.zeros((H0, W0, 3), dtype=torch.uint8, device=dev)
    assert hip_ops.plot_series(t, RECT0, [], (0, 1), torch.tensor(UNIT, device=dev)) is t and not bool(t.any())


def test_nan_gaps(dev):
    y = np.array([0.1, 0.9, NAN, 0.5, NAN, INF, 0.2, 0.8, -INF, NAN, 0.4], dtype=np.float32)
    s = dict(y=y, color=(255, 255, 255), alpha=255, width=1)
    run_series(dev, [s], (0, 10), seed=8)
    run_series(dev, [dict(s, marker="o", marker_size=5, width=2)], (0, 10), seed=8)
    lim = np.asarray(UNIT, dtype=np.float32)
    cov = R.series_coverage(s, RECT0, (0, 10), lim)
    px0, py0, pw, ph = RECT0
    cols = [c - px0 for c in R.columns(11, 0, 1, 0, 10, px0, pw)]
    rows = (R.rows_of(y, lim, py0, ph) - py0).tolist()
    assert cov[rows[3], cols[3]] and cov[:, cols[3]].sum() == 1      # the isolated finite sample paints its point, only that
    assert cov[rows[10], cols[10]] and cov[:, cols[10]].sum() == 1
    for a, b in ((1, 3), (3, 6), (7, 10)):                           # no segment crosses a gap
        assert not cov[:, cols[a] + 1:cols[b]].any(), (a, b)
    assert cov[:, cols[0]:cols[1] + 1].any(axis=0).all() and cov[:, cols[6]:cols[7] + 1].any(axis=0).all()
    run_series(dev, [dict(y=np.full(9, NAN, dtype=np.float32), width=3, marker="s", marker_size=5)], (0, 8), expect_empty=True)
    run_series(dev, [dict(y=np.array([INF, -INF], dtype=np.float32))], (0, 1), expect_empty=True)


def test_limits_record_edge_cases(dev):
    y = wave(40)
    for lim in ((0.3, 0.6), (5.0, 6.0), (-3e38, 3e38), (0.5, 0.5), (-3.4e38, 3.4e38)):            # clamped rows, lo == hi, an infinite span
        run_series(dev, [dict(y=y, width=1, marker="o", marker_size=1)], (0, 39), lim=lim, seed=3)
    run_series(dev, [dict(y=np.array([3e38, -3e38, 0], dtype=np.float32))], (0, 2), lim=R.limits([np.array([3e38, -3e38], dtype=np.float32)]))
    run_series(dev, [dict(y=y, x_first=1, x_step=10, marker="^", marker_size=5)], (0, 400), seed=5)   # the evaluation panels' abscissae
    run_series(dev, [dict(y=y[:4])] * 4, (0, 3))                                                    # four series in one launch


# --------------------------------------------------------------------------------------------------------------------- K4
def run_items(dev, font, items, H=40, W=50, row_pad=5, seed=0, expect_empty=False):
    from two_stage_object_detection_amd import hip_ops
    row = 3 * W + row_pad
    buf = np.random.default_rng(seed).integers(0, 256, size=(H, row), dtype=np.uint8)
    want = buf.copy()
    view = np.lib.stride_tricks.as_strided(want, shape=(H, W, 3), strides=(row, 3, 1))
    R.plot_items(view, items, font)
    assert np.array_equal(want, buf) == expect_empty
    on_dev = [dict(it, limits=torch.tensor(it["limits"], dtype=torch.float32, device=dev)) if it["kind"] == "number" else it
              for it in items]
    t = torch.from_numpy(buf.copy()).to(dev)
    hip_ops.plot_items(t.as_strided((H, W, 3), (row, 3, 1)), on_dev)
    got = t.cpu().numpy()
    diff = np.argwhere(got != want)
    assert diff.size == 0, f"{len(diff)} bytes differ, first at (y, byte) = {diff[0].tolist()}"
    return view


def test_rectangles_dashes_and_clipping(dev, font):
    items = [dict(kind="rect", x=3, y=4, w=20, h=10, color=(255, 0, 0)), dict(kind="rect", x=10, y=8, w=30, h=20, color=(0, 255, 0), alpha=128),
             dict(kind="rect", x=-5, y=-5, w=9, h=9, color=(0, 0, 255), alpha=77), dict(kind="rect", x=45, y=35, w=90, h=90, alpha=200),
             dict(kind="rect", x=25, y=0, w=2, h=40, color=(128, 128, 128), alpha=128, dash=(6, 4)),
             dict(kind="rect", x=30, y=3, w=1, h=33, dash=(5, 1)), dict(kind="rect", x=0, y=20, w=50, h=1, alpha=77)]
    run_items(dev, font, items)
    for k, it in enumerate(items):
        run_items(dev, font, [it], seed=k)
    # outside, empty, transparent: nothing is painted; an opaque full-image rectangle stores its colour everywhere
    run_items(dev, font, [dict(kind="rect", x=50, y=0, w=5, h=5), dict(kind="rect", x=0, y=-9, w=5, h=9), dict(kind="rect", x=1, y=1, w=0, h=5),
                          dict(kind="rect", x=1, y=1, w=5, h=5, alpha=0)], expect_empty=True)
    out = run_items(dev, font, [dict(kind="rect", x=0, y=0, w=50, h=40, color=(255, 255, 255))])
    assert (out == 255).all()
    run_items(dev, font, [], expect_empty=True)


def test_text_items(dev, font):
    items = [dict(kind="text", x=2, y=2, text="Loss 0.5:"), dict(kind="text", x=49, y=12, text="mAP", align="right", color=(200, 0, 0)),
             dict(kind="text", x=25, y=22, text="Epoch", align="center", scale=2, alpha=128), dict(kind="text", x=-4, y=34, text="clipped (a/b)_%"),
             dict(kind="text", x=40, y=-3, text="Top", scale=3), dict(kind="text", x=10, y=30, text="@~"), dict(kind="text", x=3, y=3, text="")]
    run_items(dev, font, items, H=44, W=63)
    for k, it in enumerate(items[:-1]):
        run_items(dev, font, [it], seed=k)
    run_items(dev, font, [dict(kind="text", x=0, y=0, text="x" * 32, color=(9, 9, 9))], H=9, W=200, row_pad=0)
    run_items(dev, font, [dict(kind="text", x=5, y=5, text="a", alpha=0), dict(kind="text", x=60, y=5, text="a")], expect_empty=True)


@pytest.mark.parametrize("lim", [(0.0, 1.0), (-0.0005, 12.3456), (-2e6, 2e6), (-3e38, 3e38), (-7.25, -1.5), (0.0, 999999.0)])
def test_device_formatted_tick_labels(dev, font, lim):
    T = 5
    strings = [R.format_number(lim, k, T) for k in range(T + 1)]
    if lim == (0.0, 1.0):
        assert strings == [b"0.000", b"0.200", b"0.400", b"0.600", b"0.800", b"1.000"]
    if lim == (-2e6, 2e6):
        assert strings[0] == strings[-1] == b"-.---" and b"-400000.000" in strings       # beyond the printable range at the ends only
    if lim == (-3e38, 3e38):
        assert set(strings) == {b"-.---"}
    items = [dict(kind="number", x=78, y=2 + 9 * k, limits=lim, tick=k, ticks=T, align="right", color=(0, 0, 120)) for k in range(T + 1)]
    items += [dict(kind="number", x=82, y=2 + 9 * k, limits=lim, tick=k, ticks=T, alpha=150) for k in range(T + 1)]
    items += [dict(kind="number", x=80, y=60, limits=lim, tick=2, ticks=T, align="center", scale=2), dict(kind="number", x=9, y=80, limits=lim, tick=1, ticks=0)]
    run_items(dev, font, items, H=90, W=160, row_pad=2)


def test_many_items_keep_their_order_across_chunks_and_tiles(dev, font):
    rng = np.random.default_rng(21)
    items = []
    for k in range(600):                                             # more than two reads of 256 items, over many 64 x 4 tiles
        kind = ("rect", "text", "number")[k % 3]
        it = dict(kind=kind, x=int(rng.integers(-10, 140)), y=int(rng.integers(-10, 70)), color=tuple(int(v) for v in rng.integers(0, 256, 3)),
                  alpha=int(rng.integers(1, 256)))
        if kind == "rect":
            it.update(w=int(rng.integers(1, 40)), h=int(rng.integers(1, 30)), dash=(int(rng.integers(0, 7)), int(rng.integers(0, 5))))
        elif kind == "text":
            it.update(text="".join(chr(int(c)) for c in rng.integers(32, 127, int(rng.integers(0, 9)))), scale=int(rng.integers(1, 3)),
                      align=("left", "right", "center")[int(rng.integers(0, 3))])
        else:
            it.update(limits=(float(rng.standard_normal()), float(rng.standard_normal() * 50 + 60)), tick=int(rng.integers(0, 6)), ticks=5,
                      align=("left", "right", "center")[int(rng.integers(0, 3))])
        items.append(it)
    run_items(dev, font, items, H=67, W=131, row_pad=3)
    run_items(dev, font, items[:257], H=4, W=64, row_pad=0)


# ------------------------------------------------------------------------------------------------------------- the figure
def curves(n_train, n_eval, seed=0):
    rng = np.random.default_rng(seed)
    train = (2.0 * np.exp(-np.arange(n_train) / max(n_train / 3, 1)) + 0.3 + 0.2 * rng.standard_normal(n_train)).astype(np.float32)
    ev = (1.5 * np.exp(-np.arange(n_eval) / 2.0) + 0.5).astype(np.float32)
    data = dict(train_loss=train, ema_train_loss=R.ema(train, 0.01) if n_train else train, eval_loss=ev,
                ema_eval_loss=R.ema(ev, 0.01) if n_eval else ev, mAP50_list=np.linspace(0.1, 0.7, n_eval, dtype=np.float32),
                mAP50_95_list=np.linspace(0.05, 0.45, n_eval, dtype=np.float32), mAP95_list=np.linspace(0.0, 0.12, n_eval, dtype=np.float32))
    return data


def figure_args(data, dev):
    from two_stage_object_detection_amd.utils import draw
    return [torch.from_numpy(data[key]).to(dev) for panel in draw.SERIES for key, *_ in panel]


@pytest.mark.parametrize("size,n_train,n_eval,epochs", [((244, 200), 120, 3, 4), ((300, 240), 1000, 4, 31), ((300, 240), 57, 0, 3),
                                                         ((330, 260), 1, 1, 1)])
def test_figure_equals_the_restatement_composed_the_same_way(dev, font, size, n_train, n_eval, epochs):
    from two_stage_object_detection_amd.utils import draw
    if size == (244, 200):
        assert size == draw.MIN_SIZE
    data = curves(n_train, n_eval)
    got = draw.plot_training_metrics(epochs, n_train, *figure_args(data, dev), size=size)
    assert got.shape == (*size, 3) and got.dtype == torch.uint8 and got.is_cuda
    plan = draw.figure_plan(epochs, n_train, {k: len(v) for k, v in data.items()}, size)
    want = R.figure(plan, data, font)
    got = got.cpu().numpy()
    diff = np.argwhere((got != want).any(axis=-1))
    assert diff.size == 0, f"{len(diff)} pixels differ, first at (y, x) = {diff[0].tolist()}"
    assert (want == 255).all(axis=-1).mean() > 0.5 and len(np.unique(want.reshape(-1, 3), axis=0)) > 8     # white paper, many inks
    if n_eval == 0:                                                  # frame, grid and text only in panels 2 and 3
        for p in plan["panels"][1:]:
            px0, py0, pw, ph = p["rect"]
            inner = want[py0:py0 + ph, px0:px0 + pw]
            assert (inner[..., 0] == inner[..., 1]).all() and (inner[..., 1] == inner[..., 2]).all()         # grays only


def test_figure_input_forms_out_and_path(dev, tmp_path):
    from two_stage_object_detection_amd.utils import draw
    from two_stage_object_detection_amd.utils.utils import TrainingLog
    data = curves(90, 3, seed=2)
    tensors = figure_args(data, dev)
    base = draw.plot_training_metrics(3, 90, *tensors, size=(300, 240))
    log = TrainingLog(dev, capacity=16)
    for v in tensors[0]:
        log.append(v)
    as_log = draw.plot_training_metrics(3, list(range(90)), log, log.ema(0.01), *tensors[2:], size=(300, 240))
    assert torch.equal(as_log, base)                                 # (log.ema is the restated EMA, bit for bit)
    as_lists = draw.plot_training_metrics(3, 90, *[list(t) for t in tensors], size=(300, 240))       # lists of 0-d device tensors
    assert torch.equal(as_lists, base)
    as_floats = draw.plot_training_metrics(3, 90, *tensors[:4], *[[float(v) for v in data[k]] for k in ("mAP50_list", "mAP50_95_list", "mAP95_list")],
                                           size=(300, 240), device=dev)
    assert torch.equal(as_floats, base)
    out = torch.full((300, 240, 3), 9, dtype=torch.uint8, device=dev)
    assert draw.plot_training_metrics(3, 90, *tensors, out=out, path=tmp_path / "training_metrics.png") is out and torch.equal(out, base)
    blob = open(tmp_path / "training_metrics.png", "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n" and blob[12:16] == b"IHDR" and blob[16:24] == (240).to_bytes(4, "big") + (300).to_bytes(4, "big")
    pitched = torch.zeros((300, 250, 3), dtype=torch.uint8, device=dev)
    draw.plot_training_metrics(3, 90, *tensors, out=pitched[:, :240])
    assert torch.equal(pitched[:, :240], base) and not bool(pitched[:, 240:].any())


def test_figure_makes_no_host_read(dev):
    """With device-resident inputs the whole figure runs under torch's sync debug mode "error": no device-to-host copy and no
    blocking copy anywhere in the call."""
    from two_stage_object_detection_amd.utils import draw
    from two_stage_object_detection_amd.utils.utils import TrainingLog
    data = curves(300, 3, seed=4)
    tensors = figure_args(data, dev)
    log = TrainingLog(dev, capacity=8)
    want = draw.plot_training_metrics(5, 300, *tensors, size=(300, 240))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for v in tensors[0]:
            log.append(v)
        got = draw.plot_training_metrics(5, 300, log, log.ema(0.01), *tensors[2:], size=(300, 240))
        with pytest.raises(RuntimeError):                            # the mode is live on this build: a host read is refused
            tensors[0][0].item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, want)
