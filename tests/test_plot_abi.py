"""Training curves without a device: the EMA restatement and ``update_ema`` against the reference's
recorded values; header, binding and library agree; the struct layouts against the C compiler's; every refusal of the four
calls (on the host, before any launch); ``save_png`` read back by a reader written out here; the figure's host layout."""
import ctypes
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plot_restated as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from two_stage_object_detection_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi, _ffi.lib()


def _status(L, rc):
    return L.tsod_status_str(rc).decode().upper() if rc else "OK"


# ------------------------------------------------------------------------------------------------------------------- EMA
def test_restated_ema_equals_the_reference_bit_for_bit(golden_dir):
    z = np.load(os.path.join(golden_dir, "ema_ref.npz"))
    assert z["x"].dtype == np.float32 and z["x"].shape == (1000,) and list(z["alphas"]) == [0.01, 0.3]
    for k, alpha in enumerate(z["alphas"]):
        got = R.ema(z["x"], float(alpha))
        assert np.array_equal(got.view(np.uint32), z[f"ema_{k}"].view(np.uint32)), alpha
    # an FMA-contracted chain is a different function: the recorded values tell the two apart
    a, b = R.ema_constants(0.01)
    fused, prev = np.empty(1000, dtype=np.float32), np.float32(0)
    for i, v in enumerate(z["x"]):
        prev = v if i == 0 else np.float32(float(a) * float(v) + float(np.float32(b * prev)))
        fused[i] = prev
    assert not np.array_equal(fused, z["ema_0"])


def test_update_ema_equals_the_reference(golden_dir):
    from two_stage_object_detection_amd.utils.utils import update_ema
    z = np.load(os.path.join(golden_dir, "ema_ref.npz"))
    assert update_ema(2.0, 0.5) == 2.0 and update_ema(2.0, 0.5, 4.0) == 3.0 and update_ema(1.0, 0.25, last_ema=5.0) == 4.0
    train_loss = [v for v in torch.from_numpy(z["x"])]               # 0-d f32 tensors, as the reference's script holds them
    for k, alpha in enumerate(z["alphas"]):
        ema = []
        for i, v in enumerate(train_loss):
            ema.append(v if i == 0 else update_ema(v, float(alpha), ema[i - 1]))
        assert torch.equal(torch.stack(ema), torch.from_numpy(z[f"ema_{k}"])), alpha


def test_training_log_on_the_host_keeps_every_value_across_growth():
    from two_stage_object_detection_amd.utils.utils import TrainingLog
    log = TrainingLog("cpu", capacity=2)
    vals = [0.5, 1.25, -3.0, 7.0, 2.0]
    for i, v in enumerate(vals):
        log.append(torch.tensor(v) if i % 2 else v)
        assert len(log) == i + 1
    assert log.capacity == 8 and log.values.tolist() == vals and log.values.dtype == torch.float32
    with pytest.raises(ValueError):
        log.append(torch.zeros(2))
    with pytest.raises(ValueError):
        TrainingLog("cpu", capacity=0)


# ------------------------------------------------------------------------------------------------- header, binding, library
CALLS = (("tsod_ema_scan_f32", 9), ("tsod_plot_limits_f32", 7), ("tsod_plot_series_u8", 14), ("tsod_plot_items_u8", 7))


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    raw_text = open(os.path.join(ROOT, "include", "tsod.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in CALLS:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name) and name in _ffi.EXPORTED_SYMBOLS, name
    for macro in ("MAX_SERIES", "MAX_WIDTH", "MAX_HEIGHT", "BLOCK_COLUMNS", "STRING_BYTES", "LIMITS_WORKSPACE_BYTES"):
        assert int(re.search(r"#define TSOD_PLOT_" + macro + r" (\d+)", raw_text).group(1)) == getattr(_ffi, "PLOT_" + macro), macro
    for name in ("MARKER_NONE", "MARKER_CIRCLE", "MARKER_SQUARE", "MARKER_TRIANGLE", "ITEM_RECT", "ITEM_TEXT", "ITEM_NUMBER"):
        assert int(re.search(r"TSOD_PLOT_" + name + r" = (\d)", raw_text).group(1)) == getattr(_ffi, "PLOT_" + name), name
    assert L.tsod_version() == 242                                   # the change only adds exports
    makefile = open(os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "Makefile")).read()
    assert "plot.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    # the font is shared with the overlay, not copied
    csrc = os.path.join(ROOT, "two_stage_object_detection_amd", "csrc")
    plot = open(os.path.join(csrc, "plot.hip")).read()
    assert '#include "font5x7.h"' in plot and "0b0" not in plot


@pytest.mark.parametrize("struct_name,mirror", [("tsod_plot_series", "PlotSeries"), ("tsod_plot_item", "PlotItem")])
def test_struct_layouts_match_header(tmp_path, struct_name, mirror):
    _ffi, _ = _lib()
    G = getattr(_ffi, mirror)
    names = [f[0] for f in G._fields_]
    fmt = " ".join(["%zu"] * (len(names) + 1))
    args = ", ".join([f"sizeof({struct_name})"] + [f"offsetof({struct_name}, {n})" for n in names])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsod.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(G)] + [getattr(G, n).offset for n in names]
    header = re.search(r"typedef struct " + struct_name + r" \{(.*?)\} " + struct_name + ";",
                       open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S).group(1)
    declared = re.findall(r"\**(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert declared == names


# ------------------------------------------------------------------------------------------------------------ the refusals
A = 0x10000


def test_ema_scan_argument_errors():
    _, L = _lib()
    call = lambda x=A, rows=2, n=10, xp=12, out=A + 0x1000, op=10: _status(L, L.tsod_ema_scan_f32(x, rows, n, xp, 0.5, 0.5, out, op, None))
    for kw in (dict(rows=-1), dict(n=-1), dict(x=None), dict(out=None), dict(xp=9), dict(op=9)):
        assert "INVALID" in call(**kw), kw
    for kw in (dict(rows=0), dict(n=0), dict(rows=0, x=None, out=None), dict(n=0, x=None, out=None, xp=0, op=0)):
        assert call(**kw) == "OK", kw                                # empty work: nothing is launched, so this needs no device


def test_plot_limits_argument_errors():
    _ffi, L = _lib()
    WS = _ffi.PLOT_LIMITS_WORKSPACE_BYTES

    def call(pointers=(A, A), lengths=(5, 0), n=None, limits=A + 0x100, ws=A + 0x1000, ws_bytes=WS, arrays=True):
        k = max(len(pointers), 1)
        ps, ls = (ctypes.c_void_p * k)(*pointers), (ctypes.c_int64 * k)(*lengths)
        return _status(L, L.tsod_plot_limits_f32(ps if arrays else None, ls if arrays else None, len(pointers) if n is None else n,
                                                 limits, ws, ws_bytes, None))

    for kw in (dict(limits=None), dict(n=-1), dict(n=5, pointers=(A,) * 5, lengths=(1,) * 5), dict(arrays=False),
               dict(lengths=(5, -1)), dict(pointers=(None, A), lengths=(5, 0))):
        assert "INVALID" in call(**kw), kw
    assert "WORKSPACE" in call(ws=None) and "WORKSPACE" in call(ws_bytes=WS - 1)
    assert "ALIGN" in call(ws=A + 0x1002)


def test_plot_series_argument_errors():
    _ffi, L = _lib()

    def call(image=A, H=50, W=40, row=None, rect=(5, 8, 32, 37), n_series=1, x=(0, 99), limits=A + 0x100, series=True, **kw):
        s = dict(y=A + 0x1000, n=100, x_first=0, x_step=1, width=1, marker=0, marker_size=1)
        s.update(kw)
        arr = (_ffi.PlotSeries * 5)()
        for rec in arr:
            for k, v in s.items():
                setattr(rec, k, v)
            rec.color = (ctypes.c_uint8 * 4)(1, 2, 3, 255)
        return _status(L, L.tsod_plot_series_u8(image, H, W, 3 * W if row is None else row, *rect, arr if series else None,
                                                n_series, x[0], x[1], limits, None))

    # null pointers, sizes, the pitch, the rectangle
    assert call(n=0) == "OK"                                         # the defaults are a valid call (with nothing to draw)
    for kw in (dict(image=None), dict(limits=None), dict(H=0), dict(W=-1), dict(row=119), dict(rect=(5, 8, 0, 37)),
               dict(rect=(5, 8, 32, -1)), dict(rect=(-1, 8, 32, 37)), dict(rect=(5, -1, 32, 37)), dict(rect=(9, 8, 32, 37)),
               dict(rect=(5, 14, 32, 37)), dict(x=(5, 4))):
        assert "INVALID" in call(**kw), kw
    assert "INVALID" in call(n_series=5) and "INVALID" in call(n_series=-1) and "INVALID" in call(series=False)
    # the series: counts, abscissae, width, marker and marker size
    for kw in (dict(n=-1), dict(y=None), dict(x_step=0), dict(x_first=-1), dict(n=101), dict(x_step=2), dict(width=-1), dict(width=16),
               dict(marker=4), dict(marker=-1), dict(marker_size=0), dict(marker_size=17), dict(marker_size=4), dict(marker=1, marker_size=2)):
        assert "INVALID" in call(**kw), kw
    # beyond 32-bit geometry, and a rectangle taller than the LDS bitmask
    assert "UNSUPPORTED" in call(H=1 << 16, W=1 << 15, rect=(0, 0, 8, 8))
    assert "UNSUPPORTED" in call(H=5000, rect=(5, 8, 32, _ffi.PLOT_MAX_HEIGHT + 1))
    assert "UNSUPPORTED" in call(x=(0, 1 << 31)) and "UNSUPPORTED" in call(x=(-(1 << 31), 99))
    # empty work: nothing is launched
    assert call(n_series=0) == "OK" and call(n_series=0, series=False) == "OK" and call(n=0) == "OK" and call(n=0, y=None) == "OK"


def test_plot_items_argument_errors():
    _, L = _lib()
    call = lambda image=A, H=40, W=50, row=150, items=A + 0x1000, n=3: _status(L, L.tsod_plot_items_u8(image, H, W, row, items, n, None))
    for kw in (dict(image=None), dict(H=0), dict(W=0), dict(row=149), dict(n=-1), dict(items=None)):
        assert "INVALID" in call(**kw), kw
    assert "UNSUPPORTED" in call(H=1 << 16, W=1 << 15, row=3 << 15)
    assert "ALIGN" in call(items=A + 0x1004)
    assert call(n=0) == "OK" and call(n=0, items=None) == "OK"


def test_wrappers_refuse_host_tensors_and_bad_items():
    from two_stage_object_detection_amd import _ffi, hip_ops
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_ffi.TsodError, match="HIP-only"):
        hip_ops.ema_scan(torch.zeros(4), 0.5)
    with pytest.raises(_ffi.TsodError, match="HIP-only"):
        hip_ops.plot_items(img, [])
    with pytest.raises(_ffi.TsodError, match="HIP-only"):
        hip_ops.plot_series(img, (0, 0, 8, 8), [], (0, 1), torch.zeros(2))
    with pytest.raises(_ffi.TsodError, match="HIP-only"):
        hip_ops.plot_limits([torch.zeros(4)])
    with pytest.raises(ValueError):
        hip_ops.pack_plot_items([dict(kind="circle", x=0, y=0)])
    with pytest.raises(ValueError, match="32"):
        hip_ops.pack_plot_items([dict(kind="text", x=0, y=0, text="x" * 33)])
    with pytest.raises(ValueError):
        hip_ops.pack_plot_items([dict(kind="rect", x=0, y=0, w=1, h=1, color=(0, 0, 256))])
    packed = hip_ops.pack_plot_items([dict(kind="rect", x=1, y=2, w=3, h=4, dash=(6, 4), alpha=9),
                                      dict(kind="text", x=-5, y=7, text="Ab", scale=2, align="center", color=(1, 2, 3))])
    assert packed.shape == (2, ctypes.sizeof(_ffi.PlotItem)) and packed.dtype == torch.uint8
    recs = (_ffi.PlotItem * 2).from_buffer_copy(packed.numpy().tobytes())
    assert (recs[0].kind, recs[0].x, recs[0].y, recs[0].w, recs[0].h, recs[0].dash_period, recs[0].dash_on, recs[0].color[3]) == \
        (_ffi.PLOT_ITEM_RECT, 1, 2, 3, 4, 6, 4, 9)
    assert (recs[1].kind, recs[1].x, recs[1].scale, recs[1].align, recs[1].len, bytes(recs[1].text[:2]), list(recs[1].color)) == \
        (_ffi.PLOT_ITEM_TEXT, -5, 2, 2, 2, b"Ab", [1, 2, 3, 255])


# ----------------------------------------------------------------------------------------------------- the restated rules
def test_restated_segment_rule_properties():
    """The four properties the header promises of the segment rule, on seeded segments and written-out cases."""
    rng = np.random.default_rng(7)
    for _ in range(2000):
        c0, r0, r1 = int(rng.integers(0, 50)), int(rng.integers(0, 60)), int(rng.integers(0, 60))
        c1 = c0 + int(rng.integers(0, 40))
        spans = [R.segment_rows(c0, r0, c1, r1, c) for c in range(c0, c1 + 1)]
        assert spans[0][0] <= r0 <= spans[0][1] and spans[-1][0] <= r1 <= spans[-1][1]              # both endpoints
        assert all(min(r0, r1) <= a <= b <= max(r0, r1) for a, b in spans)                          # inside the rows' span
        assert all(max(p[0], q[0]) <= min(p[1], q[1]) for p, q in zip(spans, spans[1:]))            # neighbours share a row
        if r0 == r1:
            assert all(s == (r0, r0) for s in spans)                                                # horizontal: one row
    assert [R.segment_rows(0, 0, 4, 4, c) for c in range(5)] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 4)]
    assert [R.segment_rows(0, 9, 2, 0, c) for c in range(3)] == [(7, 9), (2, 7), (0, 2)]
    assert R.segment_rows(3, 8, 3, 2, 3) == (2, 8)


def test_restated_small_cases():
    lim = np.array([0, 1], dtype=np.float32)
    assert R.columns(5, 0, 1, 0, 4, 10, 9) == [10, 12, 14, 16, 18] and R.columns(3, 1, 10, 0, 30, 0, 31) == [1, 11, 21]
    assert R.columns(2, 7, 1, 7, 7, 3, 9) == [3, 3]                  # x_hi == x_lo: the first column
    assert R.rows_of([0, 1, 0.5, -9, 9, 0.25], lim, 100, 5).tolist() == [104, 100, 102, 104, 100, 103]
    assert R.rows_of([3.0], np.array([3, 3], dtype=np.float32), 0, 5).tolist() == [4]          # lo == hi: a NaN product, the bottom row
    assert sorted(R.marker_pixels(1, 1)) == [(0, 0)] and len(R.marker_pixels(2, 5)) == 25
    assert len(R.marker_pixels(1, 5)) == 21 and (2, 2) not in R.marker_pixels(1, 5)            # a disc: the square less its corners
    assert sorted(R.marker_pixels(3, 3)) == [(-1, 1), (0, -1), (0, 0), (0, 1), (1, 1)]         # apex up
    assert R.limits([[1, 3], [np.nan, np.inf, 2]]).tolist() == [np.float32(1) - np.float32(0.1), np.float32(3) + np.float32(0.1)]
    assert R.limits([]).tolist() == [0, 1] and R.limits([[np.nan]]).tolist() == [0, 1] and R.limits([[2, 2]]).tolist() == [1.5, 2.5]
    big = R.limits([[-3e38, 3e38]])
    assert np.isfinite(big).all() and big[0] < np.float32(-3e38) and big[1] > np.float32(3e38)
    assert R.format_number((0, 1), 3, 5) == b"0.600" and R.format_number((0, 1), 5, 5) == b"1.000"
    assert R.format_number((-0.0005, 12.3456), 0, 5) == b"0.000" and R.format_number((-0.0005, 12.3456), 5, 5) == b"12.346"
    assert R.format_number((-2.5, 0), 0, 5) == b"-2.500" and R.format_number((-999999.9, 0), 0, 1) == b"-999999.872"       # (the f32 product is a multiple of 64 here)
    assert R.format_number((-2e6, 2e6), 0, 4) == b"-.---" and R.format_number((-3e38, 3e38), 1, 5) == b"-.---"
    assert R.format_number((np.nan, 1), 0, 5) == b"-.---"
    # a two-point line of width 1 in a 4 x 4 rectangle, blended once at alpha 128
    img = np.full((6, 6, 3), 100, dtype=np.uint8)
    n = R.plot_series(img, (1, 1, 4, 4), [dict(y=np.array([0, 1], dtype=np.float32), color=(200, 200, 200), alpha=128)], (0, 1), lim)
    want = np.zeros((6, 6), dtype=bool)
    want[4, 1] = want[3, 2] = want[4, 2] = want[2, 3] = want[3, 3] = want[1, 4] = want[2, 4] = True
    assert n == 7 and np.array_equal(img[..., 0] == 150, want) and np.array_equal(img[..., 0] == 100, ~want)


# --------------------------------------------------------------------------------------------------------------- save_png
def _read_png(path):
    """A PNG reader for what save_png writes: signature, chunk CRCs, IHDR, filter-0 rows -> u8 [H, W, 3]."""
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(blob):
        (n,), tag = struct.unpack(">I", blob[at:at + 4]), blob[at + 4:at + 8]
        body = blob[at + 8:at + 8 + n]
        assert struct.unpack(">I", blob[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff, tag
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == H * (1 + 3 * W)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert not rows[:, 0].any()                                      # filter type 0 on every row
    return rows[:, 1:].reshape(H, W, 3)


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7)])
def test_save_png_round_trip(tmp_path, H, W):
    from two_stage_object_detection_amd.utils.draw import save_png
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H * W))
    save_png(img, tmp_path / "a.png")
    assert np.array_equal(_read_png(tmp_path / "a.png"), img.numpy())
    wide = torch.randint(0, 256, (H, W + 3, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    save_png(wide[:, :W], tmp_path / "b.png")                        # a pitched view
    assert np.array_equal(_read_png(tmp_path / "b.png"), wide[:, :W].numpy())
    for bad in (torch.zeros(H, W, 3), torch.zeros(H, W, dtype=torch.uint8), torch.zeros(0, W, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            save_png(bad, tmp_path / "c.png")


# ------------------------------------------------------------------------------------------------------------- the layout
def test_figure_layout_refusals_and_geometry():
    from two_stage_object_detection_amd.utils import draw
    empty = [[]] * 7
    with pytest.raises(ValueError, match="range"):
        draw.plot_training_metrics(2, [0, 1, 3], *empty)
    with pytest.raises(ValueError, match="range"):
        draw.plot_training_metrics(2, [1, 2, 3], *empty)
    mh, mw = draw.MIN_SIZE
    for size in ((mh - 1, mw), (mh, mw - 1), (10, 10)):
        with pytest.raises(ValueError, match=re.escape(str(draw.MIN_SIZE))):
            draw.plot_training_metrics(2, 10, *empty, size=size)
    with pytest.raises(ValueError):
        draw.figure_plan(0, 10, {})
    lengths = dict(train_loss=100, ema_train_loss=100, eval_loss=2, ema_eval_loss=2, mAP50_list=2, mAP50_95_list=2, mAP95_list=2)
    for size in (draw.MIN_SIZE, (300, 240), (1500, 1200)):
        plan = draw.figure_plan(4, 100, lengths, size)
        H, W = size
        assert [len(p["series"]) for p in plan["panels"]] == [2, 2, 3] and plan["panels"][2]["fixed_limits"] == (0.0, 1.0)
        for p in plan["panels"]:
            px0, py0, pw, ph = p["rect"]
            assert 0 < px0 and px0 + pw < W and 0 < py0 and py0 + ph < H and pw >= 100 and ph >= 40
        rects = [p["rect"] for p in plan["panels"]]
        assert all(a[1] + a[3] < b[1] for a, b in zip(rects, rects[1:]))                             # stacked, not overlapping
        for it in plan["background"] + plan["legends"]:                                             # nothing starts outside
            assert 0 <= it["x"] <= W and 0 <= it["y"] <= H, it
        texts = [it["text"] for it in plan["background"] + plan["legends"] if it["kind"] == "text"]
        for want in (draw.SUPTITLE, *draw.TITLES, "Epoch", "Loss", "mAP", "Train Loss", "EMA Train Loss", "Eval Loss", "EMA Eval Loss",
                     "mAP 0.5", "mAP 0.5:0.95", "mAP 0.95", "0", "3", "1", "11"):
            assert want in texts, want
        numbers = [it for it in plan["background"] if it["kind"] == "number"]
        assert len(numbers) == 3 * (draw.Y_TICKS + 1) and {it["panel"] for it in numbers} == {0, 1, 2}
        dashed = [it for it in plan["background"] if it.get("dash")]
        cols = [plan["panels"][0]["rect"][0] + (25 * i * (plan["panels"][0]["rect"][2] - 1)) // 99 for i in (1, 2, 3)]
        assert [it["x"] for it in dashed] == cols and all(it["color"] == draw.GRAY and it["alpha"] == 128 for it in dashed)
    # empty evaluation lists: frame, grid and text only - no series and no legend for panels 2 and 3
    plan = draw.figure_plan(4, 100, dict(train_loss=100, ema_train_loss=100), (300, 240))
    assert [len(p["series"]) for p in plan["panels"]] == [2, 0, 0]
    assert sum(it["kind"] == "text" for it in plan["legends"]) == 2
