"""The detection overlay without a device: header, binding and library agree; the group struct's layout
against the C compiler's; every refusal of tsod_draw_groups_u8 (on the host, before any launch); the font against bitmaps written
out here; utils.overlay's host logic (with the device checks and the launch stubbed out)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_restated as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from two_stage_object_detection_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi, _ffi.lib()


def _status(L, rc):
    return L.tsod_status_str(rc).decode().upper() if rc else "OK"


def test_exports_exist_in_header_binding_and_library():
    _ffi, L = _lib()
    raw_text = open(os.path.join(ROOT, "include", "tsod.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, n_args in (("tsod_draw_groups_u8", 11), ("tsod_draw_font5x7", 1)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(_ffi._SIGNATURES[name][1]), name
        assert hasattr(raw, name) and name in _ffi.EXPORTED_SYMBOLS, name
    for macro, value in (("TSOD_DRAW_MAX_GROUPS", _ffi.DRAW_MAX_GROUPS), ("TSOD_DRAW_LIST_CAPACITY", _ffi.DRAW_LIST_CAPACITY),
                         ("TSOD_DRAW_STRING_BYTES", _ffi.DRAW_STRING_BYTES), ("TSOD_DRAW_MAX_STYLE", _ffi.DRAW_MAX_STYLE)):
        assert int(re.search(r"#define " + macro + r" (\d+)", raw_text).group(1)) == value, macro
    tags = re.search(r"TSOD_DRAW_TAG_NONE = (\d), TSOD_DRAW_TAG_ABOVE = (\d), TSOD_DRAW_TAG_BELOW = (\d)", raw_text)
    assert tuple(int(v) for v in tags.groups()) == (_ffi.DRAW_TAG_NONE, _ffi.DRAW_TAG_ABOVE, _ffi.DRAW_TAG_BELOW)
    assert L.tsod_version() == 242                                   # the change only adds exports
    makefile = open(os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "Makefile")).read()
    assert "augment.hip draw.hip" in makefile


def test_group_layout_matches_header(tmp_path):
    """The ctypes mirror of tsod_draw_group against the C compiler's own layout of include/tsod.h: the size and every field."""
    _ffi, _ = _lib()
    G = _ffi.DrawGroup
    names = [f[0] for f in G._fields_]
    fmt = " ".join(["%zu"] * (len(names) + 1))
    args = ", ".join(["sizeof(tsod_draw_group)"] + [f"offsetof(tsod_draw_group, {n})" for n in names])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsod.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(G)] + [getattr(G, n).offset for n in names]
    header = re.search(r"typedef struct tsod_draw_group \{(.*?)\} tsod_draw_group;", open(os.path.join(ROOT, "include", "tsod.h")).read(),
                       flags=re.S).group(1)
    declared = re.findall(r"\**(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert declared == names                                         # no field of the header is missing from the mirror


def test_argument_errors():
    """Every refusal returns its code on the host, before any launch (the pointers are never dereferenced)."""
    _ffi, L = _lib()
    A = 0x10000

    def call(images=A, B=2, H=40, W=50, row=None, img=None, n_groups=None, strings=A + 0x4000, n_strings=3, groups=True, **kw):
        g = dict(boxes=A + 0x1000, R=5, pitch=6, thickness=2, font_scale=1, padding=2, tag=_ffi.DRAW_TAG_BELOW, score_line=1,
                 string_first=0, string_count=n_strings, sx=1.0, sy=1.0)
        g.update(kw)
        arr = (_ffi.DrawGroup * 5)()
        for rec in arr:
            for k, v in g.items():
                setattr(rec, k, v)
        row = 3 * W if row is None else row
        img = H * row if img is None else img
        return _status(L, L.tsod_draw_groups_u8(images, B, H, W, row, img, arr if groups else None,
                                                1 if n_groups is None else n_groups, strings, n_strings, None))

    # null image, sizes, pitches
    for kw in (dict(images=None), dict(B=0), dict(H=0), dict(W=-3), dict(row=149), dict(img=40 * 150 - 1), dict(row=152, img=40 * 150)):
        assert "INVALID" in call(**kw), kw
    # more than four groups, a missing group array, a bad string table
    assert "INVALID" in call(n_groups=5) and "INVALID" in call(n_groups=-1) and "INVALID" in call(groups=False)
    assert "INVALID" in call(n_strings=-1, string_count=0) and "INVALID" in call(strings=None)
    assert "ALIGN" in call(strings=A + 0x4002)
    for kw in (dict(string_first=-1), dict(string_count=-1), dict(string_first=2, string_count=2)):
        assert "INVALID" in call(**kw), kw
    # the group: R, pitch, the row lists, the style
    for kw in (dict(R=-1), dict(boxes=None), dict(pitch=5), dict(pitch=0), dict(keep=A), dict(n_kept=A),
               dict(keep=A, n_kept=A, counts=A), dict(thickness=0), dict(font_scale=0), dict(padding=-1), dict(tag=3), dict(tag=-1),
               dict(score_line=2), dict(pitch=4, score_line=1)):
        assert "INVALID" in call(**kw), kw
    # beyond 32-bit geometry
    assert "UNSUPPORTED" in call(B=1, H=1 << 16, W=1 << 15, R=0)
    assert "UNSUPPORTED" in call(B=1 << 16, H=1, W=1, R=1 << 15)
    for kw in (dict(thickness=1 << 15), dict(font_scale=1 << 15), dict(padding=1 << 15)):
        assert "UNSUPPORTED" in call(**kw), kw
    # valid no-ops: no groups, R == 0 (nothing is launched, so this needs no device)
    assert call(n_groups=0) == "OK" and call(n_groups=0, groups=False) == "OK" and call(R=0) == "OK" and call(R=0, boxes=None) == "OK"
    assert call(n_groups=0, strings=None, n_strings=0) == "OK"
    assert "INVALID" in _status(L, L.tsod_draw_font5x7(None))


def _art(rows):
    return [int(r.replace(".", "0").replace("#", "1"), 2) for r in rows]


KNOWN_GLYPHS = {
    "A": [".###.", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"],
    "g": [".....", ".####", "#...#", "#...#", ".####", "....#", ".###."],
    "0": [".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."],
    ":": [".....", ".##..", ".##..", ".....", ".##..", ".##..", "....."],
    " ": ["....."] * 7,
    "~": ["#####"] * 7,                                              # no glyph of its own: the block
}


def test_font_table():
    from two_stage_object_detection_amd import hip_ops
    font = hip_ops.draw_font5x7()
    assert font.shape == (128, 7) and font.dtype == np.uint8
    assert int(font.max()) <= 0x1f                                   # only the 5 low bits
    for ch, rows in KNOWN_GLYPHS.items():
        assert list(font[ord(ch)]) == _art(rows), ch
    own = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz.:-_%()/"
    block = [0x1f] * 7
    for c in range(128):
        assert (list(font[c]) == block) == (chr(c) not in own), c
    shapes = {bytes(font[ord(ch)]) for ch in own}
    assert len(shapes) == len(own)                                   # no two characters share a shape
    # the header is the only place that holds the shapes
    csrc = os.path.join(ROOT, "two_stage_object_detection_amd", "csrc")
    assert len(re.findall(r"^TSOD_GLYPH\(", open(os.path.join(csrc, "font5x7.h")).read(), flags=re.M)) == len(own)


def test_restatement_small_cases():
    """The NumPy restatement on cases small enough to write the answer out."""
    from two_stage_object_detection_amd import hip_ops
    font = hip_ops.draw_font5x7()
    img = np.zeros((1, 5, 7, 3), dtype=np.uint8)
    g = dict(boxes=np.array([[[1, 1, 5, 3]]], dtype=np.float32), color=(10, 20, 30), alpha=255, width=1, tag="none")
    D.draw(img, [g], None, font)
    want = np.zeros((5, 7), dtype=bool)
    want[1, 1:6] = want[3, 1:6] = want[1:4, 1] = want[1:4, 5] = True
    assert np.array_equal(img[0, ..., 0] == 10, want) and np.array_equal(img[0, ..., 2] == 30, want)
    # blending rounds to nearest: (128 * 200 + 127 * 100 + 127) // 255 = 150
    img = np.full((1, 2, 2, 3), 100, dtype=np.uint8)
    D.draw(img, [dict(boxes=np.array([[[0, 0, 1, 1]]], dtype=np.float32), color=(200, 200, 200), alpha=128, width=1, tag="none")], None, font)
    assert int(img[0, 0, 0, 0]) == 150
    # ties go to even, products are clamped, a reversed or non-finite box draws nothing
    assert D.to_pixel(1.0, 0.5) == 0 and D.to_pixel(1.0, 1.5) == 2 and D.to_pixel(1.0, -2.5) == -2
    assert D.to_pixel(1.0, 1e30) == 2 ** 24 and D.to_pixel(2.0, -1e30) == -2 ** 24
    assert D.to_pixel(1.0, float("inf")) is None and D.to_pixel(float("inf"), 0.0) is None
    rec = dict(boxes=np.array([[[0, 0, 4, 4, 0.9995, 12]]], dtype=np.float32), score_line=True, label_offset=-13, strings=(0, 0))
    assert D.tag_lines(rec, 0, 0, None) == [b"class_-1", b"Conf: 1.000"]
    rec["boxes"][0, 0, 4] = np.nan
    assert D.tag_lines(rec, 0, 0, None)[1] == b"Conf: -.---"
    rec["boxes"][0, 0, 4] = 0.0004
    assert D.tag_lines(rec, 0, 0, None)[1] == b"Conf: 0.000"
    # a tag: 2 characters at scale 1, padding 1 -> 14 x 10 pixels above the box, flipped inside when it would leave the top
    strings = np.zeros((1, 32), dtype=np.uint8)
    strings[0, :2] = list(b"A:")
    img = np.zeros((1, 30, 30, 3), dtype=np.uint8)
    g = dict(boxes=np.array([[[3, 4, 20, 20]]], dtype=np.float32), labels=np.array([[0]]), color=(1, 1, 1), alpha=0, width=1,
             tag="above", text_color=(255, 0, 0), tag_bg=(9, 9, 9), tag_alpha=255, font_scale=1, padding=1, strings=(0, 1))
    D.draw(img, [g], strings, font)
    painted = img[0].any(axis=-1)
    assert painted[4:14, 3:17].all() and int(painted.sum()) == 140          # top = Y1 (4 - 10 < 0)
    glyph = (img[0, 5:12, 4:9, 0] == 255)
    assert np.array_equal(glyph, np.array([[c == "#" for c in r] for r in KNOWN_GLYPHS["A"]]))


@pytest.fixture()
def stub(monkeypatch):
    """utils.overlay on CPU tensors: the device checks pass and the launch records its arguments."""
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.utils import metrics, overlay
    calls = []
    monkeypatch.setattr(overlay, "require_cuda", lambda t, what: None)
    monkeypatch.setattr(metrics, "require_cuda", lambda t, what: None)
    monkeypatch.setattr(hip_ops, "draw_groups", lambda images, groups, strings=None: calls.append((images, groups, strings)) or images)
    monkeypatch.setattr(overlay, "_TABLES", {})
    return overlay, calls


def test_overlay_refuses_cpu_tensors():
    from two_stage_object_detection_amd import _ffi, hip_ops
    from two_stage_object_detection_amd.utils import overlay
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_ffi.TsodError, match="HIP-only"):
        overlay.draw_bounding_boxes(img, torch.zeros(1, 2, 4))
    with pytest.raises(_ffi.TsodError, match="HIP-only"):
        overlay.draw_detections(img, torch.zeros(1, 2, 6))
    with pytest.raises(_ffi.TsodError, match="HIP-only"):
        hip_ops.draw_groups(img, [])


def test_overlay_argument_conventions(stub):
    overlay, calls = stub
    img = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    boxes = torch.zeros(2, 5, 4)
    keep, n = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for kw in (dict(keep=keep), dict(n_kept=n), dict(keep=keep, n_kept=n, counts=n), dict(counts=torch.zeros(3, dtype=torch.int32)),
               dict(keep=keep[:, :4], n_kept=n), dict(labels=torch.zeros(2, 4, dtype=torch.int64)), dict(scores=torch.zeros(2, 4)),
               dict(tag="left")):
        with pytest.raises(ValueError):
            overlay.draw_bounding_boxes(img, boxes, **kw)
    for bad in (torch.zeros(2, 5, 5), torch.zeros(3, 5, 4), torch.zeros(5, 4)):
        with pytest.raises(ValueError):
            overlay.draw_bounding_boxes(img, bad)
    with pytest.raises(ValueError):
        overlay.draw_bounding_boxes(torch.zeros(2, 8, 8, 3), boxes)                      # not u8
    with pytest.raises(ValueError):
        overlay.draw_bounding_boxes(img, [boxes[0]], counts=n)                           # a list brings its own counts
    with pytest.raises(ValueError):
        overlay.draw_detections(img, torch.zeros(2, 5, 4))                               # records are six wide
    # a copy by default, `out` when given, in place with out=images; [H,W,3] is a batch of one
    calls.clear()
    got = overlay.draw_bounding_boxes(img, boxes)
    assert got is not img and calls[-1][0] is got
    out = torch.ones_like(img)
    assert overlay.draw_bounding_boxes(img, boxes, out=out) is out and not out.any()
    assert overlay.draw_bounding_boxes(img, boxes, out=img) is img
    one = overlay.draw_bounding_boxes(img[0], boxes[0], labels=torch.zeros(5, dtype=torch.int64))
    assert one.shape == (8, 8, 3) and calls[-1][0].shape == (1, 8, 8, 3) and calls[-1][1][0]["labels"].shape == (1, 5)
    # the group that reaches the launch
    calls.clear()
    overlay.draw_bounding_boxes(img, boxes, scores=torch.full((2, 5), 0.5), class_names=["a", "b"], prefix="P: ", label_offset=-1,
                                box_scale=(2.0, 3.0), color=(1, 2, 3), width=3, alpha=7, font_scale=2, keep=keep, n_kept=n,
                                labels=torch.ones(2, 5, dtype=torch.int64))
    _, (g,), strings = calls[-1]
    assert g["boxes"].shape == (2, 5, 6) and bool((g["boxes"][..., 4] == 0.5).all()) and g["score_line"] and g["strings"] == (0, 2)
    assert (g["scale"], g["color"], g["width"], g["alpha"], g["font_scale"], g["label_offset"], g["tag"]) == \
        ((2.0, 3.0), (1, 2, 3), 3, 7, 2, -1, "below")
    assert g["keep"] is not None and g["counts"] is None and bytes(strings[1].tolist()).rstrip(b"\0") == b"P: b"
    # scores without labels: the bare prefix as the only string
    overlay.draw_bounding_boxes(img, boxes, scores=torch.zeros(2, 5), prefix="Pred")
    _, (g,), strings = calls[-1]
    assert strings.shape == (1, 32) and g["strings"] == (0, 1) and g["labels"] is None and g["label_offset"] == 0
    # neither names nor a table: every label prints class_<n>
    overlay.draw_bounding_boxes(img, torch.zeros(2, 5, 6))
    assert calls[-1][2] is None and calls[-1][1][0]["strings"] == (0, 0)


def test_overlay_string_tables_and_padding(stub):
    overlay, calls = stub
    names = ["cat", "dog"]
    t = overlay.string_table(names, "GT: ", "cpu")
    assert overlay.string_table(tuple(names), "GT: ", "cpu") is t and overlay.string_table(names, "Pred: ", "cpu") is not t
    assert t.shape == (2, 32) and t.dtype == torch.uint8
    assert bytes(t[1].tolist()) == b"GT: dog" + b"\0" * 25
    assert overlay.string_table({0: "cat", 2: "emu"}, "", "cpu")[1].tolist()[:8] == list(b"class_1\0")
    assert overlay.encode_strings(["x" * 31]).shape == (1, 32) and int(overlay.encode_strings(["x" * 31])[0, 31]) == 0
    with pytest.raises(ValueError, match="31"):
        overlay.encode_strings(["x" * 32])
    with pytest.raises(ValueError, match="31"):
        overlay.string_table(["x" * 27], "Pred: ", "cpu")
    # draw_detections: one launch, ground truth first; one table with a window per group, cached
    img = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    det = [torch.rand(3, 6), torch.rand(1, 6)]
    gtb, gtl = [torch.rand(2, 4), torch.rand(4, 4)], [torch.tensor([0, 1]), torch.tensor([1, 1, 0, 0])]
    overlay.draw_detections(img, det, gtb, gtl, class_names=names, box_scale=(1.5, 2.0))
    assert len(calls) == 1
    _, (gt, pred), strings = calls[0]
    assert strings.shape == (4, 32) and gt["strings"] == (0, 2) and pred["strings"] == (2, 2)
    assert bytes(strings[3].tolist()).rstrip(b"\0") == b"Pred: dog" and bytes(strings[0].tolist()).rstrip(b"\0") == b"GT: cat"
    assert (gt["color"], gt["tag"], gt["score_line"], gt["width"]) == ((0, 128, 0), "above", False, 2)
    assert (pred["color"], pred["tag"], pred["score_line"], pred["width"]) == ((255, 0, 0), "below", True, 2)
    assert gt["tag_bg"] == pred["tag_bg"] == (255, 255, 255) and gt["tag_alpha"] == pred["tag_alpha"] == 204
    assert gt["scale"] == pred["scale"] == (1.5, 2.0)
    # lists are padded with zero rows to the longest (at least one row), the counts say how many are real
    assert pred["boxes"].shape == (2, 3, 6) and pred["counts"].tolist() == [3, 1] and not pred["boxes"][1, 1:].any()
    assert torch.equal(pred["boxes"][0], det[0]) and pred["keep"] is None
    assert gt["boxes"].shape == (2, 4, 4) and gt["counts"].tolist() == [2, 4] and gt["labels"][0].tolist() == [0, 1, -1, -1]
    overlay.draw_detections(img, [torch.zeros(0, 6), torch.zeros(0, 6)], class_names=names)
    assert calls[-1][1][0]["boxes"].shape == (2, 1, 6) and calls[-1][1][0]["counts"].tolist() == [0, 0]
    assert calls[-1][2] is strings                                  # the cached table
    # postprocess's triple passes straight through
    keep, n = torch.zeros(2, 5, dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
    overlay.draw_detections(img, torch.zeros(2, 5, 6), keep=keep, n_kept=n)
    (pred,) = calls[-1][1]
    assert pred["keep"].shape == (2, 5) and pred["n_kept"].tolist() == [1, 0] and pred["counts"] is None and calls[-1][2] is None
