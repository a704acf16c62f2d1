"""The reference's training transform (dataset/transform.py:4-12), CPU part: the drop-in import, the draw
order, hand-derived cases of every colour and box rule (checked on the float32 restatement and, for the colour ops, on the
library's own per-pixel arithmetic through its HOST entry point), the C ABI's argument checks and the kernels' metadata."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_transform_restated as R
from two_stage_object_detection_amd import _ffi, hip_ops
from two_stage_object_detection_amd._ffi import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
P = 0x10000          # a fake device pointer: validation must fail before it is ever dereferenced


def prm(**kw):
    """A draw record; the factors are f32 values, as ``torch.empty(1).uniform_(...).item()`` returns them."""
    base = dict(brightness=None, contrast=None, saturation=None, hue=None, contrast_before=True, perm=None, flip=False)
    base.update(kw)
    for k in ("brightness", "contrast", "saturation", "hue"):
        if base[k] is not None:
            base[k] = float(np.float32(base[k]))
    return base


def photo(p, white=1.0):
    return hip_ops.photometric(p["brightness"], p["contrast"], p["saturation"], p["hue"], p["contrast_before"], p["perm"],
                               white)


def both(pixels, p, white=1.0, mean=None):
    """(restatement, library host arithmetic) of the colour ops on [N,3] pixels; they must agree."""
    x = torch.tensor(pixels, dtype=torch.float32).reshape(-1, 3)
    ref = R.color(x.t().reshape(3, -1, 1), p, white, mean).reshape(3, -1).t()
    m = mean
    if m is None:
        m = R.contrast_mean(x.t().reshape(3, -1, 1), p, white).item() if p["contrast"] is not None else 0.0
    got = torch.from_numpy(hip_ops.augment_color_host(x.numpy(), photo(p, white), m))
    assert torch.allclose(got, ref, rtol=1e-6, atol=1e-6), (got, ref)
    return ref


# ------------------------------------------------------------------------------------------- the drop-in and the draws
def test_dropin_exposes_the_training_transform():
    code = ("import two_stage_object_detection_amd as p; p.install_dropin()\n"
            "from dataset.transform import transform, TrainTransform, eval_transform, EvalTransform\n"
            "assert isinstance(transform, TrainTransform) and transform.size == (600, 600)\n"
            "assert (transform.scale_range, transform.flip_p, transform.min_size) == ((0.8, 1.2), 0.5, 1.0)\n"
            "assert transform.photometric_white == 1.0 and isinstance(eval_transform, EvalTransform)\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_make_params_follows_the_draw_order():
    from two_stage_object_detection_amd.dataset.transform import TrainTransform
    seen = {k: set() for k in ("brightness", "contrast", "saturation", "hue", "perm", "flip", "contrast_before")}
    for seed in range(200):
        H, W = (480, 640) if seed % 2 else (1080, 1920)
        want = R.draw_sequence(H, W, torch.Generator().manual_seed(seed))
        got = TrainTransform(generator=torch.Generator().manual_seed(seed)).make_params(H, W)
        assert got.__dict__ == want, (seed, got, want)
        for k in seen:
            seen[k].add(want[k] is None if k in ("brightness", "contrast", "saturation", "hue", "perm") else want[k])
        lo = min(600 / H, 600 / W)
        assert int(H * lo * 0.8) - 1 <= got.size[0] <= int(H * lo * 1.2) + 1
    assert all(v == {True, False} for v in seen.values()), seen            # every branch taken


def test_make_params_uses_the_global_rng_by_default():
    from two_stage_object_detection_amd.dataset.transform import TrainTransform
    torch.manual_seed(7)
    a = TrainTransform().make_params(375, 500)
    want = R.draw_sequence(375, 500, torch.Generator().manual_seed(7))
    assert a.__dict__ == want


# ------------------------------------------------------------------------------------------- colour rules, by hand
def test_brightness_clamps_into_the_reference_range():
    out = both([[200.0, 100.0, 50.0], [0.5, 0.2, 0.0]], prm(brightness=1.1))
    assert out[0].tolist() == [1.0, 1.0, 1.0]
    assert out[1].tolist() == pytest.approx([0.55, 0.22, 0.0], abs=1e-7)


def test_contrast_blends_towards_the_mean():
    out = both([[0.2, 0.4, 0.6]], prm(contrast=0.5), mean=0.5)
    assert out[0].tolist() == pytest.approx([0.35, 0.45, 0.55], abs=1e-7)
    # the mean is the grayscale mean over the image: black and white pixels -> (0 + 0.9999) / 2
    img = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    assert torch.allclose(both(img, prm(contrast=0.5)), both(img, prm(contrast=0.5), mean=0.9999 / 2), rtol=0, atol=1e-7)
    # contrast after hue sees the hue-shifted image, before saturation it sees the brightness-scaled one
    a = both([[0.9, 0.1, 0.3], [0.2, 0.6, 0.4]], prm(contrast=1.3, saturation=0.6, contrast_before=True))
    b = both([[0.9, 0.1, 0.3], [0.2, 0.6, 0.4]], prm(contrast=1.3, saturation=0.6, contrast_before=False))
    assert not torch.equal(a, b)


def test_saturation_keeps_a_gray_pixel():
    # gray weights sum to 0.9999, so a gray pixel moves by at most (1 - f) * 1e-4 of its value
    out = both([[0.3, 0.3, 0.3]], prm(saturation=0.5))
    assert out[0].tolist() == pytest.approx([0.3] * 3, abs=2e-5)
    out = both([[0.8, 0.2, 0.2]], prm(saturation=0.0))
    g = 0.8 * 0.2989 + 0.2 * 0.587 + 0.2 * 0.114
    assert out[0].tolist() == pytest.approx([g] * 3, abs=1e-6)


def test_hue_sector_corners_and_gray():
    corners = [[1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 1, 1], [0, 0, 1], [1, 0, 1]]          # H = 0, 1/6, ..., 5/6
    out = both(corners, prm(hue=0.0))
    assert torch.allclose(out, torch.tensor(corners, dtype=torch.float32), atol=1e-6)
    out = both([[1, 0, 0]], prm(hue=1 / 3))                                               # red -> green
    assert torch.allclose(out, torch.tensor([[0.0, 1.0, 0.0]]), atol=1e-6)
    out = both([[1, 0.5, 0]], prm(hue=1 / 12))                                            # H 1/12 -> 1/6: yellow
    assert torch.allclose(out, torch.tensor([[1.0, 1.0, 0.0]]), atol=1e-6)
    out = both([[1, 0.5, 0]], prm(hue=-1 / 12))                                           # -> red
    assert torch.allclose(out, torch.tensor([[1.0, 0.0, 0.0]]), atol=1e-6)
    out = both([[0.4, 0.4, 0.4]], prm(hue=0.05))                                          # maxc == minc: unchanged
    assert torch.equal(out[0], torch.full((3,), 0.4))


def test_hue_keeps_v_above_one_in_reference_mode():
    # s = 0.75, H = 1/18: sector 0, (v, t, p) with t = 100 and p = 50 clamped to 1, v = 200 not clamped
    out = both([[200.0, 100.0, 50.0]], prm(hue=0.0))
    assert out[0].tolist() == [200.0, 1.0, 1.0]


def test_permutation():
    out = both([[1.0, 2.0, 3.0]], prm(perm=(2, 0, 1)))
    assert out[0].tolist() == [3.0, 1.0, 2.0]


def test_white_255_runs_the_ops_on_x_over_255():
    g = torch.Generator().manual_seed(3)
    px = torch.randint(0, 256, (64, 3), generator=g).float().numpy()
    for p in (prm(brightness=1.1), prm(contrast=0.7, contrast_before=False, hue=0.03), prm(saturation=1.4, perm=(1, 2, 0)),
              prm(brightness=0.9, contrast=1.2, saturation=0.6, hue=-0.04)):
        mean = float(R.gray(torch.from_numpy(px / np.float32(255)).t().float()).mean()) if p["contrast"] else 0.0
        lifted = both(px, p, white=255.0, mean=mean)
        scaled = both(px / np.float32(255), p, white=1.0, mean=mean)
        assert torch.equal(lifted, scaled * 255)
        assert lifted.max() > 1.5                                    # not clamped into [0, 1]


def test_every_op_combination_agrees_with_the_library():
    g = torch.Generator().manual_seed(4)
    px = torch.randint(0, 256, (200, 3), generator=g).float()
    px[:20] = px[:20, :1]                                            # gray pixels: maxc == minc
    for mask in range(16):
        for before in (True, False):
            for white in (1.0, 255.0):
                p = prm(brightness=1.07 if mask & 1 else None, contrast=0.62 if mask & 2 else None,
                        saturation=1.3 if mask & 4 else None, hue=-0.035 if mask & 8 else None, contrast_before=before,
                        perm=(1, 0, 2) if mask & 1 else None)
                both(px.numpy() if white == 255.0 else px.numpy() / 255.0, p, white)


# ------------------------------------------------------------------------------------------- box rules, by hand
def right_edge_case():
    """(W, new_w) where a box on the right edge lands past the canvas after the two f32 multiplications."""
    f32 = np.float32
    for W in range(300, 2000):
        for nw in range(int(W * 0.3), int(W * 1.5)):
            x = f32(f32(W) * f32(nw / W)) * f32(600 / nw)
            if x > f32(600):
                return W, nw, float(x)
    raise AssertionError("no right-edge case")


def test_flip_boxes():
    b, lab = R.boxes([[10.0, 5.0, 30.0, 20.0]], [4], 50, 100, prm(flip=True, size=(50, 100)), out_size=(50, 100))
    assert b.tolist() == [[70.0, 5.0, 90.0, 20.0]] and lab.tolist() == [4]


def test_right_edge_box_is_dropped_by_the_two_multiplications():
    W, nw, x = right_edge_case()
    assert x > 600.0
    box = [[W - 50.0, 10.0, float(W), 60.0]]
    b, lab = R.boxes(box, [1], 300, W, prm(size=(300, nw)), out_size=(600, 600))
    assert b.shape == (0, 4) and lab.shape == (0,)
    # one composed ratio would have kept it: the order of the multiplications decides
    assert np.float32(W) * np.float32(600 / W) <= 600.0
    b, _ = R.boxes([[W - 50.0, 10.0, float(W) - 1, 60.0]], [1], 300, W, prm(size=(300, nw)), out_size=(600, 600))
    assert b.shape == (1, 4)


def test_min_size_negative_and_label_order():
    box = [[0.0, 0.0, 10.0, 10.0],          # kept
           [5.0, 5.0, 5.9, 20.0],           # 0.9 wide: dies at min_size
           [-0.5, 0.0, 10.0, 10.0],         # negative coordinate
           [1.0, 1.0, 2.0, 2.0],            # exactly min_size: kept
           [2.0, 2.0, 30.0, 40.0],          # kept
           [0.0, 0.0, 10.0, 60.5]]          # past the bottom edge
    b, lab = R.boxes(box, [10, 11, 12, 13, 14, 15], 60, 30, prm(size=(60, 30)), out_size=(60, 30))
    assert lab.tolist() == [10, 13, 14]
    assert b.tolist() == [box[0], box[3], box[4]]


# ------------------------------------------------------------------------------------------- the C ABI
def test_augment_abi_validation():
    L = lib()
    good = photo(prm(contrast=0.8))
    none = photo(prm())
    bad_perm = photo(prm(perm=(0, 0, 1)))
    bad_white = photo(prm(brightness=1.0), white=0.0)
    bad_hue = photo(prm(hue=0.6))
    unknown = photo(prm())
    unknown.flags = 64
    g = L.tsod_augment_gray_mean_partials
    assert g(None, 8, 8, 24, good, P, None) == INVALID
    assert g(P, 0, 8, 24, good, P, None) == INVALID
    assert g(P, 8, 8, 23, good, P, None) == INVALID                          # row < 3W
    assert g(P, 8, 8, 24, none, P, None) == INVALID                          # no contrast drawn
    assert g(P, 8, 8, 24, good, None, None) == INVALID
    assert g(P, 8, 8, 24, None, P, None) == INVALID
    r = L.tsod_augment_resize_u8_f32
    args = lambda p, parts, flip, c_out: (P, 8, 8, 24, p, parts, flip, P, P, P, P, P, P, 4, 4, P, 16, 4, 1, c_out, None)
    assert r(*args(good, None, 0, 4)) == INVALID                             # contrast without its partials
    assert r(*args(none, None, 2, 4)) == INVALID                             # flip is 0 or 1
    assert r(*args(none, None, 0, 2)) == INVALID                             # C_out < 3
    for p in (bad_perm, bad_white, bad_hue, unknown):
        assert r(*args(p, None, 0, 4)) == INVALID
    f = L.tsod_resize_bilinear_aa_f32
    assert f(P, 8, 8, 5, 8, 1, 64, P, P, P, P, P, P, 4, 4, P, 16, 4, 1, 4, None) == INVALID          # C = 5
    assert f(P, 8, 8, 3, 8, 1, 64, P, P, P, P, P, P, 4, 4, P, 16, 4, 1, 2, None) == INVALID          # C_out < C
    assert f(P, 8, 8, 3, -8, 1, 64, P, P, P, P, P, P, 4, 4, P, 16, 4, 1, 4, None) == INVALID         # negative stride
    b = L.tsod_augment_boxes_f32
    assert b(P, P, 0, P, P, P, P, P, None) == INVALID
    assert b(P, P, 70000, P, P, P, P, P, None) == INVALID
    assert b(None, P, 1, P, P, P, P, P, None) == INVALID
    assert b(P, P, 1, P, P, P, P, None, None) == INVALID
    h = L.tsod_augment_color_host
    buf = (ctypes.c_float * 3)()
    assert h(ctypes.addressof(buf), -1, none, 0.0, ctypes.addressof(buf)) == INVALID
    assert h(ctypes.addressof(buf), 1, bad_perm, 0.0, ctypes.addressof(buf)) == INVALID
    assert h(ctypes.addressof(buf), 1, none, 0.0, ctypes.addressof(buf)) == 0
    with pytest.raises(_ffi.TsodError):
        hip_ops.augment_color_host(np.zeros((1, 3), np.float32), bad_hue)


def test_photometric_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsod.h"\nint main(void) { printf("%zu %zu %zu %zu %d %d %d '
                   '%d %d %d %d\\n", sizeof(tsod_photometric), offsetof(tsod_photometric, hue), offsetof(tsod_photometric, white), '
                   'offsetof(tsod_photometric, perm), TSOD_AUGMENT_MEAN_PARTS, TSOD_AUG_BRIGHTNESS, TSOD_AUG_CONTRAST, '
                   'TSOD_AUG_SATURATION, TSOD_AUG_HUE, TSOD_AUG_CONTRAST_FIRST, TSOD_AUG_PERMUTE); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = tuple(int(v) for v in subprocess.check_output([str(exe)]).split())
    S = _ffi.Photometric
    assert got == (ctypes.sizeof(S), S.hue.offset, S.white.offset, S.perm.offset, _ffi.AUG_MEAN_PARTS, _ffi.AUG_BRIGHTNESS,
                   _ffi.AUG_CONTRAST, _ffi.AUG_SATURATION, _ffi.AUG_HUE, _ffi.AUG_CONTRAST_FIRST, _ffi.AUG_PERMUTE)


def test_augment_kernels_use_no_scratch_memory(tmp_path):
    from test_kernel_metadata import _kernel_notes
    kernels = _kernel_notes(tmp_path)
    aug = {k: v for k, v in kernels.items() if any(s in k for s in ("gray_mean_kernel", "resize_tile_kernel",
                                                                    "resize_flat_kernel", "boxes_kernel"))}
    # the tiled and the flat resize, each over its three sources (u8 bytes, augmented u8, strided f32)
    assert len(aug) == 8, sorted(aug)
    assert sum(s in k for k in aug for s in ("U8Bytes", "AugU8", "StridedF32")) == 6, sorted(aug)
    bad = {k: v for k, v in aug.items() if v.get("private_segment_fixed_size", 0) != 0 or v.get("vgpr_spill_count", 0) != 0}
    assert not bad, bad
