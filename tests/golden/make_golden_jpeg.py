"""Writes tests/golden/jpeg_ref.npz: JPEG files encoded by Pillow and the pixels Pillow's Image.open(...).convert("RGB") decodes
from them - what the reference's dataset/dataloader.py:35 and multi_inference.py:65 hand to the transform.  Needs Pillow
(libjpeg-turbo); never run by a test.  Usage: python tests/golden/make_golden_jpeg.py

Keys: `names` (one string per case), `file_<i>` (u8, the file), `pixels_<i>` (u8 [H,W,3]); `progressive` and `cmyk` (u8, files
the decoder refuses - bytes only)."""
import io
import os

import numpy as np
from PIL import Image

SIZES = [(1, 1), (2, 3), (1, 9), (9, 1), (9, 2), (9, 4), (9, 5), (5, 7), (8, 8), (17, 9), (16, 16), (17, 33), (37, 53), (24, 130)]
SETTINGS = [("q12", dict(quality=12)), ("q75", dict(quality=75)), ("q100", dict(quality=100)),
            ("opt", dict(quality=60, optimize=True)), ("rstb", dict(quality=85, restart_marker_blocks=1)),
            ("rstr", dict(quality=40, restart_marker_rows=1))]
GREY = [((1, 1), 1), ((17, 9), 3), ((37, 53), 4)]


def picture(rng, H, W, channels=3):
    """Gradients, hard edges and noise: every kind of block a photograph has, saturated regions included."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.empty((H, W, channels), dtype=np.float64)
    for c in range(channels):
        a, b = rng.uniform(-3, 3, size=2)
        img[..., c] = 128 + 16 * (a * xx + b * yy)
    img[(xx // 5 + yy // 3) % 2 == 0] = rng.integers(0, 256, size=channels)        # hard-edged tiles of one saturated colour
    noisy = rng.random((H, W)) < 0.3
    img[noisy] += rng.normal(0, 60, size=(int(noisy.sum()), channels))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr if arr.shape[2] > 1 else arr[..., 0]).save(buf, "JPEG", **kw)
    return buf.getvalue()


def main():
    rng = np.random.default_rng(20240607)
    out, names = {}, []

    def add(name, data):
        i = len(names)
        names.append(name)
        out[f"file_{i}"] = np.frombuffer(data, dtype=np.uint8)
        out[f"pixels_{i}"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    for s, (H, W) in enumerate(SIZES):
        for sub in (0, 1, 2):
            for k in ((s + sub) % 6, (s + sub + 3) % 6):          # two of the six settings per (size, sampling), all six in turn
                tag, kw = SETTINGS[k]
                add(f"{H}x{W}_s{sub}_{tag}", encode(picture(rng, H, W), subsampling=sub, **kw))
    for (H, W), k in GREY:
        tag, kw = SETTINGS[k]
        add(f"{H}x{W}_grey_{tag}", encode(picture(rng, H, W, 1), **kw))
    out["names"] = np.array(names)
    out["progressive"] = np.frombuffer(encode(picture(rng, 17, 33), quality=75, progressive=True), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(picture(rng, 9, 5, 4), "CMYK").save(buf, "JPEG", quality=75)
    out["cmyk"] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_ref.npz")
    np.savez_compressed(path, **out)
    print(path, len(names), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
