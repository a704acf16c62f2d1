"""Writes tests/golden/jpeg_large.npz: two noise-textured JPEG files without restart markers whose entropy-coded segments are long
enough for the device Huffman pass to walk them in at least three rounds at the default subsequence
length - 256 lanes x 1024 bits = 32 KiB per round, so more than 64 KiB each.  One is 4:2:0, one 4:4:4.  File bytes only: the
tests compare with the host pass, and with Pillow where it is installed.  Needs Pillow (libjpeg-turbo) and the built library
(the host pass must accept both files); never run by a test.  Usage: python tests/golden/make_golden_jpeg_large.py

Keys: `names` (one string per case), `file_<i>` (u8, the file)."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROUND_BYTES = 256 * 1024 // 8
CASES = [("216x296_s2_noise", 216, 296, 2, 97), ("152x200_s0_noise", 152, 200, 0, 96)]


def texture(rng, H, W):
    """Smooth ramps under dense noise: long codes, few end-of-block shortcuts."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([96 + 0.4 * xx + 0.2 * yy, 160 - 0.3 * xx + 0.1 * yy, 128 + 0.2 * xx - 0.3 * yy], axis=2)
    img += rng.normal(0, 48, size=img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    sys.path.insert(0, ROOT)
    from two_stage_object_detection_amd import hip_ops
    rng = np.random.default_rng(20240923)
    out, names = {}, []
    for name, H, W, sub, quality in CASES:
        buf = io.BytesIO()
        Image.fromarray(texture(rng, H, W)).save(buf, "JPEG", quality=quality, subsampling=sub)
        data = buf.getvalue()
        status, info = hip_ops.jpeg_parse(data)
        assert status == 0 and info.restart_interval == 0 and (info.hmax, info.vmax) == ((2, 2) if sub == 2 else (1, 1)), name
        coef = np.zeros(info.coef_total, dtype=np.int16)
        assert hip_ops.jpeg_entropy_decode(data, coef) == 0, name    # the host pass accepts it
        scan = data.index(b"\xff\xda")
        assert 2 * ROUND_BYTES < len(data) - scan - 16 < 3 * ROUND_BYTES, (name, len(data) - scan)
        out[f"file_{len(names)}"] = np.frombuffer(data, dtype=np.uint8)
        names.append(name)
        print(name, len(data), "bytes")
    out["names"] = np.array(names)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_large.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
