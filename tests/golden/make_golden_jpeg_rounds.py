"""Writes tests/golden/jpeg_rounds.npz: four small JPEG files of seeded noise without restart markers whose entropy-coded segments
are exactly 256, 257, 512 and 513 one-word subsequences long - the round boundaries of the device Huffman pass (DESIGN.md
section 4.29): a last round that is full, and a last round of one lane that starts from the carried state.  At two words per
subsequence the last two are 256 and 257 again.  Needs Pillow (libjpeg-turbo).  The seeds below were found with Pillow 12.2;
every count is checked with tests/jpeg_scan_restated.py, and a seed that misses it with another encoder is replaced by the
first one from 0 upwards that hits it.  Never run by a test.
Usage: python tests/golden/make_golden_jpeg_rounds.py

Keys: `names` (one string per case), `subseqs` (int32, one-word subsequences per case), `file_<i>` (u8, the file), `pixels_<i>`
(u8 [H,W,3], Pillow's decode)."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
# (seed, H, W, quality, Pillow subsampling, one-word subsequences)
CASES = [(20, 48, 31, 79, 2, 256), (7, 37, 43, 67, 2, 257), (17, 65, 24, 95, 2, 512), (25, 28, 55, 71, 0, 513)]


def encode(S, seed, H, W, quality, sub):
    """(file bytes, one-word subsequences of its one segment)"""
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=sub)
    records = S.scan(buf.getvalue())[2]
    assert len(records) == 1, "no restart markers"
    return buf.getvalue(), -(-records[0][3] // 32)


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import jpeg_scan_restated as S
    out, names = {}, []
    for seed, H, W, quality, sub, subseqs in CASES:
        data, got = encode(S, seed, H, W, quality, sub)
        if got != subseqs:
            seed = next(k for k in range(100000) if encode(S, k, H, W, quality, sub)[1] == subseqs)
            data, got = encode(S, seed, H, W, quality, sub)
        assert got == subseqs
        name = f"{H}x{W}_s{sub}_q{quality}_{subseqs}"
        out[f"file_{len(names)}"] = np.frombuffer(data, dtype=np.uint8)
        out[f"pixels_{len(names)}"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        names.append(name)
        print(name, "seed", seed, len(data), "bytes")
    out["names"] = np.array(names)
    out["subseqs"] = np.array([c[5] for c in CASES], dtype=np.int32)
    path = os.path.join(HERE, "jpeg_rounds.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
