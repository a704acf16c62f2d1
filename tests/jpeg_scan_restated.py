"""A NumPy restatement of what ``tsod_jpeg_scan_prepare`` writes (include/tsod.h): the entropy-coded bytes
of a file with FF 00 unstuffed and the restart markers removed, every restart interval on a 4-byte boundary; one record per
interval; the scan's code tables in the fixed device layout.  Built on tests/jpeg_restated.py's marker parser; none of it is code
under test.  Also the seeded single-byte corruptions of the entropy-coded segment that the CPU and the GPU tests share."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_restated as R  # noqa: E402


class BadRestart(Exception):
    pass


def scan(data):
    """(info, stream u8 ndarray, [(first_mcu, n_mcu, stream_offset, bit_length, flags)]) of one file."""
    data = bytes(data)
    info = R.parse(data)
    d = np.frombuffer(data, dtype=np.uint8)
    n_mcu = info["mcus_x"] * info["mcus_y"]
    interval = info["restart_interval"] or n_mcu
    ff = np.flatnonzero(d == 0xFF)
    nxt = np.where(ff + 1 < d.size, d[np.minimum(ff + 1, d.size - 1)], 1)
    stops = ff[nxt != 0]                                             # an FF that is not followed by 00 ends the supply
    pos, out, records, rst = info["scan"], [], [], 0
    at = 0
    for first in range(0, n_mcu, interval):
        later = stops[stops >= pos]
        stop = int(later[0]) if later.size else d.size
        seg = d[pos:stop]
        keep = np.ones(seg.size, dtype=bool)
        keep[1:][seg[:-1] == 0xFF] = False                          # the 00 after every FF inside the segment
        seg = seg[keep]
        last = first + interval >= n_mcu
        records.append((first, n_mcu - first if last else interval, at, 8 * seg.size, 0 if last else 1))
        pad = -seg.size % 4
        out += [seg, np.zeros(pad, dtype=np.uint8)]
        at += seg.size + pad
        if not last:
            p = stop
            while p < d.size and d[p] == 0xFF:
                p += 1
            if p >= d.size or p == stop or d[p] != 0xD0 + rst:
                raise BadRestart(first)
            rst = (rst + 1) & 7
            pos = p + 1
    return info, np.concatenate(out) if out else np.zeros(0, dtype=np.uint8), records


def table_layout(table):
    """tsod_jpeg_huff's four arrays from jpeg_restated's {(length, code): symbol}."""
    look = np.zeros(512, dtype=np.uint16)
    maxcode, valoff = np.zeros(17, dtype=np.int32), np.zeros(17, dtype=np.int32)
    vals = np.zeros(256, dtype=np.uint8)
    code = k = 0
    for length in range(1, 17):
        codes = sorted(c for (l, c) in table if l == length)
        assert codes == list(range(code, code + len(codes)))
        valoff[length] = k - code
        for c in codes:
            vals[k] = table[(length, c)]
            if length <= 9:
                look[c << (9 - length):(c + 1) << (9 - length)] = (length << 8) | table[(length, c)]
            k += 1
        code += len(codes)
        maxcode[length] = code - 1 if codes else -1
        code <<= 1
    return look, maxcode, valoff, vals


def entropy_range(data):
    """[first, last): the bytes between the SOS header and the EOI marker."""
    data = bytes(data)
    assert data[-2:] == b"\xff\xd9"
    return R.parse(data)["scan"], len(data) - 2


def corruptions(data, count, seed):
    """`count` copies of the file, each with one byte of its entropy-coded segment XORed with a nonzero value."""
    first, last = entropy_range(data)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(data)
        b[int(rng.integers(first, last))] ^= int(rng.integers(1, 256))
        out.append(bytes(b))
    return out


# The damaged files of the status tests: one fixture per sampling, one of them with restart markers, 200 seeded draws each.
# tests/test_jpeg_scan_abi.py sweeps exactly these through the CPU program before tests/test_jpeg_huffman_gpu.py runs them.
STATUS_FIXTURES = ("37x53_s2_rstr", "37x53_s1_q75", "37x53_s0_opt")


def status_corruptions(name, data):
    return corruptions(data, 200, 7000 + STATUS_FIXTURES.index(name))
