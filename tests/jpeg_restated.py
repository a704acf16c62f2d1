"""NumPy restatement of the JPEG decoder, written from ITU-T T.81 and the arithmetic stated in
include/tsod.h: marker parsing, the Huffman pass, dequantisation with the 13-bit integer inverse DCT, chroma upsampling and the
YCbCr conversion.  It is the definition the library's host decoder and the two kernels are held to, and is itself held to
Pillow's pixels through tests/golden/jpeg_ref.npz.  All 32-bit arithmetic wraps (int32 arrays)."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


class Unsupported(Exception):
    pass


class Corrupt(Exception):
    pass


def _huffman(counts, vals):
    """T.81 Annex C: {(length, code): symbol}."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


def parse(data):
    """The markers up to the first scan: a dict with the frame, the tables and the offset of the entropy-coded bytes."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise Corrupt("no SOI")
    quant, dc, ac, frame, restart, adobe = {}, {}, {}, None, 0, None
    pos = 2
    while True:
        if pos + 2 > len(data) or data[pos] != 0xFF:
            raise Corrupt("marker expected")
        while pos < len(data) and data[pos] == 0xFF:
            pos += 1
        if pos >= len(data):
            raise Corrupt("truncated")
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0x00, 0xD8, 0xD9):
            raise Corrupt("unexpected marker")
        if 0xC0 <= m <= 0xCF and m not in (0xC0, 0xC1, 0xC4):
            raise Unsupported(f"SOF{m - 0xC0}")
        if pos + 2 > len(data):
            raise Corrupt("truncated")
        length = int.from_bytes(data[pos:pos + 2], "big")
        if length < 2 or pos + length > len(data):
            raise Corrupt("segment length")
        seg = data[pos + 2:pos + length]
        pos += length
        if m == 0xDB:
            while seg:
                pq, tq = seg[0] >> 4, seg[0] & 15
                n = 128 if pq else 64
                if pq > 1 or tq > 3 or len(seg) < 1 + n:
                    raise Corrupt("DQT")
                q = np.frombuffer(seg[1:1 + n], dtype=">u2" if pq else np.uint8).astype(np.int64)
                table = np.zeros(64, dtype=np.int64)
                table[ZIGZAG] = q
                quant[tq] = table
                seg = seg[1 + n:]
        elif m == 0xC4:
            while seg:
                tc, th = seg[0] >> 4, seg[0] & 15
                counts = list(seg[1:17])
                if tc > 1 or th > 3 or len(counts) < 16 or len(seg) < 17 + sum(counts):
                    raise Corrupt("DHT")
                (ac if tc else dc)[th] = _huffman(counts, list(seg[17:17 + sum(counts)]))
                seg = seg[17 + sum(counts):]
        elif m in (0xC0, 0xC1):
            if seg[0] != 8:
                raise Unsupported("precision")
            H, W, n_comp = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            if H == 0 or W == 0 or n_comp == 0:
                raise Corrupt("dimensions")
            if n_comp not in (1, 3):
                raise Unsupported("components")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(n_comp)]
            if n_comp == 1:
                comps = [(comps[0][0], 1, 1, comps[0][3])]
            elif (comps[0][1:3] not in ((1, 1), (2, 1), (2, 2))) or comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1):
                raise Unsupported("sampling")
            frame = dict(H=H, W=W, comps=comps)
        elif m == 0xDD:
            restart = int.from_bytes(seg[:2], "big")
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Corrupt("SOS before SOF")
            ns = seg[0]
            if ns != len(frame["comps"]):
                raise Unsupported("multi-scan")
            sel = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ns)]
            if adobe == 0 and ns == 3:
                raise Unsupported("Adobe RGB")
            break
    hmax, vmax = frame["comps"][0][1], frame["comps"][0][2]
    mcus_x, mcus_y = -(-frame["W"] // (8 * hmax)), -(-frame["H"] // (8 * vmax))
    return dict(H=frame["H"], W=frame["W"], n_comp=len(frame["comps"]), h=[c[1] for c in frame["comps"]],
                v=[c[2] for c in frame["comps"]], tq=[c[3] for c in frame["comps"]], hmax=hmax, vmax=vmax, mcus_x=mcus_x,
                mcus_y=mcus_y, restart_interval=restart, blocks_w=[mcus_x * c[1] for c in frame["comps"]],
                blocks_h=[mcus_y * c[2] for c in frame["comps"]], quant=[quant[c[3]] for c in frame["comps"]],
                dc=[dc[s[0]] for s in sel], ac=[ac[s[1]] for s in sel], scan=pos)


class _Bits:
    """The entropy-coded segment as a string of bits, FF 00 unstuffed, cut at every marker."""

    def __init__(self, data, pos):
        self.data, self.pos, self.bits, self.at = data, pos, "", 0
        self._load()

    def _load(self):
        out, d, p = [], self.data, self.pos
        while p < len(d):
            if d[p] == 0xFF:
                if p + 1 >= len(d) or d[p + 1] != 0:
                    break
                out.append(0xFF)
                p += 2
            else:
                out.append(d[p])
                p += 1
        self.pos, self.at = p, 0
        self.bits = "".join(format(b, "08b") for b in out)

    def take(self, n):
        if self.at + n > len(self.bits):
            raise Corrupt("out of bits")
        v = int(self.bits[self.at:self.at + n], 2) if n else 0
        self.at += n
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (length, code) in table:
                return table[(length, code)]
        raise Corrupt("bad code")

    def restart(self, expected):
        p = self.pos
        while p < len(self.data) and self.data[p] == 0xFF:
            p += 1
        if p >= len(self.data) or p == self.pos or self.data[p] != 0xD0 + expected or len(self.bits) - self.at >= 8:
            raise Corrupt("restart marker")
        self.pos = p + 1
        self._load()


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy_decode(data, info=None):
    """(info, [int16 [blocks_h, blocks_w, 64] per component]): coefficients in natural order, not dequantised."""
    data = bytes(data)
    info = info or parse(data)
    coefs = [np.zeros((info["blocks_h"][c], info["blocks_w"][c], 64), dtype=np.int16) for c in range(info["n_comp"])]
    bits = _Bits(data, info["scan"])
    pred, rst, ri = [0] * 3, 0, info["restart_interval"]
    for mcu in range(info["mcus_x"] * info["mcus_y"]):
        if ri and mcu and mcu % ri == 0:
            bits.restart(rst)
            rst, pred = (rst + 1) & 7, [0] * 3
        my, mx = divmod(mcu, info["mcus_x"])
        for c in range(info["n_comp"]):
            for v in range(info["v"][c]):
                for h in range(info["h"][c]):
                    blk = coefs[c][my * info["v"][c] + v, mx * info["h"][c] + h]
                    s = bits.symbol(info["dc"][c])
                    if s > 15:
                        raise Corrupt("DC category")
                    if s:
                        pred[c] += _extend(bits.take(s), s)
                    blk[0] = np.array(pred[c] & 0xFFFF, dtype=np.uint16).astype(np.int16)
                    k = 1
                    while k < 64:
                        rs = bits.symbol(info["ac"][c])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            if k + 15 > 63:
                                raise Corrupt("run")
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise Corrupt("run")
                        blk[ZIGZAG[k]] = np.array(_extend(bits.take(s), s) & 0xFFFF, dtype=np.uint16).astype(np.int16)
                        k += 1
    return info, coefs


def _descale(x, n):
    return (x + np.int32(1 << (n - 1))) >> n


def _pass(d, n):
    """One 8-point pass along axis 0 of int32 ``d`` [8, ...] (jidctint.c), descaled by n bits."""
    i32 = np.int32
    z1 = (d[2] + d[6]) * i32(4433)
    tmp2 = z1 + d[6] * i32(-15137)
    tmp3 = z1 + d[2] * i32(6270)
    tmp0 = (d[0] + d[4]) << 13
    tmp1 = (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * i32(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * i32(2446), tmp1 * i32(16819), tmp2 * i32(25172), tmp3 * i32(12299)
    z1, z2, z3, z4 = z1 * i32(-7373), z2 * i32(-20995), z3 * i32(-16069) + z5, z4 * i32(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([_descale(tmp10 + tmp3, n), _descale(tmp11 + tmp2, n), _descale(tmp12 + tmp1, n), _descale(tmp13 + tmp0, n),
                     _descale(tmp13 - tmp0, n), _descale(tmp12 - tmp1, n), _descale(tmp11 - tmp2, n), _descale(tmp10 - tmp3, n)])


def idct_blocks(coef, quant):
    """u8 [n, 8, 8] samples of int16 [n, 64] coefficients with the 64 quantiser entries ``quant`` (values up to 65535)."""
    with np.errstate(over="ignore"):
        q = np.asarray(quant).astype(np.int64).astype(np.int32).reshape(1, 64)
        d = (np.asarray(coef, dtype=np.int16).astype(np.int32) * q).reshape(-1, 8, 8)
        ws = _pass(d.transpose(1, 0, 2), 11)                     # columns: axis 0 = the row index
        out = _pass(ws.transpose(2, 1, 0), 18)                   # rows: axis 0 = the column index -> [col, n, row]
    j = out.transpose(1, 2, 0) & 1023
    return np.where(j < 128, j + 128, np.where(j < 512, 255, np.where(j < 896, 0, j - 896))).astype(np.uint8)


def planes_from(info, coefs):
    """The u8 component planes [8 blocks_h, 8 blocks_w] of the coefficient arrays of ``entropy_decode``."""
    planes = []
    for c, co in enumerate(coefs):
        bh, bw = co.shape[:2]
        px = idct_blocks(co.reshape(-1, 64), info["quant"][c]).reshape(bh, bw, 8, 8)
        planes.append(np.ascontiguousarray(px.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)))
    return planes


def upsample(plane, H, W, hs, vs):
    """int32 [H, W]: one chroma plane (any padded size) brought to the image's size by libjpeg's rules."""
    dw, dh = -(-W // hs), -(-H // vs)
    a = plane[:dh, :dw].astype(np.int32)
    if hs == 1:
        return a[:H, :W]
    if dw <= 2:
        return np.repeat(np.repeat(a, vs, axis=0), 2, axis=1)[:H, :W]
    left, right = np.concatenate([a[:, :1], a[:, :-1]], axis=1), np.concatenate([a[:, 1:], a[:, -1:]], axis=1)
    out = np.empty((dh * vs, 2 * dw), dtype=np.int32)
    if vs == 1:
        out[:, 0::2] = (3 * a + left + 1) >> 2
        out[:, 1::2] = (3 * a + right + 2) >> 2
        return out[:H, :W]
    up, down = np.concatenate([a[:1], a[:-1]], axis=0), np.concatenate([a[1:], a[-1:]], axis=0)
    for parity, other in ((0, up), (1, down)):
        t = 3 * a + other
        tl, tr = np.concatenate([t[:, :1], t[:, :-1]], axis=1), np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
        out[parity::2, 0::2] = (3 * t + tl + 8) >> 4
        out[parity::2, 1::2] = (3 * t + tr + 7) >> 4
    return out[:H, :W]


def to_rgb(planes, H, W, hs=1, vs=1):
    """u8 [H, W, 3] from the component planes (one: grey; three: Y Cb Cr with luma sampling hs x vs)."""
    y = planes[0][:H, :W].astype(np.int32)
    if len(planes) == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    cb, cr = upsample(planes[1], H, W, hs, vs) - 128, upsample(planes[2], H, W, hs, vs) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data):
    """u8 [H, W, 3]: what Pillow's Image.open(...).convert("RGB") gives for a supported file."""
    info, coefs = entropy_decode(data)
    return to_rgb(planes_from(info, coefs), info["H"], info["W"], info["hmax"], info["vmax"])
