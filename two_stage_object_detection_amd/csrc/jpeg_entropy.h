// jpeg_entropy.h -- the host half of the JPEG decoder: marker parsing and the Huffman pass of one
// baseline / extended-sequential file into int16 coefficients.  Plain C++17, no HIP, no statics, no allocation: every table lives
// in a tsod_jpeg::State on the caller's stack, so any number of threads may decode at once.  Nothing is read outside
// [data, data + n) and nothing is written outside [coef, coef + capacity).  Written from ITU-T T.81 (Annex B markers, Annex C
// code tables, Annex F.2 decoding).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/tsod.h"

namespace tsod_jpeg {

// T.81 Figure A.6: position in the zigzag sequence -> natural (row-major) position
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLookBits = 9;

struct Huffman {
    bool present;
    uint8_t vals[256];
    int32_t maxcode[17];              // largest code of each length, -1 when the length has none
    int32_t valoff[17];               // vals index of a length's first code, minus that code
    uint16_t look[1 << kLookBits];    // (length << 8) | symbol for codes of at most kLookBits bits, 0: longer or absent
};

struct State {
    tsod_jpeg_info info;
    uint16_t quant[4][64];            // natural order
    bool quant_present[4];
    Huffman dc[4], ac[4];
    int td[3], ta[3];                 // the scan's table selectors
    size_t scan;                      // offset of the entropy-coded segment
};

inline int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

// T.81 Annex C: the code table from BITS and HUFFVAL.  `p` holds the 16 counts and then the values, `len` bytes in all.
// Returns the bytes used, or 0 when the table is cut short or assigns more codes to a length than the length has.
inline size_t build_huffman(Huffman &h, const uint8_t *p, size_t len) {
    if (len < 16) return 0;
    int total = 0;
    for (int l = 1; l <= 16; ++l) total += p[l - 1];
    if (total > 256 || len < 16 + (size_t)total) return 0;
    memset(&h, 0, sizeof(h));
    memcpy(h.vals, p + 16, (size_t)total);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int count = p[l - 1];
        if (code + count > (1 << l)) return 0;
        h.valoff[l] = k - code;
        for (int i = 0; i < count; ++i, ++k, ++code)
            if (l <= kLookBits) {
                const int first = code << (kLookBits - l);
                for (int j = 0; j < (1 << (kLookBits - l)); ++j) h.look[first + j] = (uint16_t)((l << 8) | h.vals[k]);
            }
        h.maxcode[l] = count ? code - 1 : -1;
        code <<= 1;
    }
    h.present = true;
    return 16 + (size_t)total;
}

// Markers up to the first scan.  On TSOD_OK st.info is complete and st.scan is where the entropy-coded bytes start.
inline int parse(const uint8_t *data, size_t n, State &st) {
    memset(&st, 0, sizeof(st));
    if (!data || n < 4 || data[0] != 0xFF || data[1] != 0xD8) return TSOD_ERR_INVALID_ARG;
    tsod_jpeg_info &info = st.info;
    bool have_frame = false, adobe_rgb = false;
    uint8_t comp_id[3] = {0, 0, 0};
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n || data[pos] != 0xFF) return TSOD_ERR_INVALID_ARG;
        while (pos < n && data[pos] == 0xFF) ++pos;              // fill bytes
        if (pos >= n) return TSOD_ERR_INVALID_ARG;
        const int m = data[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;     // TEM, RSTn: no segment
        if (m == 0x00 || m == 0xD8 || m == 0xD9) return TSOD_ERR_INVALID_ARG;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC0 && m != 0xC1 && m != 0xC4) return TSOD_ERR_UNSUPPORTED;   // other frame types
        if (pos + 2 > n) return TSOD_ERR_INVALID_ARG;
        const size_t len = (size_t)be16(data + pos);
        if (len < 2 || len > n - pos) return TSOD_ERR_INVALID_ARG;
        const uint8_t *p = data + pos + 2;
        size_t left = len - 2;
        pos += len;
        if (m == 0xDB) {                                         // DQT
            while (left) {
                const int pq = p[0] >> 4, tq = p[0] & 15;
                const size_t need = 1 + (pq ? 128u : 64u);
                if (pq > 1 || tq > 3 || left < need) return TSOD_ERR_INVALID_ARG;
                for (int i = 0; i < 64; ++i) st.quant[tq][kNatural[i]] = (uint16_t)(pq ? be16(p + 1 + 2 * i) : p[1 + i]);
                st.quant_present[tq] = true;
                p += need, left -= need;
            }
        } else if (m == 0xC4) {                                  // DHT
            while (left) {
                const int tc = p[0] >> 4, th = p[0] & 15;
                if (tc > 1 || th > 3) return TSOD_ERR_INVALID_ARG;
                const size_t used = build_huffman(tc ? st.ac[th] : st.dc[th], p + 1, left - 1);
                if (!used) return TSOD_ERR_INVALID_ARG;
                p += 1 + used, left -= 1 + used;
            }
        } else if (m == 0xC0 || m == 0xC1) {                     // SOF0 / SOF1
            if (have_frame || left < 6) return TSOD_ERR_INVALID_ARG;
            if (p[0] != 8) return TSOD_ERR_UNSUPPORTED;
            info.H = be16(p + 1), info.W = be16(p + 3), info.n_comp = p[5];
            if (info.H == 0 || info.W == 0 || info.n_comp == 0) return TSOD_ERR_INVALID_ARG;
            if (info.n_comp != 1 && info.n_comp != 3) return TSOD_ERR_UNSUPPORTED;
            if (left != 6 + 3 * (size_t)info.n_comp) return TSOD_ERR_INVALID_ARG;
            for (int c = 0; c < info.n_comp; ++c) {
                const uint8_t *q = p + 6 + 3 * c;
                comp_id[c] = q[0];
                info.h[c] = q[1] >> 4, info.v[c] = q[1] & 15, info.tq[c] = q[2];
                if (info.h[c] < 1 || info.h[c] > 4 || info.v[c] < 1 || info.v[c] > 4 || info.tq[c] > 3) return TSOD_ERR_INVALID_ARG;
            }
            if (info.n_comp == 1) {
                info.h[0] = info.v[0] = 1;                       // a one-component scan is never interleaved (T.81 A.2.2)
            } else {
                const bool luma = (info.h[0] == 1 && info.v[0] == 1) || (info.h[0] == 2 && info.v[0] <= 2);
                if (!luma || info.h[1] != 1 || info.v[1] != 1 || info.h[2] != 1 || info.v[2] != 1) return TSOD_ERR_UNSUPPORTED;
            }
            have_frame = true;
        } else if (m == 0xDD) {                                  // DRI
            if (left != 2) return TSOD_ERR_INVALID_ARG;
            info.restart_interval = be16(p);
        } else if (m == 0xEE) {                                  // APP14: Adobe's colour transform flag
            if (left >= 12 && memcmp(p, "Adobe", 5) == 0 && p[11] == 0) adobe_rgb = true;
        } else if (m == 0xDA) {                                  // SOS
            if (!have_frame || left < 1) return TSOD_ERR_INVALID_ARG;
            const int ns = p[0];
            if (ns < 1 || ns > 4 || left != 4 + 2 * (size_t)ns) return TSOD_ERR_INVALID_ARG;
            if (ns != info.n_comp) return TSOD_ERR_UNSUPPORTED;  // one scan per component: not built
            for (int c = 0; c < ns; ++c) {
                if (p[1 + 2 * c] != comp_id[c]) return TSOD_ERR_UNSUPPORTED;
                st.td[c] = p[2 + 2 * c] >> 4, st.ta[c] = p[2 + 2 * c] & 15;
                if (st.td[c] > 3 || st.ta[c] > 3) return TSOD_ERR_INVALID_ARG;
                if (!st.dc[st.td[c]].present || !st.ac[st.ta[c]].present || !st.quant_present[info.tq[c]]) return TSOD_ERR_INVALID_ARG;
            }
            const uint8_t *tail = p + 1 + 2 * ns;
            if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return TSOD_ERR_INVALID_ARG;
            if (adobe_rgb && info.n_comp == 3) return TSOD_ERR_UNSUPPORTED;
            break;
        }                                                        // APPn, COM and the rest: skipped
    }
    info.hmax = info.h[0], info.vmax = info.v[0];
    info.mcus_x = (info.W + 8 * info.hmax - 1) / (8 * info.hmax);
    info.mcus_y = (info.H + 8 * info.vmax - 1) / (8 * info.vmax);
    for (int c = 0; c < info.n_comp; ++c) {
        info.blocks_w[c] = info.mcus_x * info.h[c], info.blocks_h[c] = info.mcus_y * info.v[c];
        info.plane_w[c] = 8 * info.blocks_w[c], info.plane_h[c] = 8 * info.blocks_h[c];
        info.coef_count[c] = (int64_t)64 * info.blocks_w[c] * info.blocks_h[c];
        info.coef_total += info.coef_count[c];
        memcpy(info.quant[c], st.quant[info.tq[c]], sizeof(info.quant[c]));
    }
    st.scan = pos;
    return TSOD_OK;
}

// T.81 F.2.2.5 NEXTBIT with byte stuffing (FF 00 -> FF): `acc` holds `cnt` real bits at its top, zeros below them.  A marker or
// the end of the data stops the supply; asking for more bits than there are is an error.
struct Bits {
    const uint8_t *data;
    size_t pos, end;
    uint64_t acc;
    int cnt;
    bool stopped;

    void fill() {
        while (cnt <= 56 && !stopped) {
            if (pos >= end) { stopped = true; break; }
            const uint8_t b = data[pos];
            if (b == 0xFF) {
                if (pos + 1 >= end || data[pos + 1] != 0x00) { stopped = true; break; }
                pos += 2;
            } else {
                pos += 1;
            }
            acc |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    uint32_t peek(int nbits) const { return (uint32_t)(acc >> (64 - nbits)); }
    bool take(int nbits) {
        if (nbits > cnt) return false;
        acc <<= nbits, cnt -= nbits;
        return true;
    }
};

// T.81 F.2.2.3 DECODE: -1 for a code the table does not hold or bits that are not there
inline int decode_symbol(Bits &b, const Huffman &h) {
    if (b.cnt < 32) b.fill();                                    // (no code or value is longer than 16 bits)
    const uint16_t e = h.look[b.peek(kLookBits)];
    if (e) return b.take(e >> 8) ? (e & 0xFF) : -1;
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)b.peek(l);
        if (code <= h.maxcode[l]) return b.take(l) ? h.vals[h.valoff[l] + code] : -1;
    }
    return -1;
}

// T.81 F.2.2.1 RECEIVE + EXTEND of an s-bit value, 1 <= s <= 15
inline bool receive_extend(Bits &b, int s, int32_t &v) {
    if (b.cnt < 32) b.fill();
    v = (int32_t)b.peek(s);
    if (!b.take(s)) return false;
    if (v < (1 << (s - 1))) v -= (1 << s) - 1;
    return true;
}

// The Huffman pass: coefficients in natural order, not dequantised, component after component, each block-raster over its
// padded grid (info.blocks_w x info.blocks_h blocks of 64).  Writes exactly [coef, coef + info.coef_total).
inline int decode(const uint8_t *data, size_t n, int16_t *coef, size_t capacity, State &st) {
    const int rc = parse(data, n, st);
    if (rc != TSOD_OK) return rc;
    const tsod_jpeg_info &info = st.info;
    if (!coef || capacity < (size_t)info.coef_total) return TSOD_ERR_INVALID_ARG;
    memset(coef, 0, (size_t)info.coef_total * sizeof(int16_t));
    int16_t *base[3] = {coef, coef + info.coef_count[0], coef + info.coef_count[0] + info.coef_count[1]};
    Bits b = {data, st.scan, n, 0, 0, false};
    int32_t pred[3] = {0, 0, 0};
    const int64_t n_mcu = (int64_t)info.mcus_x * info.mcus_y;
    int next_rst = 0;
    for (int64_t mcu = 0; mcu < n_mcu; ++mcu) {
        if (info.restart_interval && mcu && mcu % info.restart_interval == 0) {
            b.fill();                                            // what is left are the pad bits of the last byte
            if (!b.stopped || b.cnt >= 8) return TSOD_ERR_INVALID_ARG;
            size_t p = b.pos;
            while (p < n && data[p] == 0xFF) ++p;
            if (p >= n || p == b.pos || data[p] != 0xD0 + next_rst) return TSOD_ERR_INVALID_ARG;
            next_rst = (next_rst + 1) & 7;
            b.pos = p + 1, b.acc = 0, b.cnt = 0, b.stopped = false;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int my = (int)(mcu / info.mcus_x), mx = (int)(mcu % info.mcus_x);
        for (int c = 0; c < info.n_comp; ++c)
            for (int v = 0; v < info.v[c]; ++v)
                for (int h = 0; h < info.h[c]; ++h) {
                    int16_t *blk = base[c] + ((int64_t)(my * info.v[c] + v) * info.blocks_w[c] + (mx * info.h[c] + h)) * 64;
                    const int s = decode_symbol(b, st.dc[st.td[c]]);
                    if (s < 0 || s > 15) return TSOD_ERR_INVALID_ARG;
                    if (s) {
                        int32_t diff;
                        if (!receive_extend(b, s, diff)) return TSOD_ERR_INVALID_ARG;
                        pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)diff);
                    }
                    blk[0] = (int16_t)(uint16_t)(uint32_t)pred[c];
                    const Huffman &ac = st.ac[st.ta[c]];
                    for (int k = 1; k < 64;) {
                        const int rs = decode_symbol(b, ac);
                        if (rs < 0) return TSOD_ERR_INVALID_ARG;
                        const int r = rs >> 4, sz = rs & 15;
                        if (sz == 0) {
                            if (r != 15) break;                  // EOB
                            if (k + 15 > 63) return TSOD_ERR_INVALID_ARG;
                            k += 16;                             // ZRL
                            continue;
                        }
                        k += r;
                        if (k > 63) return TSOD_ERR_INVALID_ARG;
                        int32_t val;
                        if (!receive_extend(b, sz, val)) return TSOD_ERR_INVALID_ARG;
                        blk[kNatural[k++]] = (int16_t)val;
                    }
                }
    }
    return TSOD_OK;                                              // (a missing EOI is accepted)
}

}  // namespace tsod_jpeg
