// jpeg_huffman_core.h -- the per-lane core of the device Huffman pass: the bit reader over an unstuffed
// big-endian word stream, T.81 F.2.2.3 DECODE and F.2.2.1 RECEIVE + EXTEND on the fixed-size table of include/tsod.h, and the
// step from parser state to parser state.  Every function is __host__ __device__-clean: csrc/jpeg_huffman.hip runs it one lane
// per subsequence, tests/jpeg_huffman_main.cpp runs the very same code lane by lane on the CPU (under ASan / UBSan, and that
// program is where to use gdb).  No statics, no allocation.  Nothing is read outside [words, words + n_words) or the tables,
// nothing is written outside the blocks of the segment's own MCUs.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "jpeg_entropy.h"

#if defined(__HIPCC__)
#define TSOD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TSOD_HD inline
#endif

namespace tsod_jpeg {

constexpr int kHuffLanes = 256;          // subsequences per round: one lane each
constexpr int kHuffTables = TSOD_JPEG_HUFF_TABLES;
constexpr uint32_t kErrorP = 0xFFFFFFFFu;
constexpr int32_t kStatusError = 1, kStatusBlocks = 2, kStatusLeftover = 4;   // bits of status[image]

// One restart interval as the lanes see it: `words` starts the segment, n_words = ceil(bits / 32) is its padded extent.
struct SegmentBits {
    const uint32_t *words;               // memory order; a word's first byte holds its first bits
    uint32_t n_words, bits;
};

// The parser state between two symbols: the bit position of the next one, the block slot inside the MCU and the zigzag index
// (0: a DC symbol is next).  p == kErrorP is the one absorbing ERROR value: an invalid code, a DC category above 15, a run
// past coefficient 63, the end of the bits inside a symbol.
struct HuffState {
    uint32_t p, mz;                      // mz = m << 8 | z
};
TSOD_HD bool same(const HuffState &a, const HuffState &b) { return a.p == b.p && a.mz == b.mz; }
TSOD_HD HuffState error_state() { return HuffState{kErrorP, 0u}; }

// Completed blocks and the sums of DC differences of each component (wrapping uint32, as on the host): what a lane adds, and -
// scanned over the lanes before it plus the carry of the rounds before - where it stands.
struct HuffTally {
    uint32_t blocks, dc[3];
};

// What the address of a block needs, from the checked image record and the checked segment record only.
struct HuffGeometry {
    int64_t coef0, coef1, coef2;         // coef_offset and blocks_w of each component (named, not arrays: they stay in registers)
    int32_t bw0, bw1, bw2;
    int32_t n_comp, hs, vs, luma_slots, slots, mcus_x, first_mcu;
    uint32_t n_blocks;                   // n_mcu * slots
};

TSOD_HD HuffGeometry huff_geometry(const tsod_jpeg_image &im, const tsod_jpeg_segment &seg) {
    HuffGeometry g;
    g.coef0 = im.coef_offset[0], g.coef1 = im.coef_offset[1], g.coef2 = im.coef_offset[2];
    g.bw0 = im.blocks_w[0], g.bw1 = im.blocks_w[1], g.bw2 = im.blocks_w[2];
    g.n_comp = im.n_comp, g.hs = im.hs, g.vs = im.vs;
    g.luma_slots = im.hs * im.vs;
    g.slots = g.luma_slots + (im.n_comp == 3 ? 2 : 0);
    g.mcus_x = im.blocks_w[0] / im.hs;
    g.first_mcu = seg.first_mcu;
    g.n_blocks = (uint32_t)seg.n_mcu * (uint32_t)g.slots;
    return g;
}

TSOD_HD int slot_component(const HuffGeometry &g, int m) { return m < g.luma_slots ? 0 : 1 + m - g.luma_slots; }

// The host pass's MCU -> (component, v, h) -> block address arithmetic for block number `b` of the segment, b < g.n_blocks
TSOD_HD int64_t block_address(const HuffGeometry &g, uint32_t b) {
    const int mcu = g.first_mcu + (int)(b / (uint32_t)g.slots), m = (int)(b % (uint32_t)g.slots);
    const int my = mcu / g.mcus_x, mx = mcu % g.mcus_x;
    const int c = slot_component(g, m);
    const int v = c ? 0 : m / g.hs, h = c ? 0 : m % g.hs;
    const int vc = c ? 1 : g.vs, hc = c ? 1 : g.hs;
    const int64_t base = c == 0 ? g.coef0 : (c == 1 ? g.coef1 : g.coef2);
    const int32_t bw = c == 0 ? g.bw0 : (c == 1 ? g.bw1 : g.bw2);
    return base + ((int64_t)(my * vc + v) * bw + (mx * hc + h)) * 64;
}

TSOD_HD uint32_t load_be(const SegmentBits &s, uint32_t w) {
    if (w >= s.n_words) return 0u;                               // clamped to the segment's padded extent
    const uint32_t x = s.words[w];
    return (x << 24) | ((x & 0xFF00u) << 8) | ((x >> 8) & 0xFF00u) | (x >> 24);
}

// The bit reader of one lane: `acc` holds the next `have` bits of the segment at its top, have >= 33 between symbols, so its
// upper word is a full 32-bit window (no symbol with its value is longer than 31 bits); zeros beyond the segment.  The word
// after those is already loaded into `next` when the window is refilled, so a symbol never waits for the load it causes.
struct BitWindow {
    uint64_t acc;
    uint32_t have, next, w;              // w: the word `next` was loaded from, plus one
};
TSOD_HD BitWindow open_window(const SegmentBits &s, uint32_t p) {
    const uint32_t w = p >> 5, sh = p & 31u;
    BitWindow b;
    b.acc = (((uint64_t)load_be(s, w) << 32) | load_be(s, w + 1)) << sh;
    b.have = 64u - sh;
    b.next = load_be(s, w + 2);
    b.w = w + 3;
    return b;
}
TSOD_HD uint32_t window32(const BitWindow &b) { return (uint32_t)(b.acc >> 32); }
TSOD_HD void consume(const SegmentBits &s, BitWindow &b, uint32_t n) {      // 1 <= n <= 31
    b.acc <<= n;
    b.have -= n;
    if (b.have <= 32u) {
        b.acc |= (uint64_t)b.next << (32u - b.have);
        b.have += 32u;
        b.next = load_be(s, b.w++);
    }
}

// T.81 F.2.2.3 DECODE on the top bits of `window`, of which `avail` are real: the symbol, -1 for a code the table does not
// hold or bits that are not there.  `len` is the code's length.
TSOD_HD int decode_symbol(uint32_t window, uint32_t avail, const tsod_jpeg_huff &h, uint32_t &len) {
    const uint16_t e = h.look[window >> (32 - kLookBits)];
    if (e) {
        len = (uint32_t)(e >> 8);
        return len <= avail ? (int)(e & 0xFF) : -1;
    }
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(window >> (32 - l));
        if (code <= h.maxcode[l]) {
            len = (uint32_t)l;
            return len <= avail ? (int)h.vals[(uint32_t)(h.valoff[l] + code) & 255u] : -1;
        }
    }
    return -1;
}

// T.81 F.2.2.1 RECEIVE + EXTEND of the s bits (1 <= s <= 15) that follow the first `len` bits of `window`
TSOD_HD int32_t receive_extend(uint32_t window, uint32_t len, int s) {
    int32_t v = (int32_t)((window << len) >> (32 - s));
    if (v < (1 << (s - 1))) v -= (1 << s) - 1;
    return v;
}

// One lane's work: from state `st`, every symbol that starts before bit `limit` (the end of the lane's subsequence or of the
// segment); the last one may run past it.  `t` counts completed blocks and sums DC differences on top of what it holds.
// kWrite == false (the fixpoint passes): t starts at zero and nothing is stored.  kWrite == true (the last pass): t starts at
// the lane's true standing - the block number and the running predictions - and the coefficients are stored; the walk stops
// at the segment's block count, and `flags` collects what makes status[image] nonzero.  A store happens only for a block
// number below g.n_blocks and k <= 63.  The loop is bounded by the bits of the subsequence: a symbol takes at least one.
template <bool kWrite>
TSOD_HD HuffState huff_run(const SegmentBits &s, const tsod_jpeg_huff *tables, const HuffGeometry &g, HuffState st, uint32_t limit,
                           uint32_t max_symbols, bool restart_follows, HuffTally &t, int16_t *coef, int32_t &flags) {
    if (st.p == kErrorP || st.p >= limit) {                      // nothing starts here
        if (kWrite && st.p == kErrorP && t.blocks < g.n_blocks) flags |= kStatusError;
        return st;
    }
    BitWindow bw = open_window(s, st.p);
    for (uint32_t it = 0; it < max_symbols; ++it) {
        if (st.p == kErrorP || st.p >= limit) break;
        if (kWrite && t.blocks >= g.n_blocks) break;
        int m = (int)(st.mz >> 8), z = (int)(st.mz & 255u);
        const int c = slot_component(g, m);
        const uint32_t window = window32(bw), avail = s.bits - st.p;
        uint32_t len = 0;
        bool done = false;                                       // the block is complete
        if (z == 0) {
            const int sz = decode_symbol(window, avail, tables[2 * c], len);
            if (sz < 0 || sz > 15 || len + (uint32_t)sz > avail) { st = error_state(); break; }
            const uint32_t diff = sz ? (uint32_t)receive_extend(window, len, sz) : 0u;
            t.dc[0] += c == 0 ? diff : 0u, t.dc[1] += c == 1 ? diff : 0u, t.dc[2] += c == 2 ? diff : 0u;
            if (kWrite) coef[block_address(g, t.blocks)] = (int16_t)(uint16_t)(c == 0 ? t.dc[0] : (c == 1 ? t.dc[1] : t.dc[2]));
            st.p += len + (uint32_t)sz;
            consume(s, bw, len + (uint32_t)sz);
            z = 1;
        } else {
            const int rs = decode_symbol(window, avail, tables[2 * c + 1], len);
            if (rs < 0) { st = error_state(); break; }
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                if (r != 15) {
                    done = true;                                 // EOB
                } else if (z + 15 > 63) {
                    st = error_state();                          // ZRL past coefficient 63
                    break;
                } else {
                    z += 16;                                     // ZRL
                    done = z == 64;
                }
                st.p += len;
                consume(s, bw, len);
            } else {
                z += r;
                if (z > 63 || len + (uint32_t)sz > avail) { st = error_state(); break; }
                if (kWrite) coef[block_address(g, t.blocks) + kNatural[z]] = (int16_t)receive_extend(window, len, sz);
                st.p += len + (uint32_t)sz;
                consume(s, bw, len + (uint32_t)sz);
                done = ++z == 64;
            }
        }
        if (done) {
            t.blocks += 1;
            m = m + 1 == g.slots ? 0 : m + 1;
            z = 0;
            if (kWrite && t.blocks == g.n_blocks && restart_follows && s.bits - st.p >= 8) flags |= kStatusLeftover;
        }
        st.mz = (uint32_t)m << 8 | (uint32_t)z;
    }
    if (kWrite && st.p == kErrorP && t.blocks < g.n_blocks) flags |= kStatusError;
    return st;
}

// The start a lane assumes before it knows better: its subsequence's first bit, at the start of an MCU
TSOD_HD HuffState assumed_state(uint32_t first_bit) { return HuffState{first_bit, 0u}; }

}  // namespace tsod_jpeg
