// draw.hip -- the detection overlay: the last step of the reference's multi_inference.py:104-154, box outlines and
// text tags painted in place onto u8 RGB images.  The pixel rules are stated once, in include/tsod.h; this file is their per-pixel
// form.
//
//   draw_kernel   one workgroup per kTileW x kTileH tile of one image, one launch for every group.  The item stream of an image
//                 is all outlines (groups ascending, rows in drawn order), then all tags in the same order.  The workgroup reads
//                 the stream kThreads candidates at a time (one per thread), keeps those whose outline ring or tag rectangle
//                 meets the tile and appends them IN ORDER (wave ballots + a four-entry prefix) to a list of kCap entries in
//                 LDS.  When the list is full it is painted and refilled, so the painter's order holds across passes.  Painting:
//                 every thread walks the list - one trip count for the whole workgroup, the entries are LDS broadcasts - for its
//                 kRows pixels, which it loads on first touch, keeps in registers over all passes and stores once at the end.
//                 A tile that no item meets loads and stores nothing.  No atomics; nothing depends on the schedule.
// Compiled with -ffp-contract=off: sx * x1 is one f32 multiply, as the header says.
#include "tsod_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 16;
constexpr int kRows = kTileH / (kThreads / kTileW);      // pixels per thread: rows ly, ly + 4, ly + 8, ly + 12 of column lx
constexpr int kCap = TSOD_DRAW_LIST_CAPACITY;
constexpr int kStr = TSOD_DRAW_STRING_BYTES;
constexpr int kMaxG = TSOD_DRAW_MAX_GROUPS;
constexpr float kCoordMax = 16777216.f;                  // 2^24

struct Glyph {
    unsigned char ch, rows[7];
};
#define TSOD_GLYPH(c, r0, r1, r2, r3, r4, r5, r6) {(unsigned char)(c), {r0, r1, r2, r3, r4, r5, r6}},
const Glyph h_glyphs[] = {
#include "font5x7.h"
};
__constant__ Glyph d_glyphs[] = {
#include "font5x7.h"
};
#undef TSOD_GLYPH
constexpr int kGlyphs = (int)(sizeof(h_glyphs) / sizeof(h_glyphs[0]));
static_assert(kGlyphs <= kThreads, "one glyph per thread when the font is unpacked");

struct Groups {
    tsod_draw_group g[kMaxG];
};

// One list entry.  kind 0: outline, [x0, x1] x [y0, y1] = the box, s = thickness, fill = colour | alpha << 24.
// kind 1: tag, [x0, x1] x [y0, y1] = its rectangle (before clipping), s = font scale, fill = background | alpha << 24.
struct Item {
    int kind, x0, y0, x1, y1, s, pad;
    unsigned fill, ink;
    int len[2];                                          // characters of line 1, line 2 (0: no line 2)
    unsigned char text[2][kStr];
};

__device__ __forceinline__ unsigned pack4(const uint8_t c[4]) {
    return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16 | (unsigned)c[3] << 24;
}

// include/tsod.h "Box to pixels"; false: the row draws nothing
__device__ __forceinline__ bool to_pixel(float s, float v, int &out) {
    if (!isfinite(v)) return false;
    const float p = s * v;
    if (p != p) return false;
    out = (int)rintf(fminf(fmaxf(p, -kCoordMax), kCoordMax));
    return true;
}

// column 5 -> int32: truncated, saturating, NaN -> 0
__device__ __forceinline__ int class_of(float c) {
    if (c != c) return 0;
    if (c >= 2147483648.f) return 2147483647;
    if (c <= -2147483648.f) return -2147483647 - 1;
    return (int)c;
}

__device__ __forceinline__ int decimal_digits(unsigned long long v) {
    int n = 1;
#pragma unroll 1
    for (int k = 0; k < 19; ++k) {                       // (a fixed trip count: no lane waits for another's number)
        v /= 10ull;
        n += v != 0ull ? 1 : 0;
    }
    return n;
}

// length of the zero-terminated string in 32 bytes (8 aligned words), 31 when there is no terminator
__device__ __forceinline__ int string_length(const unsigned *w) {
    int len = kStr - 1;
#pragma unroll
    for (int k = kStr / 4 - 1; k >= 0; --k) {
        const unsigned v = w[k];
        const unsigned zeros = (v - 0x01010101u) & ~v & 0x80808080u;     // its lowest set bit marks the first zero byte
        if (zeros) len = 4 * k + ((__ffs((int)zeros) - 1) >> 3);
    }
    return len < kStr - 1 ? len : kStr - 1;
}

// A candidate of the stream, as the thread that examined it keeps it until it is written into the list.
struct Cand {
    int kind, x0, y0, x1, y1, g, len1;
    long long index;                                     // label index (tags)
    float score;
};

__device__ __forceinline__ void write_item(Item &it, const Cand &c, const tsod_draw_group &G, const unsigned char *strings) {
    it.kind = c.kind;
    it.x0 = c.x0, it.y0 = c.y0, it.x1 = c.x1, it.y1 = c.y1;
    if (c.kind == 0) {
        it.s = G.thickness;
        it.pad = 0;
        it.fill = pack4(G.color);
        it.ink = 0;
        it.len[0] = it.len[1] = 0;
        return;
    }
    it.s = G.font_scale;
    it.pad = G.padding;
    it.fill = pack4(G.tag_bg);
    it.ink = pack4(G.text_rgb) & 0xffffffu;
    it.len[0] = c.len1;
    unsigned *t0 = reinterpret_cast<unsigned *>(it.text[0]);
    if (c.index >= 0 && c.index < (long long)G.string_count) {
        const unsigned *w = reinterpret_cast<const unsigned *>(strings + (G.string_first + c.index) * kStr);
#pragma unroll
        for (int k = 0; k < kStr / 4; ++k) t0[k] = w[k];
    } else {                                             // "class_<index>": at most 6 + 1 + 19 characters
        const char head[6] = {'c', 'l', 'a', 's', 's', '_'};
#pragma unroll
        for (int k = 0; k < 6; ++k) it.text[0][k] = (unsigned char)head[k];
        unsigned long long v = c.index < 0 ? 0ull - (unsigned long long)c.index : (unsigned long long)c.index;
        if (c.index < 0) it.text[0][6] = '-';
        const int first = c.index < 0 ? 7 : 6;
#pragma unroll 1
        for (int k = 0; k < 20; ++k) {                   // (a fixed trip count, as in decimal_digits)
            const int at = c.len1 - 1 - k;
            if (at >= first) it.text[0][at] = (unsigned char)('0' + (int)(v % 10ull));
            v /= 10ull;
        }
    }
    it.len[1] = G.score_line ? 11 : 0;
    if (G.score_line) {
        const char head[6] = {'C', 'o', 'n', 'f', ':', ' '};
#pragma unroll
        for (int k = 0; k < 6; ++k) it.text[1][k] = (unsigned char)head[k];
        unsigned char *d = it.text[1] + 6;
        d[1] = '.';
        if (c.score != c.score) {
            d[0] = d[2] = d[3] = d[4] = '-';
        } else {
            const int m = (int)rintf(fminf(fmaxf(c.score, 0.f), 1.f) * 1000.f);
            d[0] = (unsigned char)('0' + m / 1000);
            d[2] = (unsigned char)('0' + m / 100 % 10);
            d[3] = (unsigned char)('0' + m / 10 % 10);
            d[4] = (unsigned char)('0' + m % 10);
        }
    }
}

__device__ __forceinline__ unsigned blend1(unsigned a, unsigned c, unsigned src) { return (a * c + (255u - a) * src + 127u) / 255u; }

__global__ void __launch_bounds__(kThreads)
draw_kernel(unsigned char *__restrict__ images, int H, int W, long long row_bytes, long long image_bytes, Groups args, int n_groups,
            const unsigned char *__restrict__ strings, int tiles_x, int tiles_y) {
    __shared__ tsod_draw_group sg[kMaxG];
    __shared__ long long s_first[kMaxG + 1];             // first stream position of each group within a phase
    __shared__ Item list[kCap];
    __shared__ unsigned char font[128][8];
    __shared__ int wave_hits[kThreads / 64];

    const int tid = threadIdx.x;
    const int per_image = tiles_x * tiles_y;             // (the host refuses more than 2^31 - 1 tiles in all)
    const int b = (int)(blockIdx.x / (unsigned)per_image);
    const int tile = (int)(blockIdx.x % (unsigned)per_image);
    const int tx0 = (tile % tiles_x) * kTileW, ty0 = (tile / tiles_x) * kTileH;
    const int tx1 = W - 1 - tx0 < kTileW - 1 ? W - 1 : tx0 + kTileW - 1;   // the tile's last column and row, inside the image
    const int ty1 = H - 1 - ty0 < kTileH - 1 ? H - 1 : ty0 + kTileH - 1;

    // the groups travel by value; constant indices keep them out of scratch
    if (tid == 0) sg[0] = args.g[0];
    if (tid == 1) sg[1] = args.g[1];
    if (tid == 2) sg[2] = args.g[2];
    if (tid == 3) sg[3] = args.g[3];
    __syncthreads();
    if (tid == 0) {
        long long at = 0;
        for (int g = 0; g < kMaxG; ++g) {
            s_first[g] = at;
            if (g < n_groups) {
                const tsod_draw_group &G = sg[g];
                int n = G.keep ? G.n_kept[b] : (G.counts ? G.counts[b] : G.R);
                n = n < 0 ? 0 : (n > G.R ? G.R : n);
                at += n;
            }
        }
        s_first[kMaxG] = at;
    }
    __syncthreads();
    const long long N = s_first[kMaxG];
    if (N == 0) return;

    const int lx = tid & (kTileW - 1), ly = tid / kTileW;
    const int px = tx0 + lx;
    unsigned pr[kRows], pg[kRows], pb[kRows];
    unsigned touched = 0;
    unsigned char *const img = images + (long long)b * image_bytes;
    bool font_ready = false;
    int count = 0;                                       // entries in the list

    auto paint = [&](int n) {
        if (!font_ready) {                               // workgroup-uniform
            if (tid < 128) {
#pragma unroll
                for (int r = 0; r < 7; ++r) font[tid][r] = 0x1f;
                font[tid][7] = 0;
            }
            __syncthreads();
            if (tid < kGlyphs) {
                const Glyph gl = d_glyphs[tid];
                if (gl.ch < 128) {
#pragma unroll
                    for (int r = 0; r < 7; ++r) font[gl.ch][r] = gl.rows[r];
                }
            }
            __syncthreads();
            font_ready = true;
        }
        if (px > tx1) return;
#pragma unroll 1
        for (int e = 0; e < n; ++e) {
            const Item &it = list[e];
            const int x0 = it.x0, y0 = it.y0, x1 = it.x1, y1 = it.y1;
            if (px < x0 || px > x1) continue;
            const int kind = it.kind, s = it.s;
            const unsigned fill = it.fill;
            const unsigned a = fill >> 24;
            // what depends on the column alone: the ring's vertical edges, the character column and the glyph column
            bool xedge = false;
            unsigned col = 0, gx = 5;                    // gx = 5: between two characters or left of the text
            if (kind == 0) {
                xedge = px - x0 < s || x1 - px < s;
            } else {
                const int u = px - x0 - it.pad;
                if (u >= 0) {
                    if (s == 1) {                        // the usual scale: constant divisors
                        col = (unsigned)u / 6u, gx = (unsigned)u - col * 6u;
                    } else {
                        const unsigned cw = 6u * (unsigned)s;
                        col = (unsigned)u / cw, gx = ((unsigned)u - col * cw) / (unsigned)s;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const int py = ty0 + ly + k * (kThreads / kTileW);
                if (py > ty1 || py < y0 || py > y1) continue;
                bool glyph = false;
                if (kind == 0) {
                    if (!(xedge || py - y0 < s || y1 - py < s)) continue;
                } else {
                    const int v = py - y0 - it.pad;
                    if (v >= 0 && gx < 5u) {
                        unsigned line, gy;
                        if (s == 1) {
                            line = (unsigned)v >> 3, gy = (unsigned)v & 7u;
                        } else {
                            const unsigned chh = 8u * (unsigned)s;
                            line = (unsigned)v / chh, gy = ((unsigned)v - line * chh) / (unsigned)s;
                        }
                        if (line < 2u && gy < 7u && (int)col < it.len[line]) {
                            const unsigned ch = it.text[line][col];
                            const unsigned bits = ch < 128u ? font[ch][gy] : 0x1fu;
                            glyph = (bits >> (4u - gx)) & 1u;
                        }
                    }
                }
                if (a == 0u && !glyph) continue;
                if (!(touched & (1u << k))) {
                    const unsigned char *p = img + (long long)py * row_bytes + (long long)px * 3;
                    pr[k] = p[0], pg[k] = p[1], pb[k] = p[2];
                    touched |= 1u << k;
                }
                if (glyph) {
                    pr[k] = it.ink & 0xffu, pg[k] = (it.ink >> 8) & 0xffu, pb[k] = (it.ink >> 16) & 0xffu;
                } else {
                    pr[k] = blend1(a, fill & 0xffu, pr[k]);
                    pg[k] = blend1(a, (fill >> 8) & 0xffu, pg[k]);
                    pb[k] = blend1(a, (fill >> 16) & 0xffu, pb[k]);
                }
            }
        }
    };

#pragma unroll 1
    for (long long q0 = 0;; q0 += kThreads) {
        const bool last = q0 >= 2 * N;                   // one read past the stream's end: no candidates, paints what is left
        const long long q = q0 + tid;
        Cand c;
        bool hit = false;
        c.kind = 0, c.x0 = c.y0 = c.x1 = c.y1 = 0, c.g = 0, c.len1 = 0, c.index = 0, c.score = 0.f;
        if (q < 2 * N) {
            c.kind = q >= N ? 1 : 0;
            const long long j = c.kind ? q - N : q;
            c.g = (j >= s_first[1] ? 1 : 0) + (j >= s_first[2] ? 1 : 0) + (j >= s_first[3] ? 1 : 0);   // (read here, not held in SGPRs)
            const long long i = j - s_first[c.g];
            const tsod_draw_group &G = sg[c.g];
            const long long R = G.R;
            const long long r = G.keep ? (long long)G.keep[(long long)b * R + i] : i;
            int X1, Y1, X2, Y2;
            if (r >= 0 && r < R && !(c.kind == 1 && (G.tag == TSOD_DRAW_TAG_NONE || (!G.labels && G.pitch < 6)))) {
                const float *bx = G.boxes + ((long long)b * R + r) * G.pitch;
                if (to_pixel(G.sx, bx[0], X1) && to_pixel(G.sy, bx[1], Y1) && to_pixel(G.sx, bx[2], X2) && to_pixel(G.sy, bx[3], Y2) &&
                    X2 >= X1 && Y2 >= Y1) {
                    if (c.kind == 0) {
                        const int t = G.thickness;
                        c.x0 = X1, c.y0 = Y1, c.x1 = X2, c.y1 = Y2;
                        hit = G.color[3] != 0 && X1 <= tx1 && X2 >= tx0 && Y1 <= ty1 && Y2 >= ty0;
                        // a tile wholly inside the ring's hole meets no outline pixel
                        if (hit && tx0 - X1 >= t && X2 - tx1 >= t && ty0 - Y1 >= t && Y2 - ty1 >= t) hit = false;
                    } else {
                        c.index = (G.labels ? (long long)G.labels[(long long)b * R + r] : (long long)class_of(bx[5])) + G.label_offset;
                        if (G.pitch >= 6) c.score = bx[4];
                        if (c.index >= 0 && c.index < (long long)G.string_count)
                            c.len1 = string_length(reinterpret_cast<const unsigned *>(strings + (G.string_first + c.index) * kStr));
                        else
                            c.len1 = 6 + (c.index < 0 ? 1 : 0) +
                                     decimal_digits(c.index < 0 ? 0ull - (unsigned long long)c.index : (unsigned long long)c.index);
                        const int lines = G.score_line ? 2 : 1;
                        const int cols = G.score_line && c.len1 < 11 ? 11 : c.len1;
                        const int w = cols * 6 * G.font_scale + 2 * G.padding, h = lines * 8 * G.font_scale + 2 * G.padding;
                        int left = X1, top;
                        if (G.tag == TSOD_DRAW_TAG_ABOVE) {
                            top = Y1 - h;
                            if (top < 0) top = Y1;
                        } else {
                            top = Y2 + 1;
                            if (top + h > H) top = Y2 - h + 1;
                        }
                        if (left > 0 && left + w > W) left = W - w > 0 ? W - w : 0;
                        c.x0 = left, c.y0 = top, c.x1 = left + w - 1, c.y1 = top + h - 1;
                        hit = w > 0 && c.x0 <= tx1 && c.x1 >= tx0 && c.y0 <= ty1 && c.y1 >= ty0;
                    }
                }
            }
        }
        // ordered append: position = entries so far + hits of lower threads
        const unsigned long long ballot = __ballot(hit);
        const int wave = tid >> 6, lane = tid & 63;
        if (lane == 0) wave_hits[wave] = __popcll(ballot);
        __syncthreads();
        int before = __popcll(ballot & ((1ull << lane) - 1ull)), hits = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int n = wave_hits[w];
            before += w < wave ? n : 0;
            hits += n;
        }
        const int pos = count + before, total = count + hits;
        int lo = 0;
        while (true) {                                   // workgroup-uniform: total and lo are
            if (hit && pos >= lo && pos < lo + kCap) write_item(list[pos - lo], c, sg[c.g], strings);
            __syncthreads();
            const int left = total - lo;
            if (left <= kCap && !last) break;            // room for more: read on
            if (left > 0) paint(left < kCap ? left : kCap);      // (the one call site: the walk is not duplicated)
            if (last) break;                             // (left <= kCap here: the last read adds nothing)
            __syncthreads();
            lo += kCap;
        }
        if (last) break;
        count = total - lo;
    }

#pragma unroll
    for (int k = 0; k < kRows; ++k)
        if (touched & (1u << k)) {
            const int py = ty0 + ly + k * (kThreads / kTileW);
            unsigned char *p = img + (long long)py * row_bytes + (long long)px * 3;
            p[0] = (unsigned char)pr[k], p[1] = (unsigned char)pg[k], p[2] = (unsigned char)pb[k];
        }
}

}  // namespace

extern "C" int tsod_draw_groups_u8(uint8_t *images, int32_t B, int32_t H, int32_t W, int64_t row_bytes, int64_t image_bytes,
                                   const tsod_draw_group *groups, int32_t n_groups, const uint8_t *strings, int32_t n_strings,
                                   tsod_stream_t stream) {
    TSOD_REQUIRE(images && B > 0 && H > 0 && W > 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(row_bytes >= (int64_t)W * 3, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(row_bytes <= INT64_MAX / H && image_bytes >= (int64_t)H * row_bytes, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_groups >= 0 && n_groups <= TSOD_DRAW_MAX_GROUPS && (groups || n_groups == 0), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_strings >= 0 && (strings || n_strings == 0), TSOD_ERR_INVALID_ARG);
    Groups args = {};
    bool any = false;
    for (int g = 0; g < n_groups; ++g) {
        const tsod_draw_group &G = groups[g];
        TSOD_REQUIRE(G.R >= 0 && (G.boxes || G.R == 0) && (G.pitch == 4 || G.pitch == 6), TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE((G.keep == nullptr) == (G.n_kept == nullptr) && !(G.keep && G.counts), TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(G.thickness >= 1 && G.font_scale >= 1 && G.padding >= 0, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(G.tag >= TSOD_DRAW_TAG_NONE && G.tag <= TSOD_DRAW_TAG_BELOW, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE((G.score_line == 0 || G.score_line == 1) && !(G.score_line && G.pitch == 4), TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(G.string_first >= 0 && G.string_count >= 0 && (int64_t)G.string_first + G.string_count <= n_strings,
                     TSOD_ERR_INVALID_ARG);
        args.g[g] = G;
        any = any || G.R > 0;
    }
    TSOD_REQUIRE((int64_t)H * W <= INT32_MAX, TSOD_ERR_UNSUPPORTED);
    for (int g = 0; g < n_groups; ++g) {
        const tsod_draw_group &G = groups[g];
        TSOD_REQUIRE((int64_t)B * G.R <= INT32_MAX, TSOD_ERR_UNSUPPORTED);
        TSOD_REQUIRE(G.thickness <= TSOD_DRAW_MAX_STYLE && G.font_scale <= TSOD_DRAW_MAX_STYLE && G.padding <= TSOD_DRAW_MAX_STYLE,
                     TSOD_ERR_UNSUPPORTED);
    }
    TSOD_REQUIRE((reinterpret_cast<uintptr_t>(strings) & 3u) == 0, TSOD_ERR_ALIGNMENT);
    const int64_t tiles_x = tsod_cdiv(W, kTileW), tiles_y = tsod_cdiv(H, kTileH);
    TSOD_REQUIRE(tiles_x * tiles_y * B <= INT32_MAX, TSOD_ERR_UNSUPPORTED);
    if (!any) return TSOD_OK;
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)(tiles_x * tiles_y * B)), dim3(kThreads), 0, tsod_stream(stream), images, H, W,
                       (long long)row_bytes, (long long)image_bytes, args, n_groups, strings, (int)tiles_x, (int)tiles_y);
    return tsod_launch_status();
}

extern "C" int tsod_draw_font5x7(uint8_t out[128][7]) {
    TSOD_REQUIRE(out, TSOD_ERR_INVALID_ARG);
    for (int c = 0; c < 128; ++c)
        for (int r = 0; r < 7; ++r) out[c][r] = 0x1f;
    for (int k = 0; k < kGlyphs; ++k)
        for (int r = 0; r < 7; ++r) out[h_glyphs[k].ch][r] = h_glyphs[k].rows[r];
    return TSOD_OK;
}
