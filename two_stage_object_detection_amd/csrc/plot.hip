// plot.hip -- training curves: the EMA of the reference's train/train.py:147-160 and the pixels of its
// utils/draw.py:plot_training_metrics figure.  Every rule is stated once, in include/tsod.h ("training curves"); this file is
// their per-thread form.
//
//   ema_scan_kernel      K1: one wave per row.  64 samples in, every lane its product a x[i]; the chain c = p_k + b c runs
//                        over values the whole wave holds (p_k by lane broadcast); step k goes to word k of an LDS row,
//                        from which every lane takes its own: 64 samples out.  Three VALU operations and one LDS write
//                        per step (a per-lane select instead keeps 64 lane masks live and spills them).
//   limits_partial_kernel, limits_final_kernel   K2: finite min / max per workgroup, then over the workgroups, then the rule.
//   plot_series_kernel   K3: one workgroup per kCols columns of the rectangle; a row bitmask in LDS per series, set with
//                        integer atomicOr by the threads that walk the samples near the block, blended after a barrier.
//   plot_items_kernel    K4: one workgroup per 64x4 tile; the items are tested 256 at a time, the hits kept as wave ballots
//                        and walked in item order by every thread for its one pixel.
// Compiled with -ffp-contract=off: every product and sum below is one f32 rounding, as the header says.
#include <float.h>

#include "tsod_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCols = TSOD_PLOT_BLOCK_COLUMNS;
constexpr int kMaxWords = TSOD_PLOT_MAX_HEIGHT / 32;
constexpr int kMaxS = TSOD_PLOT_MAX_SERIES;
constexpr int kStr = TSOD_PLOT_STRING_BYTES;
constexpr int kLimitBlocks = TSOD_PLOT_LIMITS_WORKSPACE_BYTES / 8;      // one (min, max) pair per workgroup
constexpr int kItemTileW = 64, kItemTileH = kThreads / kItemTileW;
constexpr int kNumberChars = 12;                                         // '-' + 6 digits + '.' + 3 digits, rounded up
static_assert(kCols == 32, "the blend loop splits an index into (column, word) with & 31 and >> 5");

// the font of csrc/font5x7.h, unpacked at compile time: rows[c][r] = row r of byte c's glyph, 0x1f for bytes without one
struct Glyph {
    unsigned char ch, rows[7];
};
struct Font {
    unsigned char rows[128][8];
};
#define TSOD_GLYPH(c, r0, r1, r2, r3, r4, r5, r6) {(unsigned char)(c), {r0, r1, r2, r3, r4, r5, r6}},
constexpr Glyph kGlyphs[] = {
#include "font5x7.h"
};
#undef TSOD_GLYPH
constexpr Font make_font() {
    Font f{};
    for (int c = 0; c < 128; ++c)
        for (int r = 0; r < 7; ++r) f.rows[c][r] = 0x1f;
    for (const Glyph &g : kGlyphs)
        if (g.ch < 128)
            for (int r = 0; r < 7; ++r) f.rows[g.ch][r] = g.rows[r];
    return f;
}
__constant__ Font d_font = make_font();

__device__ __forceinline__ unsigned blend1(unsigned a, unsigned c, unsigned src) { return (a * c + (255u - a) * src + 127u) / 255u; }

__device__ __forceinline__ long long floor_div(long long num, long long den) {      // den > 0
    long long q = num / den;
    if (num % den != 0 && num < 0) --q;
    return q;
}

// ---------------------------------------------------------------------------------------------------------------- K1
__global__ void __launch_bounds__(64)
ema_scan_kernel(const float *x, long long n, long long x_pitch, float a, float b, float *out, long long out_pitch) {
    __shared__ float steps[64];
    const int lane = threadIdx.x;
    const float *xr = x + (long long)blockIdx.x * x_pitch;
    float *outr = out + (long long)blockIdx.x * out_pitch;
    float carry = 0.f;                                   // out[i - 1], the same in every lane
#pragma unroll 1
    for (long long base = 0; base < n; base += 64) {
        const long long i = base + lane;
        const float xv = i < n ? xr[i] : 0.f;
        const float p = a * xv;
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            const float pk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), k));
            const float t = b * carry;
            carry = pk + t;
            if (k == 0 && base == 0) carry = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xv), 0));
            steps[k] = carry;                            // (every lane writes the same value to the same word)
        }
        if (i < n) outr[i] = steps[lane];                // (one wave: its LDS operations complete in order)
    }
}

// ---------------------------------------------------------------------------------------------------------------- K2
struct Series4 {
    const float *y[kMaxS];
    long long n[kMaxS];
};

__device__ __forceinline__ void block_min_max(float &mn, float &mx, float (*scr)[2], int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((tid & 63) == 0) scr[tid >> 6][0] = mn, scr[tid >> 6][1] = mx;
    __syncthreads();
    mn = fminf(fminf(scr[0][0], scr[1][0]), fminf(scr[2][0], scr[3][0]));
    mx = fmaxf(fmaxf(scr[0][1], scr[1][1]), fmaxf(scr[2][1], scr[3][1]));
}

__global__ void __launch_bounds__(kThreads) limits_partial_kernel(Series4 s, float *partials) {
    __shared__ float scr[kThreads / 64][2];
    float mn = INFINITY, mx = -INFINITY;
    const long long first = (long long)blockIdx.x * kThreads + threadIdx.x, step = (long long)gridDim.x * kThreads;
#pragma unroll
    for (int k = 0; k < kMaxS; ++k) {
        const float *y = s.y[k];
        const long long n = s.n[k];
#pragma unroll 1
        for (long long i = first; i < n; i += step) {
            const float v = y[i];
            if (isfinite(v)) mn = fminf(mn, v), mx = fmaxf(mx, v);
        }
    }
    block_min_max(mn, mx, scr, threadIdx.x);
    if (threadIdx.x == 0) partials[2 * blockIdx.x] = mn, partials[2 * blockIdx.x + 1] = mx;
}

__global__ void __launch_bounds__(kThreads) limits_final_kernel(const float *partials, int n_partials, float *limits) {
    __shared__ float scr[kThreads / 64][2];
    float m = INFINITY, M = -INFINITY;
    if ((int)threadIdx.x < n_partials) m = partials[2 * threadIdx.x], M = partials[2 * threadIdx.x + 1];
    block_min_max(m, M, scr, threadIdx.x);
    if (threadIdx.x != 0) return;
    float lo, hi;
    if (m > M) {                                         // no finite sample
        lo = 0.f, hi = 1.f;
    } else if (M == m) {
        lo = m - 0.5f, hi = m + 0.5f;
    } else {
        const float hm = 0.5f * m;
        const float hM = 0.5f * M;
        const float half = hM - hm;
        const float pad = 0.1f * half;
        lo = m - pad, hi = M + pad;
    }
    limits[0] = fminf(fmaxf(lo, -FLT_MAX), FLT_MAX);
    limits[1] = fminf(fmaxf(hi, -FLT_MAX), FLT_MAX);
}
static_assert(kLimitBlocks <= kThreads, "the final kernel reads one partial pair per thread");

// ---------------------------------------------------------------------------------------------------------------- K3
struct SeriesArgs {
    tsod_plot_series s[kMaxS];
};

struct Block {
    unsigned *mask;
    int words, bc0, bc1, py0, ph;
};

// rows ra .. rb (image rows) of the block's column lc
__device__ __forceinline__ void set_range(const Block &B, int lc, long long ra, long long rb) {
    ra -= B.py0, rb -= B.py0;
    if (ra < 0) ra = 0;
    if (rb > B.ph - 1) rb = B.ph - 1;
    if (ra > rb) return;
    const int w0 = (int)ra >> 5, w1 = (int)rb >> 5;
    for (int w = w0; w <= w1; ++w) {
        unsigned bits = 0xffffffffu;
        if (w == w0) bits &= 0xffffffffu << ((int)ra & 31);
        if (w == w1) bits &= 0xffffffffu >> (31 - ((int)rb & 31));
        atomicOr(&B.mask[lc * B.words + w], bits);
    }
}

// skeleton rows ra <= rb of skeleton column sc, dilated to width w
__device__ __forceinline__ void cover_line(const Block &B, int w, long long sc, long long ra, long long rb) {
    const int a = w / 2;
    for (int k = 0; k < w; ++k) {
        const long long cc = sc - a + k;
        if (cc >= B.bc0 && cc <= B.bc1) set_range(B, (int)(cc - B.bc0), ra - a, rb - a + w - 1);
    }
}

__device__ __forceinline__ void cover_marker(const Block &B, int marker, int k, long long c, long long r) {
    for (int u = -k; u <= k; ++u) {
        const long long cc = c + u;
        if (cc < B.bc0 || cc > B.bc1) continue;
        const int au = u < 0 ? -u : u;
        int v0 = -k, v1 = k;
        if (marker == TSOD_PLOT_MARKER_CIRCLE) {
            int v = k;
            while (v >= 0 && au * au + v * v > k * k + k) --v;
            if (v < 0) continue;
            v0 = -v, v1 = v;
        } else if (marker == TSOD_PLOT_MARKER_TRIANGLE) {
            v0 = 2 * au - k;
            if (v0 > v1) continue;
        }
        set_range(B, (int)(cc - B.bc0), r + v0, r + v1);
    }
}

__global__ void __launch_bounds__(kThreads)
plot_series_kernel(unsigned char *__restrict__ image, long long row_bytes, int px0, int py0, int pw, int ph, SeriesArgs args,
                   int n_series, long long x_lo, long long x_hi, const float *__restrict__ limits) {
    __shared__ unsigned mask[kCols * kMaxWords];
    __shared__ tsod_plot_series ss[kMaxS];
    const int tid = threadIdx.x;
    // the series travel by value; constant indices keep them out of scratch
    if (tid == 0) ss[0] = args.s[0];
    if (tid == 1) ss[1] = args.s[1];
    if (tid == 2) ss[2] = args.s[2];
    if (tid == 3) ss[3] = args.s[3];
    Block B;
    B.mask = mask;
    B.words = (ph + 31) >> 5;
    B.bc0 = px0 + (int)blockIdx.x * kCols;
    B.bc1 = B.bc0 + kCols - 1 < px0 + pw - 1 ? B.bc0 + kCols - 1 : px0 + pw - 1;
    B.py0 = py0, B.ph = ph;
    const float lo = limits[0], hi = limits[1];
    const float range = hi - lo;
    const float s = (float)(ph - 1) / range;
    const float top = (float)(ph - 1);
    const long long span = x_hi - x_lo;
    __syncthreads();

#pragma unroll 1
    for (int q = 0; q < n_series; ++q) {
        const tsod_plot_series S = ss[q];
        const long long n = S.n;
        if (n <= 0 || S.color[3] == 0) continue;         // (workgroup-uniform)
        for (int idx = tid; idx < kCols * B.words; idx += kThreads) mask[idx] = 0u;
        __syncthreads();

        auto col = [&](long long i) -> long long {
            if (span == 0) return (long long)px0;
            return px0 + (((long long)S.x_first + i * (long long)S.x_step - x_lo) * (long long)(pw - 1)) / span;
        };
        auto row = [&](float v) -> long long {
            const float d = v - lo;
            const float t = d * s;
            return (long long)py0 + (ph - 1) - (long long)(int)rintf(fminf(fmaxf(t, 0.f), top));
        };
        auto first_at_least = [&](long long c) -> long long {      // the first sample whose column is >= c (n: none)
            long long a = 0, b = n;
            while (a < b) {
                const long long mid = a + (b - a) / 2;
                if (col(mid) >= c) b = mid; else a = mid + 1;
            }
            return a;
        };
        const int w = S.width, mk = S.marker, k = S.marker_size / 2;
        const int halo = w > S.marker_size ? w : S.marker_size;
        long long i0 = first_at_least((long long)B.bc0 - halo) - 1;
        long long i1 = first_at_least((long long)B.bc1 + halo + 1);
        if (i0 < 0) i0 = 0;
        if (i1 > n - 1) i1 = n - 1;
#pragma unroll 1
        for (long long i = i0 + tid; i <= i1; i += kThreads) {
            const float v0 = S.y[i];
            if (!isfinite(v0)) continue;
            const long long c0 = col(i), r0 = row(v0);
            if (w >= 1) cover_line(B, w, c0, r0, r0);
            if (mk != TSOD_PLOT_MARKER_NONE) cover_marker(B, mk, k, c0, r0);
            if (w < 1 || i >= i1) continue;
            const float v1 = S.y[i + 1];
            if (!isfinite(v1)) continue;
            const long long c1 = col(i + 1), r1 = row(v1);
            if (c0 == c1) {
                cover_line(B, w, c0, r0 < r1 ? r0 : r1, r0 < r1 ? r1 : r0);
                continue;
            }
            const long long dx = c1 - c0, dy = r1 - r0;
            const int a = w / 2;
            long long sc0 = (long long)B.bc0 - (w - 1) + a, sc1 = (long long)B.bc1 + a;      // skeleton columns that reach the block
            if (sc0 < c0) sc0 = c0;
            if (sc1 > c1) sc1 = c1;
            for (long long sc = sc0; sc <= sc1; ++sc) {
                const long long ra = sc == c0 ? r0 : r0 + floor_div((2 * (sc - c0) - 1) * dy + dx, 2 * dx);
                const long long rb = sc == c1 ? r1 : r0 + floor_div((2 * (sc + 1 - c0) - 1) * dy + dx, 2 * dx);
                cover_line(B, w, sc, ra < rb ? ra : rb, ra < rb ? rb : ra);
            }
        }
        __syncthreads();

        const unsigned a = S.color[3], cr = S.color[0], cg = S.color[1], cb = S.color[2];
        for (int idx = tid; idx < kCols * B.words; idx += kThreads) {
            const int lc = idx & 31, wj = idx >> 5;
            if (B.bc0 + lc > B.bc1) continue;
            unsigned m = mask[lc * B.words + wj];
            while (m) {
                const int bit = __ffs((int)m) - 1;
                m &= m - 1u;
                unsigned char *p = image + (long long)(py0 + wj * 32 + bit) * row_bytes + (long long)(B.bc0 + lc) * 3;
                p[0] = (unsigned char)blend1(a, cr, p[0]);
                p[1] = (unsigned char)blend1(a, cg, p[1]);
                p[2] = (unsigned char)blend1(a, cb, p[2]);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- K4
struct Number {
    int len, sign, nd;
    unsigned ip, fr;
    bool bad;
};

__device__ __forceinline__ Number format_number(const float *limits, int tick, int ticks) {
    const float lo = limits[0], hi = limits[1];
    const float d = hi - lo;
    const float t = (float)tick * d;
    const float q = t / (float)ticks;
    const float v = lo + q;
    const float p = fabsf(v) * 1000.f;
    Number N;
    N.bad = !(p < 1e9f);
    N.len = 5, N.sign = 0, N.nd = 1, N.ip = 0u, N.fr = 0u;
    if (N.bad) return N;
    const unsigned m = (unsigned)(int)rintf(p);
    N.ip = m / 1000u, N.fr = m % 1000u;
    N.sign = v < 0.f && m > 0u ? 1 : 0;
    N.nd = 1;
    for (unsigned r = N.ip / 10u; r != 0u; r /= 10u) ++N.nd;
    N.len = N.sign + N.nd + 4;
    return N;
}

__device__ __forceinline__ unsigned number_char(const Number &N, int j) {
    if (N.bad) return j == 1 ? '.' : '-';
    if (N.sign && j == 0) return '-';
    const int k = j - N.sign;
    if (k < N.nd) {
        unsigned v = N.ip;
        for (int e = N.nd - 1 - k; e > 0; --e) v /= 10u;
        return '0' + v % 10u;
    }
    if (k == N.nd) return '.';
    const int f = k - N.nd - 1;
    return '0' + (f == 0 ? N.fr / 100u : f == 1 ? N.fr / 10u % 10u : N.fr % 10u);
}

__global__ void __launch_bounds__(kThreads)
plot_items_kernel(unsigned char *__restrict__ image, int H, int W, long long row_bytes, const tsod_plot_item *__restrict__ items,
                  int n_items, int tiles_x) {
    __shared__ unsigned long long hits[kThreads / 64];
    const int tid = threadIdx.x;
    const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kItemTileW, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kItemTileH;
    const int tx1 = W - 1 - tx0 < kItemTileW - 1 ? W - 1 : tx0 + kItemTileW - 1;
    const int ty1 = H - 1 - ty0 < kItemTileH - 1 ? H - 1 : ty0 + kItemTileH - 1;
    const int px = tx0 + (tid & (kItemTileW - 1)), py = ty0 + tid / kItemTileW;
    const bool inside = px <= tx1 && py <= ty1;
    unsigned char *const p = image + (long long)py * row_bytes + (long long)px * 3;
    unsigned pr = 0, pg = 0, pb = 0;
    bool touched = false;

#pragma unroll 1
    for (int q0 = 0; q0 < n_items; q0 += kThreads) {
        bool hit = false;
        if (q0 + tid < n_items) {
            const tsod_plot_item &it = items[q0 + tid];
            long long x0 = 0, x1 = -1, y0 = 0, y1 = -1;                 // the item's bounding box (a superset of its pixels)
            if (it.kind == TSOD_PLOT_ITEM_RECT && it.w >= 1 && it.h >= 1) {
                x0 = it.x, x1 = (long long)it.x + it.w - 1, y0 = it.y, y1 = (long long)it.y + it.h - 1;
            } else if ((it.kind == TSOD_PLOT_ITEM_TEXT || it.kind == TSOD_PLOT_ITEM_NUMBER) && it.scale >= 1) {
                const long long reach = 6ll * it.scale * (it.kind == TSOD_PLOT_ITEM_TEXT ? (long long)kStr : (long long)kNumberChars);
                x0 = it.x - reach, x1 = it.x + reach, y0 = it.y, y1 = it.y + 7ll * it.scale - 1;
            }
            hit = it.color[3] != 0 && x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0;
        }
        const unsigned long long ballot = __ballot(hit);
        if ((tid & 63) == 0) hits[tid >> 6] = ballot;
        __syncthreads();
#pragma unroll 1
        for (int wv = 0; wv < kThreads / 64; ++wv) {
            unsigned long long m = hits[wv];
#pragma unroll 1
            while (m) {                                  // (workgroup-uniform)
                const int e = q0 + wv * 64 + (__ffsll((long long)m) - 1);
                m &= m - 1ull;
                if (!inside) continue;
                const tsod_plot_item &it = items[e];
                const unsigned a = it.color[3];
                bool paint = false;
                if (it.kind == TSOD_PLOT_ITEM_RECT) {
                    const long long u = (long long)px - it.x, v = (long long)py - it.y;
                    paint = u >= 0 && u < it.w && v >= 0 && v < it.h && (it.dash_period <= 0 || v % it.dash_period < it.dash_on);
                } else {
                    const bool number = it.kind == TSOD_PLOT_ITEM_NUMBER;
                    Number N;
                    int len = it.len;
                    if (number) {
                        N = format_number(it.limits, it.tick, it.ticks);
                        len = N.len;
                    }
                    if (len < 0 || len > kStr) continue;
                    const long long s = it.scale, width = 6ll * s * len;
                    const long long left = it.align == 1 ? it.x - width : it.align == 2 ? it.x - width / 2 : (long long)it.x;
                    const long long u = (long long)px - left, v = (long long)py - it.y;
                    if (u < 0 || v < 0 || u >= width || v >= 7 * s) continue;
                    const long long cell = u / (6 * s);
                    const int gx = (int)((u - cell * 6 * s) / s), gy = (int)(v / s);
                    if (gx >= 5) continue;
                    const unsigned ch = number ? number_char(N, (int)cell) : it.text[cell];
                    const unsigned bits = ch < 128u ? d_font.rows[ch][gy] : 0x1fu;
                    paint = (bits >> (4 - gx)) & 1u;
                }
                if (!paint) continue;
                if (!touched) {
                    pr = p[0], pg = p[1], pb = p[2];
                    touched = true;
                }
                pr = blend1(a, it.color[0], pr);
                pg = blend1(a, it.color[1], pg);
                pb = blend1(a, it.color[2], pb);
            }
        }
        __syncthreads();
    }
    if (touched) p[0] = (unsigned char)pr, p[1] = (unsigned char)pg, p[2] = (unsigned char)pb;
}

int check_image(const void *image, int32_t H, int32_t W, int64_t row_bytes) {
    TSOD_REQUIRE(image && H > 0 && W > 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(row_bytes >= (int64_t)W * 3 && row_bytes <= INT64_MAX / H, TSOD_ERR_INVALID_ARG);
    return TSOD_OK;
}

}  // namespace

extern "C" int tsod_ema_scan_f32(const float *x, int32_t rows, int64_t n, int64_t x_pitch, float a, float b, float *out,
                                 int64_t out_pitch, tsod_stream_t stream) {
    TSOD_REQUIRE(rows >= 0 && n >= 0, TSOD_ERR_INVALID_ARG);
    if (rows == 0 || n == 0) return TSOD_OK;
    TSOD_REQUIRE(x && out && x_pitch >= n && out_pitch >= n, TSOD_ERR_INVALID_ARG);
    hipLaunchKernelGGL(ema_scan_kernel, dim3((unsigned)rows), dim3(64), 0, tsod_stream(stream), x, (long long)n, (long long)x_pitch, a,
                       b, out, (long long)out_pitch);
    return tsod_launch_status();
}

extern "C" int tsod_plot_limits_f32(const float *const *series, const int64_t *lengths, int32_t n_series, float *limits,
                                    void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(limits && n_series >= 0 && n_series <= kMaxS && ((series && lengths) || n_series == 0), TSOD_ERR_INVALID_ARG);
    Series4 s = {};
    int64_t longest = 0;
    for (int k = 0; k < n_series; ++k) {
        TSOD_REQUIRE(lengths[k] >= 0 && (series[k] || lengths[k] == 0), TSOD_ERR_INVALID_ARG);
        s.y[k] = series[k], s.n[k] = lengths[k];
        longest = lengths[k] > longest ? lengths[k] : longest;
    }
    TSOD_REQUIRE(workspace && workspace_bytes >= TSOD_PLOT_LIMITS_WORKSPACE_BYTES, TSOD_ERR_WORKSPACE);
    TSOD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, TSOD_ERR_ALIGNMENT);
    float *partials = static_cast<float *>(workspace);
    int blocks = 0;
    if (longest > 0) {
        const int64_t want = tsod_cdiv(longest, (int64_t)kThreads * 8);
        blocks = (int)(want < kLimitBlocks ? want : kLimitBlocks);
        hipLaunchKernelGGL(limits_partial_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, tsod_stream(stream), s, partials);
    }
    hipLaunchKernelGGL(limits_final_kernel, dim3(1), dim3(kThreads), 0, tsod_stream(stream), partials, blocks, limits);
    return tsod_launch_status();
}

extern "C" int tsod_plot_series_u8(uint8_t *image, int32_t H, int32_t W, int64_t row_bytes, int32_t px0, int32_t py0, int32_t pw,
                                   int32_t ph, const tsod_plot_series *series, int32_t n_series, int64_t x_lo, int64_t x_hi,
                                   const float *limits, tsod_stream_t stream) {
    const int rc = check_image(image, H, W, row_bytes);
    if (rc != TSOD_OK) return rc;
    TSOD_REQUIRE(limits && pw > 0 && ph > 0 && px0 >= 0 && py0 >= 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((int64_t)px0 + pw <= W && (int64_t)py0 + ph <= H && x_hi >= x_lo, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_series >= 0 && n_series <= kMaxS && (series || n_series == 0), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((int64_t)H * W <= INT32_MAX && ph <= TSOD_PLOT_MAX_HEIGHT, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(x_lo >= -(int64_t)INT32_MAX && x_hi <= INT32_MAX, TSOD_ERR_UNSUPPORTED);
    SeriesArgs args = {};
    bool any = false;
    for (int k = 0; k < n_series; ++k) {
        const tsod_plot_series &S = series[k];
        TSOD_REQUIRE(S.n >= 0 && (S.y || S.n == 0) && S.x_step >= 1, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(S.n == 0 || (S.x_first >= x_lo && (int64_t)S.x_first + (int64_t)(S.n - 1) * S.x_step <= x_hi), TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(S.width >= 0 && S.width <= TSOD_PLOT_MAX_WIDTH, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(S.marker >= TSOD_PLOT_MARKER_NONE && S.marker <= TSOD_PLOT_MARKER_TRIANGLE, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(S.marker_size >= 1 && S.marker_size <= TSOD_PLOT_MAX_WIDTH && (S.marker_size & 1), TSOD_ERR_INVALID_ARG);
        args.s[k] = S;
        any = any || S.n > 0;
    }
    if (!any) return TSOD_OK;
    hipLaunchKernelGGL(plot_series_kernel, dim3((unsigned)tsod_cdiv(pw, kCols)), dim3(kThreads), 0, tsod_stream(stream), image,
                       (long long)row_bytes, px0, py0, pw, ph, args, n_series, (long long)x_lo, (long long)x_hi, limits);
    return tsod_launch_status();
}

extern "C" int tsod_plot_items_u8(uint8_t *image, int32_t H, int32_t W, int64_t row_bytes, const tsod_plot_item *items,
                                  int32_t n_items, tsod_stream_t stream) {
    const int rc = check_image(image, H, W, row_bytes);
    if (rc != TSOD_OK) return rc;
    TSOD_REQUIRE(n_items >= 0 && (items || n_items == 0), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((int64_t)H * W <= INT32_MAX, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE((reinterpret_cast<uintptr_t>(items) & 7u) == 0, TSOD_ERR_ALIGNMENT);
    if (n_items == 0) return TSOD_OK;
    const int64_t tiles_x = tsod_cdiv(W, kItemTileW), tiles_y = tsod_cdiv(H, kItemTileH);
    hipLaunchKernelGGL(plot_items_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(kThreads), 0, tsod_stream(stream), image, H, W,
                       (long long)row_bytes, items, n_items, (int)tiles_x);
    return tsod_launch_status();
}
