// dropout.hip -- active dropout on channel slices of an NHWC buffer: nn.Dropout(p) between HarDNet-85's
// last HarDBlock and its transition ConvLayer (reference models/hardnet.py:182-183) under .train().
//   tsod_dropout_segs_f32   dst = keep ? src * scale : 0 on the slices, the mask from Philox4x32-10 words (philox.h) of the
//                           element's LOGICAL index - independent of pitches, padding, slice placement, grid and chunking
//   tsod_dropout_key_set    the two key words of one forward into device memory, by a kernel (no copy, no synchronisation)
//   tsod_dropout_params     HOST: (thr, scale) of a probability      tsod_philox4x32_host   HOST: philox.h's function
//
// Memory-bound elementwise work with 40 integer multiplies per Philox call beside it.  A workgroup of 256 threads is
// (rows) x (quads across): the lanes of a wave walk consecutive channel quads of a pixel (16-byte loads and stores), the rows go
// round a capped grid.  A quad of four consecutive logical channels spans at most two counters, and one when its first element
// index is a multiple of 4 (always, where C and the slices' first logical channels are multiples of 4 - HarDNet-85's are): at
// most two Philox calls per quad.  A slice's last quad may be short (real width not a multiple of 4): its real lanes are loaded
// one by one - the pad lanes of src are never read - and the quad is stored whole, pad lanes as zeros.
#include <math.h>

#include "philox.h"
#include "tsod_internal.h"

namespace {

constexpr int kDropThreads = 256;
constexpr int kDropMaxBlocks = 4096;                     // the grid cap: 4096 x 256 threads, twice what the chip holds at once

struct DropTable {
    int32_t n, Q;                                        // slices; channel quads per pixel over all slices
    int32_t off[TSOD_DROPOUT_MAX_SEGMENTS];              // first channel in the pixel
    int32_t real[TSOD_DROPOUT_MAX_SEGMENTS];             // real width
    int32_t first[TSOD_DROPOUT_MAX_SEGMENTS];            // first logical channel
    int32_t q0[TSOD_DROPOUT_MAX_SEGMENTS];               // first quad (of the pixel's Q) of the slice
};

__device__ __forceinline__ uint32_t drop_pick(uint32_t lane, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return lane == 0 ? a : lane == 1 ? b : lane == 2 ? c : d;
}

__global__ __launch_bounds__(kDropThreads) void dropout_segs_kernel(const float *src, float *dst, long M, int src_pitch, int dst_pitch,
                                                                    DropTable T, int C, unsigned long long thr, float scale,
                                                                    const uint32_t *key, uint32_t ordinal, unsigned long long e0,
                                                                    int qx_log2) {   // (dst may be src: no __restrict__)
    const uint32_t k0 = key[0], k1 = key[1];
    const int qx = 1 << qx_log2, rows = kDropThreads >> qx_log2;
    const int tx = (int)threadIdx.x & (qx - 1), ty = (int)threadIdx.x >> qx_log2;
    for (long m = (long)blockIdx.x * rows + ty; m < M; m += (long)gridDim.x * rows) {
        const unsigned long long e_row = e0 + (unsigned long long)m * (unsigned long long)C;
        const float *s_row = src + m * src_pitch;
        float *d_row = dst + m * dst_pitch;
        for (int q = tx; q < T.Q; q += qx) {
            int off = T.off[0], real = T.real[0], first = T.first[0], qb = 0;
            for (int s = 1; s < T.n; ++s) {                      // (s is uniform: scalar loads, four selects per slice)
                const bool in = q >= T.q0[s];
                off = in ? T.off[s] : off;
                real = in ? T.real[s] : real;
                first = in ? T.first[s] : first;
                qb = in ? T.q0[s] : qb;
            }
            const int c = (q - qb) * 4;                          // first channel of the quad inside its slice
            const int nv = min(4, real - c);                     // real lanes of the quad (1..4)
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (nv == 4) {
                const float4 v = *reinterpret_cast<const float4 *>(s_row + off + c);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (i < nv) x[i] = s_row[off + c + i];
            }
            const unsigned long long e = e_row + (unsigned long long)(first + c);
            const unsigned long long ctr = e >> 2;
            const uint32_t lane = (uint32_t)e & 3u;
            const tsod_philox_words a = tsod_philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), ordinal, 0u, k0, k1);
            tsod_philox_words b = a;
            if (lane + (uint32_t)nv > 4u) {
                const unsigned long long ctr1 = ctr + 1ull;
                b = tsod_philox4x32_10((uint32_t)ctr1, (uint32_t)(ctr1 >> 32), ordinal, 0u, k0, k1);
            }
            const uint32_t w[4] = {drop_pick(lane, a.v[0], a.v[1], a.v[2], a.v[3]), drop_pick(lane, a.v[1], a.v[2], a.v[3], b.v[0]),
                                   drop_pick(lane, a.v[2], a.v[3], b.v[0], b.v[1]), drop_pick(lane, a.v[3], b.v[0], b.v[1], b.v[2])};
            float y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = (i < nv && (unsigned long long)w[i] >= thr) ? x[i] * scale : 0.f;
            *reinterpret_cast<float4 *>(d_row + off + c) = make_float4(y[0], y[1], y[2], y[3]);
        }
    }
}

__global__ void dropout_key_set_kernel(uint32_t *key, uint32_t lo, uint32_t hi) {
    if (threadIdx.x < 2) key[threadIdx.x] = threadIdx.x == 0 ? lo : hi;
}

inline int pad4(int c) { return (c + 3) / 4 * 4; }

}  // namespace

extern "C" void tsod_philox4x32_host(const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
    const tsod_philox_words w = tsod_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = w.v[i];
}

extern "C" int tsod_dropout_params(float p, uint64_t *thr, float *scale) {
    TSOD_REQUIRE(thr && scale, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(p >= 0.f && p <= 1.f, TSOD_ERR_INVALID_ARG);           // (a NaN fails both comparisons)
    *thr = (uint64_t)llround((double)p * 4294967296.0);
    *scale = p < 1.f ? (float)(1.0 / (1.0 - (double)p)) : 0.f;
    return TSOD_OK;
}

extern "C" int tsod_dropout_key_set(uint32_t *key, uint32_t lo, uint32_t hi, tsod_stream_t stream) {
    TSOD_REQUIRE(key, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((reinterpret_cast<uintptr_t>(key) & 3u) == 0, TSOD_ERR_ALIGNMENT);
    hipLaunchKernelGGL(dropout_key_set_kernel, dim3(1), dim3(64), 0, tsod_stream(stream), key, lo, hi);
    return tsod_launch_status();
}

extern "C" int tsod_dropout_segs_f32(const float *src, float *dst, int32_t N, int32_t H, int32_t W, int32_t src_pitch,
                                     int32_t dst_pitch, const tsod_dropout_seg *segs, int32_t n_segs, int32_t C, float p,
                                     const uint32_t *key, uint32_t ordinal, uint64_t e0, tsod_stream_t stream) {
    TSOD_REQUIRE(src && dst && segs && key, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && src_pitch > 0 && dst_pitch > 0 && n_segs > 0, TSOD_ERR_INVALID_ARG);
    uint64_t thr;
    float scale;
    TSOD_REQUIRE(tsod_dropout_params(p, &thr, &scale) == TSOD_OK, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_segs <= TSOD_DROPOUT_MAX_SEGMENTS, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(src_pitch % 4 == 0 && dst_pitch % 4 == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(src) && tsod_aligned16(dst) && (reinterpret_cast<uintptr_t>(key) & 3u) == 0, TSOD_ERR_ALIGNMENT);
    DropTable T;
    T.n = n_segs;
    T.Q = 0;
    for (int s = 0; s < TSOD_DROPOUT_MAX_SEGMENTS; ++s) T.off[s] = T.real[s] = T.first[s] = T.q0[s] = 0;
    for (int s = 0; s < n_segs; ++s) {
        const tsod_dropout_seg g = segs[s];
        TSOD_REQUIRE(g.off >= 0 && g.real >= 1 && g.first >= 0, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(g.off % 4 == 0, TSOD_ERR_ALIGNMENT);
        // the slice with its pad lanes fits both pitches; its logical channels lie inside [0, C)
        TSOD_REQUIRE((int64_t)g.off + pad4(g.real) <= src_pitch && (int64_t)g.off + pad4(g.real) <= dst_pitch, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE((int64_t)g.first + g.real <= C, TSOD_ERR_INVALID_ARG);
        for (int t = 0; t < s; ++t) {                            // no two slices share a logical channel or a lane of the pixel
            TSOD_REQUIRE(g.first + g.real <= segs[t].first || segs[t].first + segs[t].real <= g.first, TSOD_ERR_INVALID_ARG);
            TSOD_REQUIRE(g.off + pad4(g.real) <= segs[t].off || segs[t].off + pad4(segs[t].real) <= g.off, TSOD_ERR_INVALID_ARG);
        }
        T.off[s] = g.off;
        T.real[s] = g.real;
        T.first[s] = g.first;
        T.q0[s] = T.Q;
        T.Q += pad4(g.real) / 4;
    }
    const long M = (long)N * H * W;
    int qx_log2 = 0;
    while ((1 << qx_log2) < T.Q && qx_log2 < 6) ++qx_log2;       // quads across: the power of two that covers Q, at most a wave
    const int rows = kDropThreads >> qx_log2;
    const long blocks = tsod_cdiv(M, rows);
    hipLaunchKernelGGL(dropout_segs_kernel, dim3((unsigned)(blocks < kDropMaxBlocks ? blocks : kDropMaxBlocks)), dim3(kDropThreads), 0,
                       tsod_stream(stream), src, dst, M, (int)src_pitch, (int)dst_pitch, T, (int)C, (unsigned long long)thr, scale, key,
                       ordinal, (unsigned long long)e0, qx_log2);
    return tsod_launch_status();
}
