// resize_aa.h -- the antialiased bilinear resize of resize.hip and augment.hip, once: the tap loop, the output store, the
// 8 x 32 output tile with its LDS-staged source region, and one tiled and one flat kernel over a source policy.
//
//   out[oy][ox][c] = sum_j wy[oy][j] * (sum_i wx[ox][i] * px(y0 + j, x0 + i)[c]) * mul
//
// horizontal sums first, then vertical, every product and sum rounded to f32 on its own (-ffp-contract=off), the first term
// of a sum taken as it is.  A policy says what px is and how a tile's region gets into LDS:
//   static kLdsCap            the tiled form runs when region + weights fit it, else the flat form
//   static kPrologueDoubles   LDS doubles that prologue() wants (0: it does nothing)
//   C                         channels per source pixel, 1..4 (a member or a constant)
//   static region_bytes(C, cap_rows, cap_cols)   LDS bytes of a region of at most cap_rows x cap_cols source pixels
//   prologue(red)             once per workgroup, by every thread, before anything else (the mean of augment.hip)
//   stage(lds, g, cap_rows, cap_cols)            the region of tile g into LDS, by the whole workgroup
//   tile_px(lds, g, cap_rows, cap_cols, y, x)   source pixel (y, x) out of the staged region ...
//   src_px(y, x)              ... and straight from global memory (flat form): a callable c -> channel c as f32
#pragma once
#include "tsod_internal.h"
#include <math.h>

namespace {

// A kTY x kTX workgroup owns that many output pixels.  The region of a tile is [first[o0], first[oL] + count[oL]) per
// axis (both are non-decreasing in the output index).
constexpr int kTY = 8, kTX = 32, kThreads = kTY * kTX;

// read(j, i): the source pixel of tap row j, tap column i (c -> channel c; asked for c < C only)
template <class Reader>
__device__ __forceinline__ void aa_taps(float acc[4], int C, int ny, int nx, const float *wy, const float *wx, Reader read) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = 0.f;
    for (int j = 0; j < ny; ++j) {
        float h[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < nx; ++i) {
            const float w = wx[i];
            const auto px = read(j, i);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    const float v = px(c) * w;
                    h[c] = i == 0 ? v : h[c] + v;
                }
        }
        const float w = wy[j];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = h[c] * w;
            acc[c] = j == 0 ? v : acc[c] + v;
        }
    }
}

// acc * mul to out[oy][ox][0..C_out), channels C..C_out-1 zero
__device__ __forceinline__ void aa_store(const float acc[4], float mul, int C, int C_out, float *__restrict__ out, int oy,
                                         int ox, long stride_y, long stride_x, long stride_c) {
    float *o = out + oy * stride_y + ox * stride_x;
    if (stride_c == 1 && C_out == 4 && ((stride_x | stride_y) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
        // NHWC(4): one 16-byte store per pixel
        *reinterpret_cast<float4 *>(o) = make_float4(acc[0] * mul, C > 1 ? acc[1] * mul : 0.f, C > 2 ? acc[2] * mul : 0.f,
                                                     C > 3 ? acc[3] * mul : 0.f);
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < C_out) o[c * stride_c] = c < C ? acc[c] * mul : 0.f;
}

struct TileGeom {
    int oy0, ox0, ry0, rx0, rows, cols;      // first output pixel, first source pixel, extent of the region (within the cap)
};

__device__ inline TileGeom tile_geom(const int *yfirst, const int *ycount, const int *xfirst, const int *xcount, int OH,
                                     int OW, int cap_rows, int cap_cols) {
    const int tiles_x = (OW + kTX - 1) / kTX;
    TileGeom g;
    g.oy0 = (blockIdx.x / tiles_x) * kTY;
    g.ox0 = (blockIdx.x % tiles_x) * kTX;
    const int oyL = min(g.oy0 + kTY, OH) - 1, oxL = min(g.ox0 + kTX, OW) - 1;
    g.ry0 = yfirst[g.oy0];
    g.rx0 = xfirst[g.ox0];
    g.rows = min(yfirst[oyL] + ycount[oyL] - g.ry0, cap_rows);
    g.cols = min(xfirst[oxL] + xcount[oxL] - g.rx0, cap_cols);
    return g;
}

// the tile's weight rows go to LDS as well: the tap loop then touches no global memory at all
__device__ inline void stage_weights(float *s_wx, float *s_wy, const float *__restrict__ xwt, int xtaps,
                                     const float *__restrict__ ywt, int ytaps, int ox0, int oy0, int OW, int OH) {
    for (int t = threadIdx.x; t < kTX * xtaps; t += kThreads) {
        const int o = ox0 + t / xtaps;
        s_wx[t] = o < OW ? xwt[(long)o * xtaps + t % xtaps] : 0.f;
    }
    for (int t = threadIdx.x; t < kTY * ytaps; t += kThreads) {
        const int o = oy0 + t / ytaps;
        s_wy[t] = o < OH ? ywt[(long)o * ytaps + t % ytaps] : 0.f;
    }
}

// A region held as C f32 planes of cap_rows x cap_cols (the policies that convert or gather while they stage).
struct F32Planes {
    static constexpr size_t kLdsCap = 64 * 1024;
    __host__ __device__ static size_t region_bytes(int C, int cap_rows, int cap_cols) {
        return (size_t)C * cap_rows * cap_cols * sizeof(float);
    }
    __device__ static auto tile_px(const unsigned char *lds, const TileGeom &g, int cap_rows, int cap_cols, int y, int x) {
        const long plane = (long)cap_rows * cap_cols;
        const float *row = reinterpret_cast<const float *>(lds) + (long)min(y - g.ry0, cap_rows - 1) * cap_cols;
        const int col = min(x - g.rx0, cap_cols - 1);
        return [=](int c) { return row[c * plane + col]; };
    }
};

// Tiled form: the workgroup stages the source region its kTY x kTX output pixels touch into LDS (every source pixel is
// fetched from global memory once per tile instead of once per tap), then every thread runs the tap loop out of LDS.
template <class P>
__global__ void __launch_bounds__(kThreads)
resize_tile_kernel(P p, const int *__restrict__ yfirst, const int *__restrict__ ycount, const float *__restrict__ ywt,
                   int ytaps, const int *__restrict__ xfirst, const int *__restrict__ xcount, const float *__restrict__ xwt,
                   int xtaps, int OH, int OW, float mul, float *__restrict__ out, long stride_y, long stride_x,
                   long stride_c, int C_out, int cap_rows, int cap_cols) {
    extern __shared__ __align__(16) unsigned char lds[];           // the region, then the tile's weights
    p.prologue(reinterpret_cast<double *>(lds));                   // borrows the front of the LDS the staging then overwrites
    const TileGeom g = tile_geom(yfirst, ycount, xfirst, xcount, OH, OW, cap_rows, cap_cols);
    p.stage(lds, g, cap_rows, cap_cols);
    float *s_wx = reinterpret_cast<float *>(lds + P::region_bytes(p.C, cap_rows, cap_cols));
    float *s_wy = s_wx + kTX * xtaps;
    stage_weights(s_wx, s_wy, xwt, xtaps, ywt, ytaps, g.ox0, g.oy0, OW, OH);
    __syncthreads();
    const int ox = g.ox0 + (threadIdx.x % kTX), oy = g.oy0 + (threadIdx.x / kTX);
    if (ox >= OW || oy >= OH) return;
    const int x0 = xfirst[ox], nx = xcount[ox];
    const int y0 = yfirst[oy], ny = ycount[oy];
    float acc[4];
    aa_taps(acc, p.C, ny, nx, s_wy + (threadIdx.x / kTX) * ytaps, s_wx + (threadIdx.x % kTX) * xtaps,
            [&](int j, int i) { return p.tile_px(lds, g, cap_rows, cap_cols, y0 + j, x0 + i); });
    aa_store(acc, mul, p.C, C_out, out, oy, ox, stride_y, stride_x, stride_c);
}

// Flat form, for very large down-scales (the region of a tile does not fit the LDS cap): every tap straight from global
// memory through the same per-pixel function, so the same values as the tiled form.
template <class P>
__global__ void __launch_bounds__(kThreads)
resize_flat_kernel(P p, const int *__restrict__ yfirst, const int *__restrict__ ycount, const float *__restrict__ ywt,
                   int ytaps, const int *__restrict__ xfirst, const int *__restrict__ xcount, const float *__restrict__ xwt,
                   int xtaps, int OH, int OW, float mul, float *__restrict__ out, long stride_y, long stride_x,
                   long stride_c, int C_out) {
    if constexpr (P::kPrologueDoubles > 0) {
        __shared__ double red[P::kPrologueDoubles];
        p.prologue(red);
    }
    const long total = (long)OH * OW;
    for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long)gridDim.x * kThreads) {
        const int ox = (int)(t % OW), oy = (int)(t / OW);
        const int x0 = xfirst[ox], nx = xcount[ox];
        const int y0 = yfirst[oy], ny = ycount[oy];
        float acc[4];
        aa_taps(acc, p.C, ny, nx, ywt + (long)oy * ytaps, xwt + (long)ox * xtaps,
                [&](int j, int i) { return p.src_px(y0 + j, x0 + i); });
        aa_store(acc, mul, p.C, C_out, out, oy, ox, stride_y, stride_x, stride_c);
    }
}

// The largest region a tile can touch is (T-1)*scale + taps + 2 source rows / columns; lds: that region plus the weights.
struct TileCaps {
    int rows, cols;
    size_t lds;
};

template <class P>
TileCaps tile_caps(int H, int W, int OH, int OW, int C) {
    const int ytaps = tsod_resize_aa_taps(H, OH), xtaps = tsod_resize_aa_taps(W, OW);
    const float sy = (float)H / (float)OH, sx = (float)W / (float)OW;
    TileCaps c;
    c.rows = (int)ceilf((kTY - 1) * sy) + ytaps + 2;
    c.cols = (int)ceilf((kTX - 1) * sx) + xtaps + 2;
    c.lds = P::region_bytes(C, c.rows, c.cols) + (size_t)(kTX * xtaps + kTY * ytaps) * sizeof(float);
    return c;
}

inline int flat_blocks(int OH, int OW) {
    const long blocks = ((long)OH * OW + kThreads - 1) / kThreads;
    return (int)(blocks < 8192 ? blocks : 8192);
}

// One resize of an H x W source to OH x OW: tiled when a tile's region fits the policy's LDS cap, else flat.
template <class P>
int launch_resize(const P &p, int H, int W, const int32_t *yfirst, const int32_t *ycount, const float *ywt,
                  const int32_t *xfirst, const int32_t *xcount, const float *xwt, int OH, int OW, float mul, float *out,
                  int64_t stride_y, int64_t stride_x, int64_t stride_c, int C_out, tsod_stream_t stream) {
    const int ytaps = tsod_resize_aa_taps(H, OH), xtaps = tsod_resize_aa_taps(W, OW);
    const TileCaps cap = tile_caps<P>(H, W, OH, OW, p.C);
    if (cap.lds <= P::kLdsCap) {
        const int tiles = ((OH + kTY - 1) / kTY) * ((OW + kTX - 1) / kTX);
        const size_t red = P::kPrologueDoubles * sizeof(double);
        hipLaunchKernelGGL(resize_tile_kernel<P>, dim3(tiles), dim3(kThreads), cap.lds > red ? cap.lds : red,
                           tsod_stream(stream), p, yfirst, ycount, ywt, ytaps, xfirst, xcount, xwt, xtaps, OH, OW, mul, out,
                           (long)stride_y, (long)stride_x, (long)stride_c, C_out, cap.rows, cap.cols);
    } else {
        hipLaunchKernelGGL(resize_flat_kernel<P>, dim3(flat_blocks(OH, OW)), dim3(kThreads), 0, tsod_stream(stream), p,
                           yfirst, ycount, ywt, ytaps, xfirst, xcount, xwt, xtaps, OH, OW, mul, out, (long)stride_y,
                           (long)stride_x, (long)stride_c, C_out);
    }
    return tsod_launch_status();
}

}  // namespace
