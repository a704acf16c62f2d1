// conv3x3_grads.hip -- the parameter gradients of HarDNet's first layer:
//
//   y[n][oh][ow][o] = relu6(scale[o] * sum_{kh,kw,c} w[o][kh][kw][c] x4[n][oh s - 1 + kh][ow s - 1 + kw][c] + shift[o])
//
//   tsod_conv3x3_wgrad_f32   g = dy * [0 < y < 6] taken from the saved y on the fly, dWraw = g^T patches on
//                            v_mfma_f32_32x32x2_f32 over slices of output rows, then one finishing launch:
//                            dW = scale * dWraw, dscale = sum_k w * dWraw (k over the 27 real taps), dshift = sum g
//
// The image has no gradient, so there is no dx.  Channel 3 of x4 (the pad channel) is never loaded: whatever it holds cannot
// reach a result.  No float atomics; slices, the in-workgroup tree and the finishing sums depend on the shape only, so the
// results are bit-identical from run to run.  The tap reads of x4 overlap (2.25x at stride 2, 9x at stride 1); they are left to
// L1 / L2: a wave's 27 columns of one output pixel lie in three 48-byte runs of x4, and the next pair's runs share a cache line.
#include "grad_reduce.h"

namespace {

constexpr int kWaves = 8, kThreads = 64 * kWaves;
constexpr int kCols = 32;                                            // 27 real (tap, channel) columns in one MFMA tile
constexpr int kMaxSlices = 512;
constexpr int kMinPairsPerSlice = 256;
constexpr int kUnroll = 4;
constexpr int kMaxCout = 64;

struct Conv3WgradShape {
    int OH, OW, rows, pairs_per_row, rows_per_slice, splits, o_tiles;
};

// Slices are whole output rows (n, oh): as many rows per slice as keeps the slice count at or below 512 and gives every slice
// at least 256 pixel pairs; the last slice may be short.  8 x 800 x 1333 at stride 2: 3 200 rows of 334 pairs, 7 rows per
// slice, 458 slices.  600 x 600: 300 rows of 150 pairs, 2 rows per slice, 150 slices.
__host__ __device__ inline Conv3WgradShape conv3_wgrad_shape(int N, int H, int W, int cout_pad, int stride) {
    Conv3WgradShape s;
    s.OH = (H - 1) / stride + 1;
    s.OW = (W - 1) / stride + 1;
    s.rows = N * s.OH;
    s.pairs_per_row = (s.OW + 1) / 2;
    const int by_count = (s.rows + kMaxSlices - 1) / kMaxSlices;
    const int by_size = (kMinPairsPerSlice + s.pairs_per_row - 1) / s.pairs_per_row;
    s.rows_per_slice = by_count > by_size ? by_count : by_size;
    s.splits = (s.rows + s.rows_per_slice - 1) / s.rows_per_slice;
    s.o_tiles = (cout_pad + 31) / 32;
    return s;
}

inline bool conv3_wgrad_shape_ok(int64_t N, int64_t H, int64_t W, int cout_pad, int stride) {
    if (N <= 0 || H <= 0 || W <= 0 || cout_pad <= 0 || (cout_pad & 3) || cout_pad > kMaxCout) return false;
    if (stride != 1 && stride != 2) return false;
    return N * H <= 0x7fffffff / 2 && W <= 0x7fffffff / (4 * kMaxCout);   // (rows and in-row offsets stay in 32 bits)
}

// D = A B on v_mfma_f32_32x32x2_f32 with two output pixels as K: A = g^T (32 o x 2 pixels: lane l holds o = l & 31 of pixel
// l >> 5), B = the patches (2 pixels x 32 columns: lane l holds column l & 31 = 3 tap + c, tap = 3 kh + kw, of pixel l >> 5;
// columns 27..31 are zeros).  A workgroup of 8 waves owns one slice of output rows and all OT tiles of 32 output channels; wave
// v takes the pairs v, v + 8, ... of every row.  The waves are summed by tsod_wave_tree_sum (4..7 -> 0..3, 2..3 -> 0..1, 1 -> 0),
// the two pixel halves of a column sum last.
template <int OT>
__global__ void __launch_bounds__(kThreads)
conv3x3_wgrad_partial_kernel(const float *__restrict__ x4, int H, int W, const float *__restrict__ y, const float *__restrict__ dy,
                             int dy_pitch, int dy_off, int cout_pad, int stride, Conv3WgradShape sh, float *__restrict__ part,
                             float *__restrict__ part_b) {
    __shared__ float lds[(kWaves / 2) * (OT * 17) * 64];                // per lane: OT x 16 tile values + OT column sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int tap = c / 3, ch = c - 3 * tap, kh = tap / 3, kw = tap - 3 * kh;
    const bool col_ok = c < 27;
    bool o_ok[OT];
#pragma unroll
    for (int t = 0; t < OT; ++t) o_ok[t] = 32 * t + c < cout_pad;
    tsod_f32x16 acc[OT];
    float bsum[OT];
#pragma unroll
    for (int t = 0; t < OT; ++t) {
        bsum[t] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    }
    const int row_begin = blockIdx.x * sh.rows_per_slice;
    const int row_end = row_begin + sh.rows_per_slice < sh.rows ? row_begin + sh.rows_per_slice : sh.rows;
    for (int row = row_begin; row < row_end; ++row) {
        const int n = row / sh.OH, oh = row - n * sh.OH;
        const int ih = oh * stride - 1 + kh;
        const bool ih_ok = col_ok && ih >= 0 && ih < H;
        const float *xrow = x4 + ((long)n * H + (ih_ok ? ih : 0)) * W * 4 + ch;
        const float *yrow = y + (long)row * sh.OW * cout_pad + c;
        const float *drow = dy + (long)row * sh.OW * dy_pitch + dy_off + c;
        for (int j0 = wave; j0 < sh.pairs_per_row; j0 += kWaves * kUnroll) {
            float b[kUnroll], a[OT][kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int j = j0 + kWaves * u;
                const int ow = 2 * j + h;
                const bool ok = j < sh.pairs_per_row && ow < sh.OW;
                const int iw = ow * stride - 1 + kw;
                b[u] = (ok && ih_ok && iw >= 0 && iw < W) ? xrow[iw * 4] : 0.f;
#pragma unroll
                for (int t = 0; t < OT; ++t) {
                    a[t][u] = 0.f;
                    if (ok && o_ok[t]) {
                        const float yv = yrow[ow * cout_pad + 32 * t];
                        const float d = drow[ow * dy_pitch + 32 * t];
                        a[t][u] = tsod_relu6_open(yv) ? d : 0.f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u)
#pragma unroll
                for (int t = 0; t < OT; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][u], b[u], acc[t], 0, 0, 0);
                    bsum[t] += a[t][u];
                }
        }
    }
    tsod_wave_tree_sum<kWaves, OT, OT>(acc, bsum, lds, wave, lane);
    if (wave != 0) return;
    float *out = part + (long)blockIdx.x * (OT * 32 * kCols);
    float *out_b = part_b + (long)blockIdx.x * (OT * 32);
#pragma unroll
    for (int t = 0; t < OT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
            out[o * kCols + c] = acc[t][r];
        }
        const float both = bsum[t] + __shfl_xor(bsum[t], 32);
        if (h == 0) out_b[32 * t + c] = both;
    }
}

// One workgroup of 64 threads per output row o of the padded weight.  Thread t < 36 owns dW[o][t >> 2][t & 3]: dWraw = the
// slices' partials in slice order; pad rows and channel 3 are written as zeros and never
// read.  Thread 0 then adds w * dWraw over the 27 real taps in ascending (kh, kw, c): dscale.  Thread 63: dshift, slice order.
__global__ void __launch_bounds__(64)
conv3x3_wgrad_finish_kernel(const float *__restrict__ part, const float *__restrict__ part_b, int splits, int o_pad, int cout_real,
                            const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ dw,
                            float *__restrict__ dscale, float *__restrict__ dshift) {
    __shared__ float prod[27];
    const int o = blockIdx.x, t = threadIdx.x;
    const bool real = o < cout_real;
    if (t < 36) {
        const int k = t >> 2, ch = t & 3;
        const bool live = real && ch < 3;
        float raw = 0.f;
        if (live && (dw || dscale)) raw = tsod_sum_in_slice_order(part + (long)o * kCols + 3 * k + ch, (long)o_pad * kCols, splits);
        if (dw) dw[o * 36 + t] = live ? scale[o] * raw : 0.f;
        if (live && dscale) prod[3 * k + ch] = w[o * 36 + t] * raw;
    }
    __syncthreads();
    if (t == 0 && dscale) {
        float s = 0.f;
        if (real)
            for (int k = 0; k < 27; ++k) s += prod[k];
        dscale[o] = s;
    }
    if (t == 63 && dshift) {
        dshift[o] = real ? tsod_sum_in_slice_order(part_b + o, o_pad, splits) : 0.f;
    }
}

}  // namespace

extern "C" size_t tsod_conv3x3_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cout_pad, int32_t stride) {
    if (!conv3_wgrad_shape_ok(N, H, W, Cout_pad, stride)) return 0;
    const Conv3WgradShape s = conv3_wgrad_shape(N, H, W, Cout_pad, stride);
    return (size_t)s.splits * (size_t)(s.o_tiles * 32) * (kCols + 1) * sizeof(float);
}

extern "C" int tsod_conv3x3_wgrad_f32(const float *x4, int32_t N, int32_t H, int32_t W, const float *y, const float *dy,
                                      int32_t dy_pitch, int32_t dy_off, const float *w, const float *scale, int32_t Cout_pad,
                                      int32_t Cout_real, int32_t stride, float *dw, float *dscale, float *dshift, void *workspace,
                                      size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(x4 && y && dy && w && scale && (dw || dscale || dshift), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && H > 0 && W > 0 && Cout_pad > 0 && Cout_real > 0 && Cout_real <= Cout_pad && (stride == 1 || stride == 2),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(dy_off >= 0 && dy_pitch >= dy_off + Cout_pad, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((Cout_pad & 3) == 0 && (dy_pitch & 3) == 0 && (dy_off & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(x4) && tsod_aligned16(y) && tsod_aligned16(dy) && tsod_aligned16(w) && tsod_aligned16(scale),
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(conv3_wgrad_shape_ok(N, H, W, Cout_pad, stride), TSOD_ERR_UNSUPPORTED);
    const Conv3WgradShape sh = conv3_wgrad_shape(N, H, W, Cout_pad, stride);
    TSOD_REQUIRE((int64_t)sh.OW * dy_pitch <= 0x7fffffff, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) &&
                     workspace_bytes >= tsod_conv3x3_wgrad_workspace_bytes(N, H, W, Cout_pad, stride),
                 TSOD_ERR_WORKSPACE);
    const int o_pad = sh.o_tiles * 32;
    float *part = static_cast<float *>(workspace);
    float *part_b = part + (size_t)sh.splits * o_pad * kCols;
    hipStream_t st = tsod_stream(stream);
    if (sh.o_tiles == 1)
        hipLaunchKernelGGL(conv3x3_wgrad_partial_kernel<1>, dim3(sh.splits), dim3(kThreads), 0, st, x4, H, W, y, dy, dy_pitch,
                           dy_off, Cout_pad, stride, sh, part, part_b);
    else
        hipLaunchKernelGGL(conv3x3_wgrad_partial_kernel<2>, dim3(sh.splits), dim3(kThreads), 0, st, x4, H, W, y, dy, dy_pitch,
                           dy_off, Cout_pad, stride, sh, part, part_b);
    hipLaunchKernelGGL(conv3x3_wgrad_finish_kernel, dim3(Cout_pad), dim3(64), 0, st, (const float *)part, (const float *)part_b,
                       sh.splits, o_pad, Cout_real, w, scale, dw, dscale, dshift);
    return tsod_launch_status();
}
