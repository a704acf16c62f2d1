// stem_grads.hip -- the backward of ResNet's stem:
//
//   z = scale[o] * conv7x7(x4, w, stride 2, pad 3)[o] + shift[o],  y = prelu(z) with one slope a > 0,  p = maxpool3x3(y, stride 2, pad 1)
//
//   tsod_prelu_grad_pool_f32    tsod_prelu_grad_f32 on y whose dy is never written out: every element of y gathers, from the
//                               gradient dp of the pooled map, the windows it won (the first maximum in ascending (kh, kw), what
//                               torch's max_pool2d backward does), recomputing each window's winner from y
//   tsod_conv7x7s2_wgrad_f32    dWraw = g^T patches(x4) on v_mfma_f32_32x32x2_f32: in NHWC4 the 8 x 4 floats (kw, c) of one kernel
//                               row are 32 contiguous floats of x4, one MFMA column tile; slices of pixel pairs, then one finishing
//                               launch: dW = scale * dWraw, dscale = sum over the 147 real taps of w * dWraw, dshift = sum g
//
// The image has no gradient, so there is no dx.  No float atomics; every order of additions below depends on the shape only
// (grad_reduce.h), so the results are bit-identical from run to run.
#include "grad_reduce.h"

namespace {

// ------------------------------------------------------------------------------------------------ max pool + PReLU backward
constexpr int kPoolMaxBlocks = 1024;                                  // tsod_prelu_grad_f32's grid rule

inline unsigned pool_blocks(long rows, int C) {
    const long b = tsod_cdiv(rows * (C / 4), 256);
    return (unsigned)(b < kPoolMaxBlocks ? b : kPoolMaxBlocks);
}

inline bool pool_shape_ok(int64_t N, int64_t OH, int64_t OW, int64_t C) {
    if (N <= 0 || OH <= 0 || OW <= 0 || C <= 0 || (C & 3)) return false;
    // (quads and the grid's stride stay in 32 bits: total + 1024 * 256 < 2^32, rows < 2^31)
    return N * OH * OW <= 0x7fffffffL && N * OH * OW * (C / 4) < 0x7fffffffL;
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// One quad of channels of y's pixel (n, oh, ow) per thread and step, tsod_prelu_grad_f32's grid-stride loop over rows = N OH OW.
// The pixel lies in the windows ph = oh / 2 (and oh / 2 + 1 where oh is odd and that window exists), pw likewise: window ph
// covers rows 2 ph - 1 .. 2 ph + 1.  It is the winner of a window exactly where every tap before it in the (kh, kw) scan is
// strictly smaller and no tap after it is larger (taps outside the image do not take part): the first maximum under a strict
// > replacement.  dy adds the won windows' dp in ascending (ph, pw).  kSum: this workgroup's part of sum dy * y * [y < 0]
// (grad_reduce.h: tsod_strided_sum_256) goes to partial[blockIdx.x].
template <bool kSum>
__global__ void __launch_bounds__(256)
prelu_grad_pool_kernel(const float *__restrict__ y, long rows, int OH, int OW, int C4, int y_pitch, const float *__restrict__ dp,
                       int PH, int PW, int dp_pitch, float slope, float *__restrict__ g, int g_pitch, float *__restrict__ partial) {
    __shared__ float lds[256];
    const unsigned total = (unsigned)(rows * C4), step = gridDim.x * 256u;
    float sum = 0.f;
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < total; t += step) {
        const unsigned m = t / (unsigned)C4;
        const int c = 4 * (int)(t - m * (unsigned)C4);
        const unsigned row = m / (unsigned)OW, n = row / (unsigned)OH;
        const int ow = (int)(m - row * (unsigned)OW), oh = (int)(row - n * (unsigned)OH);
        const float *yn = y + (long)n * OH * OW * y_pitch + c;
        const float4 v = ld4(yn + ((long)oh * OW + ow) * y_pitch);
        const int ph0 = oh >> 1, pw0 = ow >> 1;
        const int ph1 = (oh & 1) && ph0 + 1 < PH ? ph0 + 1 : ph0;
        const int pw1 = (ow & 1) && pw0 + 1 < PW ? pw0 + 1 : pw0;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int ph = ph0 + a, pw = pw0 + b;
                if (ph > ph1 || pw > pw1) continue;
                const int mine = (oh - (2 * ph - 1)) * 3 + (ow - (2 * pw - 1));      // this pixel's place in the scan
                // all nine taps are loaded at once from clamped (always valid) places; a tap outside the image, or this
                // pixel's own, takes no part in the comparison
                float4 u[9];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int ih = 2 * ph - 1 + tap / 3, iw = 2 * pw - 1 + tap % 3;
                    const int ihc = ih < 0 ? 0 : (ih >= OH ? OH - 1 : ih), iwc = iw < 0 ? 0 : (iw >= OW ? OW - 1 : iw);
                    u[tap] = ld4(yn + ((long)ihc * OW + iwc) * y_pitch);
                }
                const float4 q = ld4(dp + (((long)n * PH + ph) * PW + pw) * dp_pitch + c);
                bool wx = true, wy = true, wz = true, ww = true;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int ih = 2 * ph - 1 + tap / 3, iw = 2 * pw - 1 + tap % 3;
                    const bool skip = (unsigned)ih >= (unsigned)OH || (unsigned)iw >= (unsigned)OW || tap == mine;
                    const bool before = tap < mine;
                    wx = wx && (skip || (before ? u[tap].x < v.x : u[tap].x <= v.x));
                    wy = wy && (skip || (before ? u[tap].y < v.y : u[tap].y <= v.y));
                    wz = wz && (skip || (before ? u[tap].z < v.z : u[tap].z <= v.z));
                    ww = ww && (skip || (before ? u[tap].w < v.w : u[tap].w <= v.w));
                }
                d.x += wx ? q.x : 0.f;
                d.y += wy ? q.y : 0.f;
                d.z += wz ? q.z : 0.f;
                d.w += ww ? q.w : 0.f;
            }
        float4 o;
        o.x = v.x > 0.f ? d.x : slope * d.x;
        o.y = v.y > 0.f ? d.y : slope * d.y;
        o.z = v.z > 0.f ? d.z : slope * d.z;
        o.w = v.w > 0.f ? d.w : slope * d.w;
        *reinterpret_cast<float4 *>(g + (long)m * g_pitch + c) = o;
        if (kSum) {
            sum += v.x < 0.f ? d.x * v.x : 0.f;
            sum += v.y < 0.f ? d.y * v.y : 0.f;
            sum += v.z < 0.f ? d.z * v.z : 0.f;
            sum += v.w < 0.f ? d.w * v.w : 0.f;
        }
    }
    if (kSum) {
        const float s = tsod_tree_sum_256(sum, lds, threadIdx.x);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}

// tsod_prelu_grad_f32's second stage: thread t adds partials t, t + 256, ... ascending, then tsod_tree_sum_256
__global__ void __launch_bounds__(256)
prelu_grad_pool_finish_kernel(const float *__restrict__ partial, int count, float *__restrict__ out) {
    __shared__ float lds[256];
    float sum = 0.f;
    for (int i = threadIdx.x; i < count; i += 256) sum += partial[i];
    const float s = tsod_tree_sum_256(sum, lds, threadIdx.x);
    if (threadIdx.x == 0) *out = s;
}

// ------------------------------------------------------------------------------------------------------- 7x7 stride-2 wgrad
constexpr int kS7Waves = 4, kS7Threads = 64 * kS7Waves;
constexpr int kS7Cout = 64, kS7Rows = 7, kS7Cols = 32 * kS7Rows;      // the pack's [64][7][8][4]: 224 columns, 147 of them real
constexpr int kS7TargetSlices = 256;                                  // one workgroup per CU: 224 accumulators, one wave per SIMD
constexpr int kS7MinPairsPerSlice = 64;
constexpr int kS7Unroll = 2;

struct Stem7Shape {
    int OH, OW, rows, pairs_per_row, pairs, pairs_per_slice, splits;
};

// Slices are runs of pixel pairs, pairs numbered (n, oh, ow / 2) ascending (a pair never spans two output rows): as many pairs
// per slice as gives at most 256 slices of at least 64 pairs; the last slice may be short.  800 x 1333: 400 rows of 334 pairs,
// 522 pairs per slice, 256 slices; 64 x 96: 768 pairs, 12 slices of 64.
__host__ __device__ inline Stem7Shape stem7_shape(int N, int H, int W) {
    Stem7Shape s;
    s.OH = (H - 1) / 2 + 1;
    s.OW = (W - 1) / 2 + 1;
    s.rows = N * s.OH;
    s.pairs_per_row = (s.OW + 1) / 2;
    s.pairs = s.rows * s.pairs_per_row;
    const int by_count = (s.pairs + kS7TargetSlices - 1) / kS7TargetSlices;
    s.pairs_per_slice = by_count > kS7MinPairsPerSlice ? by_count : kS7MinPairsPerSlice;
    s.splits = (s.pairs + s.pairs_per_slice - 1) / s.pairs_per_slice;
    return s;
}

inline bool stem7_shape_ok(int64_t N, int64_t H, int64_t W, int64_t Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cout != kS7Cout) return false;
    return N * H * W <= 0x7fffffff / 4;                               // (offsets into x4, and so the pair count, stay in 32 bits)
}

// D = A B on v_mfma_f32_32x32x2_f32 with two output pixels as K: A = g^T (32 o x 2 pixels: lane l holds o = l & 31 of pixel
// l >> 5), B = one kernel row of the patches (2 pixels x 32 columns: lane l holds column l & 31 = 4 kw + c of pixel l >> 5, the
// float x4[n][2 oh - 3 + kh][2 ow - 3 + kw][c]; a tap outside the image is a zero and is not loaded).  Columns kw = 7 and c = 3
// carry what the image holds there: a column of B reaches the same column of D only, and the finish never reads those.  A
// wave holds all 2 x 7 tiles (o tile, kh) and takes the pairs wave, wave + 4, ... of its slice; the four waves are summed by
// tsod_wave_tree_sum, one o tile at a time, the two pixel halves of dshift's column sums last.
__global__ void __launch_bounds__(kS7Threads)
conv7x7s2_wgrad_partial_kernel(const float *__restrict__ g, int g_pitch, const float *__restrict__ x4, int H, int W, Stem7Shape sh,
                               float *__restrict__ part, float *__restrict__ part_b) {
    __shared__ float lds[(kS7Waves / 2) * (kS7Rows * 16 + 1) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    tsod_f32x16 acc[2][kS7Rows];
    float bsum[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int k = 0; k < kS7Rows; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][k][r] = 0.f;
    const int p_begin = blockIdx.x * sh.pairs_per_slice;
    const int p_end = p_begin + sh.pairs_per_slice < sh.pairs ? p_begin + sh.pairs_per_slice : sh.pairs;
    for (int p0 = p_begin + wave; p0 < p_end; p0 += kS7Waves * kS7Unroll) {
        float a[kS7Unroll][2], b[kS7Unroll][kS7Rows];
#pragma unroll
        for (int u = 0; u < kS7Unroll; ++u) {
            a[u][0] = a[u][1] = 0.f;
#pragma unroll
            for (int k = 0; k < kS7Rows; ++k) b[u][k] = 0.f;
            const int p = p0 + kS7Waves * u;
            if (p >= p_end) continue;
            const unsigned row = (unsigned)p / (unsigned)sh.pairs_per_row, n = row / (unsigned)sh.OH;
            const int ow = 2 * (int)((unsigned)p - row * (unsigned)sh.pairs_per_row) + h, oh = (int)(row - n * (unsigned)sh.OH);
            if (ow >= sh.OW) continue;
            const float *gp = g + ((long)row * sh.OW + ow) * g_pitch + c;
            a[u][0] = gp[0];
            a[u][1] = gp[32];
            const int iw = 2 * ow - 3 + (c >> 2);
            if ((unsigned)iw >= (unsigned)W) continue;
            const float *xp = x4 + (((long)n * H) * W + iw) * 4 + (c & 3);
#pragma unroll
            for (int k = 0; k < kS7Rows; ++k) {
                const int ih = 2 * oh - 3 + k;
                if ((unsigned)ih < (unsigned)H) b[u][k] = xp[(long)ih * W * 4];
            }
        }
#pragma unroll
        for (int u = 0; u < kS7Unroll; ++u) {
#pragma unroll
            for (int k = 0; k < kS7Rows; ++k) {
                acc[0][k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], b[u][k], acc[0][k], 0, 0, 0);
                acc[1][k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][1], b[u][k], acc[1][k], 0, 0, 0);
            }
            bsum[0] += a[u][0];
            bsum[1] += a[u][1];
        }
    }
    tsod_wave_tree_sum<kS7Waves, kS7Rows, 1>(acc[0], &bsum[0], lds, wave, lane);
    tsod_wave_tree_sum<kS7Waves, kS7Rows, 1>(acc[1], &bsum[1], lds, wave, lane);
    if (wave != 0) return;
    float *out = part + (long)blockIdx.x * (kS7Cout * kS7Cols);
    float *out_b = part_b + (long)blockIdx.x * kS7Cout;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int k = 0; k < kS7Rows; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                out[o * kS7Cols + 32 * k + c] = acc[t][k][r];
            }
        const float both = bsum[t] + __shfl_xor(bsum[t], 32);
        if (h == 0) out_b[32 * t + c] = both;
    }
}

// One workgroup of 256 threads per output channel o.  Thread t < 224 owns column t = (kh 8 + kw) 4 + c of the pack's row:
// dWraw = the slices' partials in slice order; the pad columns (kw = 7, c = 3) are never read and written as zeros.  Thread 0
// then adds w * dWraw over the 147 real taps in ascending (kh, kw, c): dscale.  Thread 255: dshift, slice order.
__global__ void __launch_bounds__(256)
conv7x7s2_wgrad_finish_kernel(const float *__restrict__ part, const float *__restrict__ part_b, int splits,
                              const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ dw,
                              float *__restrict__ dscale, float *__restrict__ dshift) {
    __shared__ float prod[kS7Cols];
    const int o = blockIdx.x, t = threadIdx.x;
    if (t < kS7Cols) {
        const bool real = (t & 3) < 3 && ((t >> 2) & 7) < 7;
        float raw = 0.f;
        if (real && (dw || dscale)) raw = tsod_sum_in_slice_order(part + (long)o * kS7Cols + t, (long)kS7Cout * kS7Cols, splits);
        if (dw) dw[o * kS7Cols + t] = real ? scale[o] * raw : 0.f;
        prod[t] = real ? w[o * kS7Cols + t] * raw : 0.f;
    }
    __syncthreads();
    if (t == 0 && dscale) {
        float s = 0.f;
        for (int k = 0; k < kS7Cols; ++k)
            if ((k & 3) < 3 && ((k >> 2) & 7) < 7) s += prod[k];
        dscale[o] = s;
    }
    if (t == 255 && dshift) dshift[o] = tsod_sum_in_slice_order(part_b + o, kS7Cout, splits);
}

}  // namespace

extern "C" size_t tsod_prelu_grad_pool_workspace_bytes(int32_t N, int32_t OH, int32_t OW, int32_t C) {
    if (!pool_shape_ok(N, OH, OW, C)) return 0;
    return (size_t)pool_blocks((long)N * OH * OW, C) * sizeof(float);
}

extern "C" int tsod_prelu_grad_pool_f32(const float *y, int32_t N, int32_t OH, int32_t OW, int32_t C, int32_t y_pitch, const float *dp,
                                        int32_t dp_pitch, float slope, float *g, int32_t g_pitch, float *dslope_num, void *workspace,
                                        size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(y && dp && g, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && OH > 0 && OW > 0 && C > 0 && y_pitch >= C && dp_pitch >= C && g_pitch >= C, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((C & 3) == 0 && (y_pitch & 3) == 0 && (dp_pitch & 3) == 0 && (g_pitch & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(y) && tsod_aligned16(dp) && tsod_aligned16(g), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(pool_shape_ok(N, OH, OW, C), TSOD_ERR_UNSUPPORTED);
    const long rows = (long)N * OH * OW;
    const int PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1;
    const unsigned blocks = pool_blocks(rows, C);
    hipStream_t st = tsod_stream(stream);
    if (!dslope_num) {                                                  // no reduction, no workspace
        hipLaunchKernelGGL(prelu_grad_pool_kernel<false>, dim3(blocks), dim3(256), 0, st, y, rows, OH, OW, C / 4, y_pitch, dp, PH, PW,
                           dp_pitch, slope, g, g_pitch, (float *)nullptr);
        return tsod_launch_status();
    }
    TSOD_REQUIRE(workspace && workspace_bytes >= tsod_prelu_grad_pool_workspace_bytes(N, OH, OW, C), TSOD_ERR_WORKSPACE);
    float *partial = static_cast<float *>(workspace);
    hipLaunchKernelGGL(prelu_grad_pool_kernel<true>, dim3(blocks), dim3(256), 0, st, y, rows, OH, OW, C / 4, y_pitch, dp, PH, PW,
                       dp_pitch, slope, g, g_pitch, partial);
    hipLaunchKernelGGL(prelu_grad_pool_finish_kernel, dim3(1), dim3(256), 0, st, (const float *)partial, (int)blocks, dslope_num);
    return tsod_launch_status();
}

extern "C" size_t tsod_conv7x7s2_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cout) {
    if (!stem7_shape_ok(N, H, W, Cout)) return 0;
    const Stem7Shape s = stem7_shape(N, H, W);
    return (size_t)s.splits * kS7Cout * (kS7Cols + 1) * sizeof(float);
}

extern "C" int tsod_conv7x7s2_wgrad_f32(const float *g, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t g_pitch,
                                        const float *x4, const float *w, const float *scale, float *dw, float *dscale,
                                        float *dshift, void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(g && x4 && w && scale && (dw || dscale || dshift), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && g_pitch >= Cout, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((Cout & 3) == 0 && (g_pitch & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(g) && tsod_aligned16(x4) && tsod_aligned16(w) && tsod_aligned16(scale) &&
                     (!dw || tsod_aligned16(dw)),
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(stem7_shape_ok(N, H, W, Cout), TSOD_ERR_UNSUPPORTED);
    const Stem7Shape sh = stem7_shape(N, H, W);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= tsod_conv7x7s2_wgrad_workspace_bytes(N, H, W, Cout),
                 TSOD_ERR_WORKSPACE);
    float *part = static_cast<float *>(workspace);
    float *part_b = part + (size_t)sh.splits * kS7Cout * kS7Cols;
    hipStream_t st = tsod_stream(stream);
    hipLaunchKernelGGL(conv7x7s2_wgrad_partial_kernel, dim3(sh.splits), dim3(kS7Threads), 0, st, g, g_pitch, x4, H, W, sh, part, part_b);
    hipLaunchKernelGGL(conv7x7s2_wgrad_finish_kernel, dim3(kS7Cout), dim3(256), 0, st, (const float *)part, (const float *)part_b,
                       sh.splits, w, scale, dw, dscale, dshift);
    return tsod_launch_status();
}
