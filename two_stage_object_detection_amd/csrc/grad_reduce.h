// grad_reduce.h -- what the backward files (head_grads.hip, pw_grads.hip, conv_grads.hip, conv_strided_grads.hip, conv3x3_grads.hip,
// stem_grads.hip, dw_grads.hip) and optim.hip's gradient norm share, once: the
// f32 MFMA weight-gradient tile with its slice plan, the fixed-order sum of a workgroup's waves through LDS, the sum of the
// slices' partials in slice order, and the strict ReLU6 window.  The results of those files are bit-identical from run to run
// because every order below depends on the shape only; it is stated here and nowhere else:
//   tsod_wave_tree_sum        waves [lo, 2 lo) store, waves [0, lo) add, lo = W/2 ... 1: 4 waves give (w0 + w2) + (w1 + w3)
//   tsod_wgrad_tile           a wave adds its m-pairs ascending (the MFMA adds row 2p before 2p + 1), then the wave tree; the
//                             bias adds the two lane halves, then the waves as (w0 + w1) + (w2 + w3)
//   tsod_sum_in_slice_order   0 + p[0] + p[1] + ..., one add after the other, whatever number of loads is in flight
//   tsod_tree_sum_256         256 threads' values through LDS: t += t + 128, then + 64, ... + 1 (a binary tree, thread 0 has the sum)
//   tsod_tree_sum_256_f64     the same tree over 256 doubles (optim.hip's gradient norm)
//   optim.hip                 tsod_grad_norm_f32: per chunk of 2048 elements thread t adds the exact f64 squares of quads t, t + 256
//                             (elements ascending, a last short quad included, quads counted from the chunk's first element),
//                             then tsod_tree_sum_256_f64; the finish: thread t adds partials t, t + 256, ... ascending, then
//                             tsod_tree_sum_256_f64 (the chunk count depends on the element counts only)
//   tsod_wgrad_finish_row     dWraw[o][k] = the slabs in slice order; dscale[o]: thread t adds w[o][k] dWraw[o][k] over k = t,
//                             t + 256, ... ascending, then tsod_tree_sum_256; dshift[o] = the slices' column sums in slice order
//   tsod_strided_sum_256      a grid-stride loop's lane sum (elements t, t + G, ... ascending, a quad as x, y, z, w), then
//                             tsod_tree_sum_256 per workgroup; the finish: thread t adds partials t, t + 256, ... ascending, then
//                             tsod_tree_sum_256 (conv_grads.hip's PReLU slope sum; G and the partial count depend on the shape only)
//   conv_strided_grads.hip    tsod_conv3x3_strided_wgrad_f32 is tsod_wgrad_tile and tsod_wgrad_finish_row over the rows of the
//                             OUTPUT grid (m = (n, oh, ow) ascending): at stride 1 the dense kernel's orders, add for add
//   conv_grads.hip, strided   tsod_prelu_grad_d2s_f32 is tsod_strided_sum_256 over y's N H W rows (where dy is read from does
//                             not enter the order); tsod_pixel_upsample_add_f32 makes one add per element, dx + d
//   stem_grads.hip            tsod_prelu_grad_pool_f32 adds the won windows' dp in ascending (ph, pw), then tsod_strided_sum_256
//                             over y's N OH OW rows; tsod_conv7x7s2_wgrad_f32: a wave adds its pixel pairs ascending, the wave tree
//                             per tile of 32 channels, dshift's two pixel halves last, the slices by tsod_sum_in_slice_order, dscale
//                             one thread's sum over the 147 real taps in ascending (kh, kw, c)
#pragma once
#include "tsod_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------------------- ReLU6 window
// torch's hardtanh backward: the gradient passes where 0 < v < 6, both comparisons strict
__device__ __forceinline__ bool tsod_relu6_open(float v) { return v > 0.f && v < 6.f; }
__device__ __forceinline__ float4 tsod_relu6_keep(float4 d, const float4 v) {
    d.x = tsod_relu6_open(v.x) ? d.x : 0.f;
    d.y = tsod_relu6_open(v.y) ? d.y : 0.f;
    d.z = tsod_relu6_open(v.z) ? d.z : 0.f;
    d.w = tsod_relu6_open(v.w) ? d.w : 0.f;
    return d;
}

// ---------------------------------------------------------------------------------------------------------- slice order
// src[0], src[stride], ... (count values) added in that order; 16 loads are in flight at a time, the adds stay serial
__device__ inline float tsod_sum_in_slice_order(const float *__restrict__ src, long stride, int count) {
    float sum = 0.f;
    int z = 0;
    for (; z + 16 <= count; z += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = src[(z + u) * stride];
#pragma unroll
        for (int u = 0; u < 16; ++u) sum += v[u];
    }
    for (; z < count; ++z) sum += src[z * stride];
    return sum;
}

// ---------------------------------------------------------------------------------------------------------- 256-thread tree
// every thread of a 256-thread workgroup calls it; `lds`: 256 floats; the sum is the return value of thread 0 (others: partial)
__device__ __forceinline__ float tsod_tree_sum_256(float v, float *lds, int tid) {
    lds[tid] = v;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) lds[tid] += lds[tid + st];
        __syncthreads();
    }
    return lds[0];
}
// its f64 twin (`lds`: 256 doubles), the same order
__device__ __forceinline__ double tsod_tree_sum_256_f64(double v, double *lds, int tid) {
    lds[tid] = v;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) lds[tid] = lds[tid] + lds[tid + st];
        __syncthreads();
    }
    return lds[0];
}

// ---------------------------------------------------------------------------------------------------------- wave tree
// Sum over the W waves of a workgroup of NA 32x32 accumulators and NS scalars per lane, into wave 0: log2(W) rounds, in each
// waves [lo, 2 lo) store and waves [0, lo) add (lo = W/2 ... 1).  Every thread calls it.  `lds`: (W/2) (16 NA + NS) 64 floats,
// lane-contiguous rows (no bank conflicts); free again on return.
template <int W, int NA, int NS>
__device__ __forceinline__ void tsod_wave_tree_sum(tsod_f32x16 *acc, float *extra, float *lds, int wave, int lane) {
    constexpr int kPerLane = 16 * NA + NS;
#pragma unroll
    for (int lo = W / 2; lo >= 1; lo >>= 1) {
        if (wave >= lo && wave < 2 * lo) {
            float *dst = lds + (wave - lo) * (kPerLane * 64) + lane;
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[(a * 16 + r) * 64] = acc[a][r];
#pragma unroll
            for (int s = 0; s < NS; ++s) dst[(NA * 16 + s) * 64] = extra[s];
        }
        __syncthreads();
        if (wave < lo) {
            const float *src = lds + wave * (kPerLane * 64) + lane;
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][r] += src[(a * 16 + r) * 64];
#pragma unroll
            for (int s = 0; s < NS; ++s) extra[s] += src[(NA * 16 + s) * 64];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------- wgrad tile
// dW[n][k] = sum_m dY[m][n] X[m][k] as D = A B with A = dY^T (32 n x 2 m), B = X (2 m x 32 k) on v_mfma_f32_32x32x2_f32:
// lane l holds A[n = l & 31][m = l >> 5] and B[m = l >> 5][k = l & 31].  A workgroup (4 waves) owns a 64 n x 128 k tile over
// one M-slice; every wave runs m-pairs w, w + 4, ... of the slice with 2 x 4 accumulators: one 16-byte load of X per lane
// feeds four MFMAs whose B columns are k0 + 4c + e (c = l & 31, e = 0..3), so the k of accumulator e, C/D column c, is
// k0 + 4c + e.  C/D rows: (r & 3) + 8 (r >> 2) + 4 (l >> 5).  The slice's partial tile goes to its own slab
// part[slice][n_pad][k_pad]; the k-tile-0 workgroups also give the column sums of dY (the bias) as f32 lane sums of the A
// operand, to part_b[slice][n_pad].  The caller's second launch adds the slabs with tsod_sum_in_slice_order.
constexpr int kWgThreads = 256;
constexpr int kWgN = 64, kWgK = 128;
constexpr int kWgMinPairsPerSlice = 64;
constexpr int kWgTargetWorkgroups = 512;
constexpr int kWgUnroll = 8;
constexpr int kWgLdsFloats = 2 * 128 * 64;                            // the wave tree: 2 waves x 128 values x 64 lanes (64 KiB)

struct tsod_wgrad_plan {
    int n_tiles, k_tiles, splits, pairs_per_split;
    long n_pad, k_pad;
};

// splits = what fills about 512 workgroups, with at least 64 m-pairs per slice.  `cap_by_operands` (tsod_pw_wgrad_f32): never
// more slab floats than the two operands together, splits * n_pad * k_pad <= M * (N + K).  1024 x 732 at 150 x 150 pixels: 6
// slices, 18.9 MB of slabs beside 158 MB of operands; the same layer at 874 rows: one slice.
__host__ __device__ inline tsod_wgrad_plan tsod_wgrad_plan_of(long M, int N, int K, bool cap_by_operands) {
    tsod_wgrad_plan s;
    s.n_tiles = (N + kWgN - 1) / kWgN;
    s.k_tiles = (K + kWgK - 1) / kWgK;
    s.n_pad = (long)s.n_tiles * kWgN;
    s.k_pad = (long)s.k_tiles * kWgK;
    const long pairs = (M + 1) / 2;
    const long tiles = (long)s.n_tiles * s.k_tiles;
    long splits = (kWgTargetWorkgroups + tiles - 1) / tiles;
    const long cap_rows = (pairs + kWgMinPairsPerSlice - 1) / kWgMinPairsPerSlice;
    const long cap_floats = M * ((long)N + K) / (s.n_pad * s.k_pad);
    if (splits > cap_rows) splits = cap_rows;
    if (cap_by_operands && splits > cap_floats) splits = cap_floats;
    if (splits < 1) splits = 1;
    s.pairs_per_split = (int)((pairs + splits - 1) / splits);
    s.splits = (int)((pairs + s.pairs_per_split - 1) / s.pairs_per_split);
    if (s.splits < 1) s.splits = 1;
    return s;
}
// the workspace: part [splits][n_pad][k_pad], then part_b [splits][n_pad]
inline size_t tsod_wgrad_plan_bytes(const tsod_wgrad_plan &s) {
    return (size_t)s.splits * (size_t)s.n_pad * (size_t)(s.k_pad + 1) * sizeof(float);
}
inline float *tsod_wgrad_plan_bias(const tsod_wgrad_plan &s, float *part) { return part + (size_t)s.splits * s.n_pad * s.k_pad; }

// xrow of a GEMM whose X rows are dY's rows (the 1x1 layers, the head): row m of X, always there
struct tsod_wgrad_same_row {
    __device__ __forceinline__ bool operator()(long m, int, long &mx) const { mx = m; return true; }
};

// The body of a kWgThreads kernel on grid (n_tiles * k_tiles, splits).  xcol(k): the column of X that holds gathered column k
// (k % 4 == 0; the quad k .. k + 3 lies there, 16-byte aligned), or -1 when k is past K.  xrow(m, k, mx): false where gathered
// column k of dY's row m (m < M) is a zero (a conv's padding), else true with mx = the row of X that holds it; k is the lane's
// first column, the same for every m it asks about.  `lds`: kWgLdsFloats.
template <class XCol, class XRow = tsod_wgrad_same_row>
__device__ __forceinline__ void tsod_wgrad_tile(const float *__restrict__ dy, long M, int N, int dy_pitch,
                                                const float *__restrict__ x, int x_pitch, XCol xcol, const tsod_wgrad_plan &sh,
                                                float *__restrict__ part, float *__restrict__ part_b, float *lds,
                                                XRow xrow = XRow()) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x, split = blockIdx.y;
    const int nt = tile / sh.k_tiles, kt = tile - nt * sh.k_tiles;
    const int n0 = nt * kWgN, k0 = kt * kWgK;
    const int c = lane & 31, h = lane >> 5;
    const long p_begin = (long)split * sh.pairs_per_split;
    long p_end = p_begin + sh.pairs_per_split;
    const long pairs = (M + 1) / 2;
    if (p_end > pairs) p_end = pairs;
    const int xc = xcol(k0 + 4 * c);
    const bool n_ok0 = n0 + c < N, n_ok1 = n0 + 32 + c < N;
    const bool want_b = kt == 0;
    tsod_f32x16 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][e][r] = 0.f;
    float bsum0 = 0.f, bsum1 = 0.f;
    // kWgUnroll m-pairs of loads in flight per wave before their MFMAs (the loop is otherwise bound by the load latency)
    for (long p0 = p_begin + wave; p0 < p_end; p0 += 4 * kWgUnroll) {
        float4 xv[kWgUnroll];
        float a0[kWgUnroll], a1[kWgUnroll];
#pragma unroll
        for (int u = 0; u < kWgUnroll; ++u) {
            const long p = p0 + 4 * u;
            const long m = 2 * p + h;
            xv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            a0[u] = a1[u] = 0.f;
            if (p < p_end && m < M) {
                if (xc >= 0) {
                    long mx;
                    if (xrow(m, k0 + 4 * c, mx)) xv[u] = *reinterpret_cast<const float4 *>(x + mx * x_pitch + xc);
                }
                const float *yr = dy + m * dy_pitch + n0;
                if (n_ok0) a0[u] = yr[c];
                if (n_ok1) a1[u] = yr[32 + c];
            }
        }
#pragma unroll
        for (int u = 0; u < kWgUnroll; ++u) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], xv[u].x, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], xv[u].x, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], xv[u].y, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], xv[u].y, acc[1][1], 0, 0, 0);
            acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], xv[u].z, acc[0][2], 0, 0, 0);
            acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], xv[u].z, acc[1][2], 0, 0, 0);
            acc[0][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], xv[u].w, acc[0][3], 0, 0, 0);
            acc[1][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], xv[u].w, acc[1][3], 0, 0, 0);
            if (want_b) { bsum0 += a0[u]; bsum1 += a1[u]; }
        }
    }
    tsod_wave_tree_sum<4, 8, 0>(&acc[0][0], nullptr, lds, wave, lane);
    float *bl = lds;                                                   // the bias: lane halves, then waves in order
    if (want_b) {
        bsum0 += __shfl_xor(bsum0, 32);
        bsum1 += __shfl_xor(bsum1, 32);
        if (h == 0) { bl[wave * 64 + c] = bsum0; bl[wave * 64 + 32 + c] = bsum1; }
    }
    __syncthreads();
    if (wave != 0) return;
    float *out = part + (long)split * sh.n_pad * sh.k_pad;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long n = n0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
            *reinterpret_cast<float4 *>(out + n * sh.k_pad + k0 + 4 * c) =
                make_float4(acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]);
        }
    if (want_b) {
        const float v = ((bl[lane] + bl[64 + lane]) + (bl[128 + lane] + bl[192 + lane]));
        part_b[(long)split * sh.n_pad + n0 + lane] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------- wgrad finish
// The body of a 256-thread kernel, one workgroup per real output row o, after tsod_wgrad_tile: dWraw[o][k] = the slabs in slice
// order, dW = scale[o] * dWraw at the real columns (real(k): the column of dw [.][k_real], or -1 for a pad column), and
// w[o][k] * dWraw[o][k] summed per thread in ascending k, then over the threads by tsod_tree_sum_256: dscale[o].
// dshift[o] = the slices' column sums in slice order.  w [.][K].  `lds`: 256 floats.
template <class RealCol>
__device__ __forceinline__ void tsod_wgrad_finish_row(const float *__restrict__ part, const float *__restrict__ part_b,
                                                      const tsod_wgrad_plan &sh, int K, int k_real, RealCol real,
                                                      const float *__restrict__ w, const float *__restrict__ scale,
                                                      float *__restrict__ dw, float *__restrict__ dscale,
                                                      float *__restrict__ dshift, float *lds) {
    const int o = blockIdx.x, tid = threadIdx.x;
    const long stride = sh.n_pad * sh.k_pad;
    const float s = scale[o];
    float dot = 0.f;
    if (dw || dscale) {
        for (int k = tid; k < K; k += 256) {
            const float raw = tsod_sum_in_slice_order(part + (long)o * sh.k_pad + k, stride, sh.splits);
            if (dw) {
                const int kr = real(k);
                if (kr >= 0) dw[(long)o * k_real + kr] = s * raw;
            }
            dot += w[(long)o * K + k] * raw;
        }
    }
    if (dscale) {
        const float sum = tsod_tree_sum_256(dot, lds, tid);
        if (tid == 0) dscale[o] = sum;
    }
    if (dshift && tid == 0) dshift[o] = tsod_sum_in_slice_order(part_b + o, sh.n_pad, sh.splits);
}

}  // namespace
