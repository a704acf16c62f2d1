// bn_rows.h -- what the train-mode BatchNorm kernels over NHWC f32 rows share (bn_train.hip, bn_prelu_train.hip; DESIGN.md
// sections 4.20 and 4.24): how a workgroup of 256 threads covers kBnRows rows x (up to) 256 channels, its f64 tree sum, the sum
// of the workgroups' partials, the dz pass's per-quad constants and element, and the entry points' slice checks.  A thread owns
// one channel quad (16-byte loads) and every rows_step-th row of the workgroup's rows.
//
// The sums are f64 with no float atomics, in an order the shape alone fixes, so results are bit-identical from run to run:
//   in a workgroup   a thread adds its rows ascending, then a binary tree over the row lanes (t += 128, 64, ... QX): bn_block_sum
//   across them      partial b of channel c lies at part[b][.][c]; 16 lanes per channel take contiguous runs of ceil(B / 16)
//                    partials ascending, lane 0 then merges the 16 runs ascending: bn_sum_finish_kernel (the statistics merge
//                    (n, mean, M2) by Chan's rule in the same order, in a kernel of their own: bn_train.hip)
#pragma once
#include "tsod_internal.h"

namespace {

constexpr int kBnThreads = 256;
constexpr int kBnRows = TSOD_BN_ROWS_PER_WORKGROUP;
constexpr int kBnFinishChannels = 16, kBnFinishRuns = kBnThreads / kBnFinishChannels;

// channel quads across a workgroup: the power of two that covers C4, at most 64 (then blockIdx.y walks chunks of 64 quads)
__host__ __device__ inline int bn_quads_across(int C4) {
    int q = 1;
    while (q < C4 && q < 64) q <<= 1;
    return q;
}
inline long bn_row_blocks(long M) { return (M + kBnRows - 1) / kBnRows; }

// v summed over the threads that share a channel quad (tid, tid + qx, tid + 2 qx, ...): a binary tree in LDS, every thread gets
// the total.  `lds`: NV * 256 doubles; the leading barrier frees them from an earlier call.
template <int NV>
__device__ __forceinline__ void bn_block_sum(double (&v)[NV], double *lds, int tid, int qx) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NV; ++e) lds[e * kBnThreads + tid] = v[e];
    __syncthreads();
    for (int s = kBnThreads / 2; s >= qx; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int e = 0; e < NV; ++e) lds[e * kBnThreads + tid] += lds[e * kBnThreads + tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) v[e] = lds[e * kBnThreads + (tid & (qx - 1))];
}

struct bn_lane {
    int q, ry, rows_step;                                               // channel quad, first row of the thread, row step
    long m0, m1;                                                        // the workgroup's rows
    bool live;
};
__device__ __forceinline__ bn_lane bn_lane_of(long M, int C4, int qx) {
    bn_lane t;
    const int tid = threadIdx.x;
    t.q = blockIdx.y * qx + (tid & (qx - 1));
    t.ry = tid / qx;
    t.rows_step = kBnThreads / qx;
    t.m0 = (long)blockIdx.x * kBnRows;
    t.m1 = t.m0 + kBnRows < M ? t.m0 + kBnRows : M;
    t.live = t.q < C4;
    return t;
}

// The workgroups' partial sums of kPlanes planes per channel, part [B][kPlanes][C_pad] doubles -> total [kPlanes][C_pad] doubles
// (what the elementwise pass reads) and the first two planes as the f32 dgamma / dbeta [C_pad]; pad channels: exact zeros.
template <int kPlanes>
__global__ void __launch_bounds__(kBnThreads)
bn_sum_finish_kernel(const double *__restrict__ part, long B, int C_real, int C_pad, double *__restrict__ total,
                     float *__restrict__ dgamma, float *__restrict__ dbeta) {
    static_assert(kPlanes >= 2, "the first two planes are dgamma and dbeta");
    __shared__ double lds[kPlanes * kBnThreads];
    const int tid = threadIdx.x;
    const int cl = tid % kBnFinishChannels, run = tid / kBnFinishChannels;
    const int c = blockIdx.x * kBnFinishChannels + cl;
    const long per = (B + kBnFinishRuns - 1) / kBnFinishRuns;
    const long b0 = run * per, b1 = b0 + per < B ? b0 + per : B;
    double s[kPlanes];
#pragma unroll
    for (int e = 0; e < kPlanes; ++e) s[e] = 0.;
    if (c < C_real) {
        for (long b = b0; b < b1; ++b) {
#pragma unroll
            for (int e = 0; e < kPlanes; ++e) s[e] += part[(kPlanes * b + e) * C_pad + c];
        }
    }
#pragma unroll
    for (int e = 0; e < kPlanes; ++e) lds[e * kBnThreads + tid] = s[e];
    __syncthreads();
    if (run != 0 || c >= C_pad) return;
    for (int r = 1; r < kBnFinishRuns; ++r) {
#pragma unroll
        for (int e = 0; e < kPlanes; ++e) s[e] += lds[e * kBnThreads + r * kBnFinishChannels + cl];
    }
#pragma unroll
    for (int e = 0; e < kPlanes; ++e) total[e * C_pad + c] = s[e];
    dgamma[c] = (float)s[0];
    dbeta[c] = (float)s[1];
}

// dz = gamma invstd (g - dbeta / M - xhat dgamma / M): what a thread of the elementwise pass holds per channel of its quad
// (channels [c, c + 4); total = [sum g xhat | sum g | ...][C_pad]; k is 0 at pad channels), and one element of it
struct bn_dz_quad { double mu[4], iv[4], k[4], a[4], b[4]; };
__device__ __forceinline__ bn_dz_quad bn_dz_quad_of(const float *__restrict__ mean, const float *__restrict__ invstd,
                                                    const float *__restrict__ gamma, const double *__restrict__ total, long M,
                                                    int C_real, int C_pad, int c) {
    bn_dz_quad q;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool real = c + e < C_real;
        q.mu[e] = (double)mean[c + e];
        q.iv[e] = (double)invstd[c + e];
        q.k[e] = real ? (double)gamma[c + e] * q.iv[e] : 0.;
        q.b[e] = total[c + e] / (double)M;
        q.a[e] = total[C_pad + c + e] / (double)M;
    }
    return q;
}
__device__ __forceinline__ float bn_dz_of(const bn_dz_quad &q, int e, float g, float z) {
    const double xh = ((double)z - q.mu[e]) * q.iv[e];
    return (float)(q.k[e] * ((double)g - q.a[e] - xh * q.b[e]));
}

inline bool bn_slice_ok(int32_t C_pad, int32_t ld, int32_t off) { return off >= 0 && ld > 0 && (long)off + C_pad <= ld; }
inline bool bn_slice_aligned(const void *p, int32_t ld, int32_t off) { return tsod_aligned16(p) && (ld & 3) == 0 && (off & 3) == 0; }
inline dim3 bn_grid(long M, int C4) { return dim3((unsigned)bn_row_blocks(M), (unsigned)tsod_cdiv(C4, bn_quads_across(C4))); }

}  // namespace
