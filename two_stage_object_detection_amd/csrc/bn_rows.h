// bn_rows.h -- what the train-mode BatchNorm kernels over NHWC f32 rows share (bn_train.hip, bn_prelu_train.hip; DESIGN.md
// sections 4.20 and 4.24): how a workgroup of 256 threads covers kBnRows rows x (up to) 256 channels, its f64 tree sum, and the
// entry points' slice checks.  A thread owns one channel quad (16-byte loads) and every rows_step-th row of the workgroup's rows.
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

inline bool bn_slice_ok(int32_t C_pad, int32_t ld, int32_t off) { return off >= 0 && ld > 0 && (long)off + C_pad <= ld; }
inline bool bn_slice_aligned(const void *p, int32_t ld, int32_t off) { return tsod_aligned16(p) && (ld & 3) == 0 && (off & 3) == 0; }
inline dim3 bn_grid(long M, int C4) { return dim3((unsigned)bn_row_blocks(M), (unsigned)tsod_cdiv(C4, bn_quads_across(C4))); }

}  // namespace
