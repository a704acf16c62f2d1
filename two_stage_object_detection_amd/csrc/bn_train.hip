// bn_train.hip -- train-mode BatchNorm over NHWC f32 rows, HarDNet's and what ResNet's Bottlenecks put
// behind one (section 4.24), as one kernel family:
//
//   tsod_bn_stats_f32              per-channel mean and biased variance of z [M][ld] (channels [off, off + C_pad)) -> mean, invstd,
//                                  the folded scale = gamma * invstd and shift = beta - mean * scale, the running-statistics update
//   tsod_bn_apply_f32              y = act(scale * z + shift) with its own pitches / offsets and the destination's range words;
//                                  scale and shift are [2][C_pad]: the f32 value and the f32 remainder of the f64 one, summed in f64
//   tsod_bn_apply_prelu_f32        y = prelu(scale * z + shift + R, slope), R nothing, a residual tensor r, or a second
//                                  normalised operand scale2 * z2 + shift2; the terms are added in f64 and rounded to f32 once,
//                                  the PReLU runs on that f32
//   tsod_bn_train_grad_f32         dgamma = sum g xhat, dbeta = sum g, dz = gamma invstd (g - dbeta / M - xhat dgamma / M)
//   tsod_bn_prelu_train_grad_f32   tsod_prelu_grad_f32 and tsod_bn_train_grad_f32 as one group of three launches: g = dy * (y > 0
//                                  ? 1 : slope) is made from the saved output y where it is used and written out only on request
//                                  (g_out), the slope's sum dy * y * [y < 0] rides along with the BatchNorm's two sums
//
// All memory-bound: a workgroup of 256 threads owns kBnRows rows x (up to) 256 channels, a thread one channel quad (16-byte
// loads) and every rows_step-th row of the workgroup's rows.  The sums are kept in f64 (what that costs beside a copy of the same
// bytes is measured in DESIGN.md section 4.20, "Cost"): the statistics are then the correctly rounded f32 of the exact ones,
// which is what torch's CPU kernels give (their accumulation type for float is double); grad_reduce.h's f32 helpers are
// therefore not used here, its rule is: no float atomics, and every order depends on the shape only, so results are
// bit-identical from run to run:
//   in a workgroup   a thread adds its rows ascending, then a binary tree over the row lanes (t += 128, 64, ... QX): bn_block_sum
//   across them      partial b of channel c lies at part[b][.][c]; 16 lanes per channel take contiguous runs of ceil(B / 16)
//                    partials ascending, lane 0 then merges the 16 runs ascending: bn_sum_finish_kernel (the statistics merge
//                    (n, mean, M2) by Chan's rule in the same order: bn_stats_finish_kernel)
//   variance         never E[x^2] - E[x]^2: a workgroup takes its own mean first and then the centred squares about it (its rows
//                    come from L2 the second time), the workgroups' (n, mean, M2) are merged by Chan's rule
//   the slope        the channels' f64 totals (real channels only) are added in ascending channel order by the first wave of the
//                    elementwise launch's workgroup (0, 0): 64 lanes take contiguous runs of ceil(C_pad / 64) channels ascending,
//                    lane 0 then merges the 64 runs ascending
#include <initializer_list>

#include "tsod_internal.h"

namespace {

constexpr int kBnThreads = 256;
constexpr int kBnRows = TSOD_BN_ROWS_PER_WORKGROUP;
constexpr int kBnFinishChannels = 16, kBnFinishRuns = kBnThreads / kBnFinishChannels;
constexpr int kSlopeRuns = 64;

// channel quads across a workgroup: the power of two that covers C4, at most 64 (then blockIdx.y walks chunks of 64 quads)
__host__ __device__ inline int bn_quads_across(int C4) {
    int q = 1;
    while (q < C4 && q < 64) q <<= 1;
    return q;
}
inline long bn_row_blocks(long M) { return (M + kBnRows - 1) / kBnRows; }
inline dim3 bn_grid(long M, int C4) { return dim3((unsigned)bn_row_blocks(M), (unsigned)tsod_cdiv(C4, bn_quads_across(C4))); }

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

// ---------------------------------------------------------------------------------------------------------------- stats
// part [B][2][C_pad] doubles: the workgroup's mean and the centred sum of squares about it, per channel
__global__ void __launch_bounds__(kBnThreads)
bn_stats_partial_kernel(const float *__restrict__ z, long M, int C4, int ld, int off, double *__restrict__ part) {
    __shared__ double lds[4 * kBnThreads];
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    const float *col = z + off + 4 * (t.live ? t.q : 0);
    double s[4] = {0., 0., 0., 0.};
    if (t.live) {
#pragma unroll 4
        for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
            const float4 v = *reinterpret_cast<const float4 *>(col + m * ld);
            s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
        }
    }
    bn_block_sum<4>(s, lds, threadIdx.x, qx);
    const double n = (double)(t.m1 - t.m0);
    const double mu[4] = {s[0] / n, s[1] / n, s[2] / n, s[3] / n};
    double d2[4] = {0., 0., 0., 0.};
    if (t.live) {
#pragma unroll 4
        for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
            const float4 v = *reinterpret_cast<const float4 *>(col + m * ld);
            const double a = (double)v.x - mu[0], b = (double)v.y - mu[1], c = (double)v.z - mu[2], d = (double)v.w - mu[3];
            d2[0] += a * a; d2[1] += b * b; d2[2] += c * c; d2[3] += d * d;
        }
    }
    bn_block_sum<4>(d2, lds, threadIdx.x, qx);
    if (t.live && t.ry == 0) {
        const long C_pad = 4L * C4;
        double *dst = part + (long)blockIdx.x * 2 * C_pad + 4 * t.q;
#pragma unroll
        for (int e = 0; e < 4; ++e) { dst[e] = mu[e]; dst[C_pad + e] = d2[e]; }
    }
}

struct bn_moments { double n, mean, m2; };
// Chan's rule: (a then b); a.n may be 0
__device__ __forceinline__ void bn_merge(bn_moments &a, double nb, double mb, double qb) {
    const double nn = a.n + nb;
    const double delta = mb - a.mean;
    a.mean += delta * (nb / nn);
    a.m2 += qb + delta * delta * (a.n * nb / nn);
    a.n = nn;
}

__global__ void __launch_bounds__(kBnThreads)
bn_stats_finish_kernel(const double *__restrict__ part, long M, long B, int C_real, int C_pad, const float *__restrict__ gamma,
                       const float *__restrict__ beta, double eps, double momentum, float *__restrict__ running_mean,
                       float *__restrict__ running_var, long long *__restrict__ num_batches_tracked, float *__restrict__ mean,
                       float *__restrict__ invstd, float *__restrict__ scale, float *__restrict__ shift) {
    __shared__ double lds[3 * kBnThreads];
    const int tid = threadIdx.x;
    const int cl = tid % kBnFinishChannels, run = tid / kBnFinishChannels;
    const int c = blockIdx.x * kBnFinishChannels + cl;
    const long per = (B + kBnFinishRuns - 1) / kBnFinishRuns;
    const long b0 = run * per, b1 = b0 + per < B ? b0 + per : B;
    bn_moments acc = {0., 0., 0.};
    if (c < C_real) {
        for (long b = b0; b < b1; ++b) {
            const long rows = (b + 1) * kBnRows <= M ? kBnRows : M - b * kBnRows;
            bn_merge(acc, (double)rows, part[(2 * b) * C_pad + c], part[(2 * b + 1) * C_pad + c]);
        }
    }
    lds[tid] = acc.n; lds[kBnThreads + tid] = acc.mean; lds[2 * kBnThreads + tid] = acc.m2;
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0 && num_batches_tracked) *num_batches_tracked += 1;
    if (run != 0 || c >= C_pad) return;
    if (c >= C_real) {                                                  // pad channels: exact zeros
        mean[c] = invstd[c] = scale[c] = shift[c] = scale[C_pad + c] = shift[C_pad + c] = 0.f;
        return;
    }
    for (int r = 1; r < kBnFinishRuns; ++r) {
        const int o = r * kBnFinishChannels + cl;
        if (lds[o] > 0.) bn_merge(acc, lds[o], lds[kBnThreads + o], lds[2 * kBnThreads + o]);
    }
    const double var = acc.m2 / (double)M;
    const double inv = 1. / sqrt(var + eps);
    const double sc = (double)gamma[c] * inv;
    mean[c] = (float)acc.mean;
    invstd[c] = (float)inv;
    // scale and shift as f32 value + f32 remainder: with |mean| invstd >> 1 the two terms of scale * z + shift cancel, and one
    // f32 each would leave ulp(mean * scale) in y (mean 1e3, two rows: 1e-2 of max |y|)
    const double sh = (double)beta[c] - acc.mean * sc;
    scale[c] = (float)sc;
    scale[C_pad + c] = (float)(sc - (double)scale[c]);
    shift[c] = (float)sh;
    shift[C_pad + c] = (float)(sh - (double)shift[c]);
    if (running_mean) running_mean[c] = (float)((1. - momentum) * (double)running_mean[c] + momentum * acc.mean);
    if (running_var) running_var[c] = (float)((1. - momentum) * (double)running_var[c] + momentum * (acc.m2 / (double)(M - 1)));
}

// ---------------------------------------------------------------------------------------------------------------- apply
// kAct: TSOD_ACT_NONE, TSOD_ACT_RELU6 or TSOD_ACT_PRELU (slope).  kR: 0 nothing, 1 the residual tensor r, 2 the second
// normalised operand (r is then its z2).
template <int kAct, int kR>
__global__ void __launch_bounds__(kBnThreads)
bn_apply_kernel(const float *__restrict__ z, long M, int C4, int C_real, int z_ld, int z_off, const float *__restrict__ scale,
                const float *__restrict__ shift, const float *__restrict__ r, int r_ld, int r_off, const float *__restrict__ scale2,
                const float *__restrict__ shift2, float slope, float *__restrict__ y, int y_ld, int y_off, unsigned *amax_out) {
    __shared__ float s_amax[kBnThreads / 64];
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    float amax = 0.f;
    if (t.live) {
        const int c = 4 * t.q;
        const int C_pad = 4 * C4;
        double a[4], b[4], a2[4] = {0., 0., 0., 0.}, b2[4] = {0., 0., 0., 0.};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[e] = (double)scale[c + e] + (double)scale[C_pad + c + e];
            b[e] = (double)shift[c + e] + (double)shift[C_pad + c + e];
            if constexpr (kR == 2) {
                a2[e] = (double)scale2[c + e] + (double)scale2[C_pad + c + e];
                b2[e] = (double)shift2[c + e] + (double)shift2[C_pad + c + e];
            }
        }
        const float *src = z + z_off + c;
        const float *res = kR != 0 ? r + r_off + c : nullptr;
        float *dst = y + y_off + c;
#pragma unroll 4
        for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
            const float4 v = *reinterpret_cast<const float4 *>(src + m * z_ld);
            const float zq[4] = {v.x, v.y, v.z, v.w};
            float rq[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (kR != 0) {
                const float4 w = *reinterpret_cast<const float4 *>(res + m * r_ld);
                rq[0] = w.x; rq[1] = w.y; rq[2] = w.z; rq[3] = w.w;
            }
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double s = a[e] * (double)zq[e] + b[e];
                if constexpr (kR == 1) s += (double)rq[e];
                if constexpr (kR == 2) s += a2[e] * (double)rq[e] + b2[e];
                o[e] = (float)s;
                if constexpr (kAct == TSOD_ACT_RELU6) o[e] = fminf(fmaxf(o[e], 0.f), 6.f);
                if constexpr (kAct == TSOD_ACT_PRELU) o[e] = o[e] > 0.f ? o[e] : slope * o[e];
                if (c + e >= C_real) o[e] = 0.f;
                amax = fmaxf(amax, fabsf(o[e]));
            }
            *reinterpret_cast<float4 *>(dst + m * y_ld) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    if (amax_out != nullptr) tsod_amax_commit(amax_out, amax, s_amax, threadIdx.x, kBnThreads);
}

// ----------------------------------------------------------------------------------------------------------------- grad
// kFromY false: dy is g itself (y, slope unused), two planes.  kFromY true: g = dy * (y > 0 ? 1 : slope) from the saved output y,
// and a third plane for the slope.  What the planes, the LDS and the unroll are per instantiation:
template <bool kFromY> constexpr int kBnGradPlanes = kFromY ? 3 : 2;
template <bool kFromY> constexpr int kBnGradUnroll = kFromY ? 8 : 4;

// part [B][planes][C_pad] doubles: the workgroup's sum of g xhat, of g and (kFromY) of dy y [y < 0], per channel
template <bool kFromY>
__global__ void __launch_bounds__(kBnThreads)
bn_grad_partial_kernel(const float *__restrict__ y, int y_ld, int y_off, const float *__restrict__ dy, int dy_ld, int dy_off,
                       const float *__restrict__ z, int z_ld, int z_off, long M, int C4, const float *__restrict__ mean,
                       const float *__restrict__ invstd, float slope, double *__restrict__ part) {
    constexpr int kPlanes = kBnGradPlanes<kFromY>, kUnroll = kBnGradUnroll<kFromY>;
    __shared__ double lds[4 * kPlanes * kBnThreads];
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    double s[4 * kPlanes];                                              // [0, 4): sum g xhat, [4, 8): sum g, [8, 12): the slope's
#pragma unroll
    for (int e = 0; e < 4 * kPlanes; ++e) s[e] = 0.;
    if (t.live) {
        const int c = 4 * t.q;
        double mu[4], iv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { mu[e] = (double)mean[c + e]; iv[e] = (double)invstd[c + e]; }
        const float *yc = kFromY ? y + y_off + c : nullptr, *dc = dy + dy_off + c, *zc = z + z_off + c;
#pragma unroll kUnroll
        for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
            float4 yv = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (kFromY) yv = *reinterpret_cast<const float4 *>(yc + m * y_ld);
            const float4 dv = *reinterpret_cast<const float4 *>(dc + m * dy_ld);
            const float4 zv = *reinterpret_cast<const float4 *>(zc + m * z_ld);
            // (spelled out: the same loads through a helper that fills a float (&)[4] cost kFromY's instantiation 100 VGPR)
            const float yq[4] = {yv.x, yv.y, yv.z, yv.w}, dq[4] = {dv.x, dv.y, dv.z, dv.w}, zq[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float g = dq[e];
                if constexpr (kFromY) g = yq[e] > 0.f ? dq[e] : slope * dq[e];
                s[e] += (double)g * (((double)zq[e] - mu[e]) * iv[e]);
                s[4 + e] += (double)g;
                if constexpr (kFromY) s[8 + e] += yq[e] < 0.f ? (double)dq[e] * (double)yq[e] : 0.;
            }
        }
    }
    bn_block_sum<4 * kPlanes>(s, lds, threadIdx.x, qx);
    if (t.live && t.ry == 0) {
        const long C_pad = 4L * C4;
        double *dst = part + (long)blockIdx.x * kPlanes * C_pad + 4 * t.q;
#pragma unroll
        for (int p = 0; p < kPlanes; ++p) {
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[p * C_pad + e] = s[4 * p + e];
        }
    }
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

// dz = gamma invstd (g - dbeta / M - xhat dgamma / M) over channels [c, c + 4) of a thread's quad; total = [sum g xhat | sum g |
// ...][C_pad]; pad channels: exact zeros.  kFromY as above; kGOut: g is also stored (pad channels zero).  With kFromY, workgroup
// (0, 0) first adds up the slope's plane where dslope_num is asked for.
template <bool kFromY, bool kGOut>
__global__ void __launch_bounds__(kBnThreads)
bn_grad_dz_kernel(const float *__restrict__ y, int y_ld, int y_off, const float *__restrict__ dy, int dy_ld, int dy_off,
                  const float *__restrict__ z, int z_ld, int z_off, long M, int C4, int C_real, const float *__restrict__ mean,
                  const float *__restrict__ invstd, const float *__restrict__ gamma, float slope, const double *__restrict__ total,
                  float *__restrict__ dz, int dz_ld, int dz_off, float *__restrict__ g_out, int g_ld, int g_off,
                  float *__restrict__ dslope_num) {
    static_assert(kFromY || !kGOut, "g is stored only where it is formed here");
    constexpr int kUnroll = kBnGradUnroll<kFromY>;
    const int C_pad = 4 * C4;
    if constexpr (kFromY) {
        __shared__ double s_runs[kSlopeRuns];
        if (dslope_num != nullptr && blockIdx.x == 0 && blockIdx.y == 0) {  // (uniform over the workgroup: the barrier is legal)
            double ss = 0.;
            if (threadIdx.x < kSlopeRuns) {
                const int per = (C_pad + kSlopeRuns - 1) / kSlopeRuns;
                const int c0 = threadIdx.x * per, c1 = c0 + per < C_real ? c0 + per : C_real;
                for (int c = c0; c < c1; ++c) ss += total[2 * C_pad + c];
                s_runs[threadIdx.x] = ss;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int r = 1; r < kSlopeRuns; ++r) ss += s_runs[r];
                *dslope_num = (float)ss;
            }
        }
    }
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    if (!t.live) return;
    const int c = 4 * t.q;
    double mu[4], iv[4], k[4], a[4], b[4];                              // k: gamma invstd, 0 at pad channels
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mu[e] = (double)mean[c + e];
        iv[e] = (double)invstd[c + e];
        k[e] = c + e < C_real ? (double)gamma[c + e] * iv[e] : 0.;
        b[e] = total[c + e] / (double)M;
        a[e] = total[C_pad + c + e] / (double)M;
    }
    const float *yc = kFromY ? y + y_off + c : nullptr, *dc = dy + dy_off + c, *zc = z + z_off + c;
    float *oc = dz + dz_off + c;
    float *gc = kGOut ? g_out + g_off + c : nullptr;
#pragma unroll kUnroll
    for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
        float4 yv = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (kFromY) yv = *reinterpret_cast<const float4 *>(yc + m * y_ld);
        const float4 dv = *reinterpret_cast<const float4 *>(dc + m * dy_ld);
        const float4 zv = *reinterpret_cast<const float4 *>(zc + m * z_ld);
        const float yq[4] = {yv.x, yv.y, yv.z, yv.w}, dq[4] = {dv.x, dv.y, dv.z, dv.w}, zq[4] = {zv.x, zv.y, zv.z, zv.w};
        float o[4], gq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool real = c + e < C_real;
            float g = dq[e];
            if constexpr (kFromY) g = yq[e] > 0.f ? dq[e] : slope * dq[e];
            const double xh = ((double)zq[e] - mu[e]) * iv[e];
            o[e] = real ? (float)(k[e] * ((double)g - a[e] - xh * b[e])) : 0.f;
            gq[e] = real ? g : 0.f;
        }
        *reinterpret_cast<float4 *>(oc + m * dz_ld) = make_float4(o[0], o[1], o[2], o[3]);
        if constexpr (kGOut) *reinterpret_cast<float4 *>(gc + m * g_ld) = make_float4(gq[0], gq[1], gq[2], gq[3]);
    }
}

// ------------------------------------------------------------------------------------------------------------ entry points
// A tensor's channel slice [off, off + C_pad) of rows of pitch ld.  An optional tensor that is absent (p null) passes both checks.
struct bn_slice { const void *p; int32_t ld, off; };
inline bool bn_slices_ok(int32_t C_pad, std::initializer_list<bn_slice> ts) {
    for (const bn_slice &t : ts)
        if (t.p != nullptr && !(t.off >= 0 && t.ld > 0 && (long)t.off + C_pad <= t.ld)) return false;
    return true;
}
inline bool bn_slices_aligned(std::initializer_list<bn_slice> ts) {
    for (const bn_slice &t : ts)
        if (t.p != nullptr && !(tsod_aligned16(t.p) && (t.ld & 3) == 0 && (t.off & 3) == 0)) return false;
    return true;
}
inline size_t bn_workspace_bytes(int64_t M, int32_t C_pad, int planes) {
    if (M < 2 || C_pad <= 0 || (C_pad & 3)) return 0;
    return (size_t)(bn_row_blocks(M) + 1) * planes * (size_t)C_pad * sizeof(double);
}

// Both apply entry points.  act: TSOD_ACT_NONE, TSOD_ACT_RELU6, TSOD_ACT_PRELU, or -1 for one its entry point does not take.
int bn_apply(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t z_ld, int32_t z_off, const float *scale,
             const float *shift, int32_t act, const float *r, int32_t r_ld, int32_t r_off, const float *z2, int32_t z2_ld,
             int32_t z2_off, const float *scale2, const float *shift2, float slope, float *y, int32_t y_ld, int32_t y_off,
             uint32_t *amax_out, tsod_stream_t stream) {
    TSOD_REQUIRE(z && scale && shift && y, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(!(r && z2) && (z2 == nullptr || (scale2 && shift2)), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(C_pad > 0 && (C_pad & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(M >= 1 && C_real > 0 && C_real <= C_pad &&
                     bn_slices_ok(C_pad, {{z, z_ld, z_off}, {y, y_ld, y_off}, {r, r_ld, r_off}, {z2, z2_ld, z2_off}}),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(act >= 0, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(bn_slices_aligned({{z, z_ld, z_off}, {y, y_ld, y_off}, {scale, 0, 0}, {shift, 0, 0}, {r, r_ld, r_off},
                                    {z2, z2_ld, z2_off}, {z2 ? scale2 : nullptr, 0, 0}, {z2 ? shift2 : nullptr, 0, 0}}) &&
                     (amax_out == nullptr || (reinterpret_cast<uintptr_t>(amax_out) & 63u) == 0),
                 TSOD_ERR_ALIGNMENT);
    auto kernel = act == TSOD_ACT_NONE    ? &bn_apply_kernel<TSOD_ACT_NONE, 0>
                  : act == TSOD_ACT_RELU6 ? &bn_apply_kernel<TSOD_ACT_RELU6, 0>
                  : z2 != nullptr         ? &bn_apply_kernel<TSOD_ACT_PRELU, 2>
                  : r != nullptr          ? &bn_apply_kernel<TSOD_ACT_PRELU, 1>
                                          : &bn_apply_kernel<TSOD_ACT_PRELU, 0>;
    hipLaunchKernelGGL(kernel, bn_grid(M, C_pad / 4), dim3(kBnThreads), 0, tsod_stream(stream), z, (long)M, C_pad / 4, C_real, z_ld,
                       z_off, scale, shift, z2 ? z2 : r, z2 ? z2_ld : r_ld, z2 ? z2_off : r_off, scale2, shift2, slope, y, y_ld, y_off,
                       amax_out);
    return tsod_launch_status();
}

// Both gradient entry points: the group of three launches (partial, finish, dz).  y null: dy is g itself, two planes.
int bn_train_grad(const float *y, int32_t y_ld, int32_t y_off, const float *dy, int32_t dy_ld, int32_t dy_off, const float *z,
                  int32_t z_ld, int32_t z_off, int64_t M, int32_t C_real, int32_t C_pad, const float *mean, const float *invstd,
                  const float *gamma, float slope, float *dz, int32_t dz_ld, int32_t dz_off, float *dgamma, float *dbeta,
                  float *dslope_num, float *g_out, int32_t g_ld, int32_t g_off, void *workspace, size_t workspace_bytes,
                  tsod_stream_t stream) {
    const bool from_y = y != nullptr;
    const int planes = from_y ? 3 : 2;
    TSOD_REQUIRE(dy && z && mean && invstd && gamma && dz && dgamma && dbeta, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(C_pad > 0 && (C_pad & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(M >= 2 && C_real > 0 && C_real <= C_pad &&
                     bn_slices_ok(C_pad, {{y, y_ld, y_off}, {dy, dy_ld, dy_off}, {z, z_ld, z_off}, {dz, dz_ld, dz_off},
                                          {g_out, g_ld, g_off}}),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(bn_slices_aligned({{y, y_ld, y_off}, {dy, dy_ld, dy_off}, {z, z_ld, z_off}, {dz, dz_ld, dz_off},
                                    {g_out, g_ld, g_off}, {mean, 0, 0}, {invstd, 0, 0}}),
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= bn_workspace_bytes(M, C_pad, planes), TSOD_ERR_WORKSPACE);
    const long B = bn_row_blocks(M);
    double *part = static_cast<double *>(workspace);
    double *total = part + B * planes * (long)C_pad;
    hipStream_t st = tsod_stream(stream);
    const dim3 grid = bn_grid(M, C_pad / 4), block(kBnThreads);
    auto partial = from_y ? &bn_grad_partial_kernel<true> : &bn_grad_partial_kernel<false>;
    auto finish = from_y ? &bn_sum_finish_kernel<3> : &bn_sum_finish_kernel<2>;
    auto elementwise = !from_y  ? &bn_grad_dz_kernel<false, false>
                       : g_out  ? &bn_grad_dz_kernel<true, true>
                                : &bn_grad_dz_kernel<true, false>;
    hipLaunchKernelGGL(partial, grid, block, 0, st, y, y_ld, y_off, dy, dy_ld, dy_off, z, z_ld, z_off, (long)M, C_pad / 4, mean, invstd,
                       slope, part);
    hipLaunchKernelGGL(finish, dim3((unsigned)tsod_cdiv(C_pad, kBnFinishChannels)), block, 0, st, (const double *)part, B, C_real,
                       C_pad, total, dgamma, dbeta);
    hipLaunchKernelGGL(elementwise, grid, block, 0, st, y, y_ld, y_off, dy, dy_ld, dy_off, z, z_ld, z_off, (long)M, C_pad / 4, C_real,
                       mean, invstd, gamma, slope, (const double *)total, dz, dz_ld, dz_off, g_out, g_ld, g_off, dslope_num);
    return tsod_launch_status();
}

}  // namespace

extern "C" size_t tsod_bn_train_workspace_bytes(int64_t M, int32_t C_pad) { return bn_workspace_bytes(M, C_pad, 2); }
extern "C" size_t tsod_bn_prelu_train_grad_workspace_bytes(int64_t M, int32_t C_pad) { return bn_workspace_bytes(M, C_pad, 3); }

extern "C" int tsod_bn_stats_f32(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t ld, int32_t off,
                                 const float *gamma, const float *beta, double eps, double momentum, float *running_mean,
                                 float *running_var, int64_t *num_batches_tracked, float *mean, float *invstd, float *scale,
                                 float *shift, void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(z && gamma && beta && mean && invstd && scale && shift, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(C_pad > 0 && (C_pad & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(M >= 2 && C_real > 0 && C_real <= C_pad && bn_slices_ok(C_pad, {{z, ld, off}}) && eps >= 0., TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(bn_slices_aligned({{z, ld, off}}), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= bn_workspace_bytes(M, C_pad, 2), TSOD_ERR_WORKSPACE);
    const long B = bn_row_blocks(M);
    double *part = static_cast<double *>(workspace);
    hipStream_t st = tsod_stream(stream);
    hipLaunchKernelGGL(bn_stats_partial_kernel, bn_grid(M, C_pad / 4), dim3(kBnThreads), 0, st, z, (long)M, C_pad / 4, ld, off, part);
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((unsigned)tsod_cdiv(C_pad, kBnFinishChannels)), dim3(kBnThreads), 0, st,
                       (const double *)part, (long)M, B, C_real, C_pad, gamma, beta, eps, momentum, running_mean, running_var,
                       reinterpret_cast<long long *>(num_batches_tracked), mean, invstd, scale, shift);
    return tsod_launch_status();
}

extern "C" int tsod_bn_apply_f32(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t z_ld, int32_t z_off,
                                 const float *scale, const float *shift, int32_t act, float *y, int32_t y_ld, int32_t y_off,
                                 uint32_t *amax_out, tsod_stream_t stream) {
    return bn_apply(z, M, C_real, C_pad, z_ld, z_off, scale, shift, act == TSOD_ACT_NONE || act == TSOD_ACT_RELU6 ? act : -1, nullptr, 0,
                    0, nullptr, 0, 0, nullptr, nullptr, 0.f, y, y_ld, y_off, amax_out, stream);
}

extern "C" int tsod_bn_apply_prelu_f32(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t z_ld, int32_t z_off,
                                       const float *scale, const float *shift, const float *r, int32_t r_ld, int32_t r_off,
                                       const float *z2, int32_t z2_ld, int32_t z2_off, const float *scale2, const float *shift2,
                                       float slope, float *y, int32_t y_ld, int32_t y_off, uint32_t *amax_out,
                                       tsod_stream_t stream) {
    return bn_apply(z, M, C_real, C_pad, z_ld, z_off, scale, shift, TSOD_ACT_PRELU, r, r_ld, r_off, z2, z2_ld, z2_off, scale2, shift2,
                    slope, y, y_ld, y_off, amax_out, stream);
}

extern "C" int tsod_bn_train_grad_f32(const float *g, int32_t g_ld, int32_t g_off, const float *z, int32_t z_ld, int32_t z_off,
                                      int64_t M, int32_t C_real, int32_t C_pad, const float *mean, const float *invstd,
                                      const float *gamma, float *dz, int32_t dz_ld, int32_t dz_off, float *dgamma, float *dbeta,
                                      void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    return bn_train_grad(nullptr, 0, 0, g, g_ld, g_off, z, z_ld, z_off, M, C_real, C_pad, mean, invstd, gamma, 1.f, dz, dz_ld, dz_off,
                         dgamma, dbeta, nullptr, nullptr, 0, 0, workspace, workspace_bytes, stream);
}

extern "C" int tsod_bn_prelu_train_grad_f32(const float *y, int32_t y_ld, int32_t y_off, const float *dy, int32_t dy_ld,
                                            int32_t dy_off, const float *z, int32_t z_ld, int32_t z_off, int64_t M, int32_t C_real,
                                            int32_t C_pad, const float *mean, const float *invstd, const float *gamma, float slope,
                                            float *dz, int32_t dz_ld, int32_t dz_off, float *dgamma, float *dbeta,
                                            float *dslope_num, float *g_out, int32_t g_ld, int32_t g_off, void *workspace,
                                            size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(y, TSOD_ERR_INVALID_ARG);
    return bn_train_grad(y, y_ld, y_off, dy, dy_ld, dy_off, z, z_ld, z_off, M, C_real, C_pad, mean, invstd, gamma, slope, dz, dz_ld,
                         dz_off, dgamma, dbeta, dslope_num, g_out, g_ld, g_off, workspace, workspace_bytes, stream);
}
