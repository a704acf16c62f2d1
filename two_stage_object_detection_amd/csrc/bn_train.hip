// bn_train.hip -- train-mode BatchNorm over NHWC f32 rows:
//
//   tsod_bn_stats_f32        per-channel mean and biased variance of z [M][ld] (channels [off, off + C_pad)) -> mean, invstd,
//                            the folded scale = gamma * invstd and shift = beta - mean * scale, the running-statistics update
//   tsod_bn_apply_f32        y = act(scale * z + shift) with its own pitches / offsets and the destination's range words;
//                            scale and shift are [2][C_pad]: the f32 value and the f32 remainder of the f64 one, summed in f64
//   tsod_bn_train_grad_f32   dgamma = sum g xhat, dbeta = sum g, dz = gamma invstd (g - dbeta / M - xhat dgamma / M)
//
// All memory-bound: a workgroup owns kBnRows rows x (up to) 256 channels, a thread one channel quad (16-byte loads) and every
// RY-th row of the workgroup's rows.  The sums are kept in f64 (what that costs beside a copy of the same bytes is measured in
// DESIGN.md section 4.20, "Cost"): the statistics are then the correctly rounded f32 of the exact ones, which is what torch's CPU kernels give
// (their accumulation type for float is double); grad_reduce.h's f32 helpers are therefore not used here, its rule is: no float
// atomics, and every order depends on the shape only (bn_rows.h: in a workgroup, across them).  On top of that:
//   variance         never E[x^2] - E[x]^2: a workgroup takes its own mean first and then the centred squares about it (its rows
//                    come from L2 the second time), the workgroups' (n, mean, M2) are merged by Chan's rule
#include "bn_rows.h"

namespace {

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
__global__ void __launch_bounds__(kBnThreads)
bn_apply_kernel(const float *__restrict__ z, long M, int C4, int C_real, int z_ld, int z_off, const float *__restrict__ scale,
                const float *__restrict__ shift, int relu6, float *__restrict__ y, int y_ld, int y_off, unsigned *amax_out) {
    __shared__ float s_amax[kBnThreads / 64];
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    float amax = 0.f;
    if (t.live) {
        const int c = 4 * t.q;
        const int C_pad = 4 * C4;
        const float4 sc = *reinterpret_cast<const float4 *>(scale + c), scl = *reinterpret_cast<const float4 *>(scale + C_pad + c);
        const float4 sh = *reinterpret_cast<const float4 *>(shift + c), shl = *reinterpret_cast<const float4 *>(shift + C_pad + c);
        const double a[4] = {(double)sc.x + (double)scl.x, (double)sc.y + (double)scl.y, (double)sc.z + (double)scl.z,
                             (double)sc.w + (double)scl.w};
        const double b[4] = {(double)sh.x + (double)shl.x, (double)sh.y + (double)shl.y, (double)sh.z + (double)shl.z,
                             (double)sh.w + (double)shl.w};
        const float *src = z + z_off + c;
        float *dst = y + y_off + c;
#pragma unroll 4
        for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
            const float4 v = *reinterpret_cast<const float4 *>(src + m * z_ld);
            float o[4] = {(float)(a[0] * (double)v.x + b[0]), (float)(a[1] * (double)v.y + b[1]), (float)(a[2] * (double)v.z + b[2]),
                          (float)(a[3] * (double)v.w + b[3])};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (relu6) o[e] = fminf(fmaxf(o[e], 0.f), 6.f);
                if (c + e >= C_real) o[e] = 0.f;
                amax = fmaxf(amax, fabsf(o[e]));
            }
            *reinterpret_cast<float4 *>(dst + m * y_ld) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    if (amax_out != nullptr) tsod_amax_commit(amax_out, amax, s_amax, threadIdx.x, kBnThreads);
}

// ----------------------------------------------------------------------------------------------------------------- grad
// part [B][2][C_pad] doubles: the workgroup's sum of g xhat and of g, per channel
__global__ void __launch_bounds__(kBnThreads)
bn_grad_partial_kernel(const float *__restrict__ g, int g_ld, int g_off, const float *__restrict__ z, int z_ld, int z_off, long M,
                       int C4, const float *__restrict__ mean, const float *__restrict__ invstd, double *__restrict__ part) {
    __shared__ double lds[8 * kBnThreads];
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    double s[8] = {0., 0., 0., 0., 0., 0., 0., 0.};                    // [0, 4): sum g xhat, [4, 8): sum g
    if (t.live) {
        const int c = 4 * t.q;
        const float4 mu = *reinterpret_cast<const float4 *>(mean + c);
        const float4 iv = *reinterpret_cast<const float4 *>(invstd + c);
        const float *gc = g + g_off + c, *zc = z + z_off + c;
#pragma unroll 4
        for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
            const float4 gv = *reinterpret_cast<const float4 *>(gc + m * g_ld);
            const float4 zv = *reinterpret_cast<const float4 *>(zc + m * z_ld);
            s[0] += (double)gv.x * (((double)zv.x - (double)mu.x) * (double)iv.x);
            s[1] += (double)gv.y * (((double)zv.y - (double)mu.y) * (double)iv.y);
            s[2] += (double)gv.z * (((double)zv.z - (double)mu.z) * (double)iv.z);
            s[3] += (double)gv.w * (((double)zv.w - (double)mu.w) * (double)iv.w);
            s[4] += (double)gv.x; s[5] += (double)gv.y; s[6] += (double)gv.z; s[7] += (double)gv.w;
        }
    }
    bn_block_sum<8>(s, lds, threadIdx.x, qx);
    if (t.live && t.ry == 0) {
        const long C_pad = 4L * C4;
        double *dst = part + (long)blockIdx.x * 2 * C_pad + 4 * t.q;
#pragma unroll
        for (int e = 0; e < 4; ++e) { dst[e] = s[e]; dst[C_pad + e] = s[4 + e]; }
    }
}

__global__ void __launch_bounds__(kBnThreads)
bn_grad_dz_kernel(const float *__restrict__ g, int g_ld, int g_off, const float *__restrict__ z, int z_ld, int z_off, long M, int C4,
                  int C_real, const float *__restrict__ mean, const float *__restrict__ invstd, const float *__restrict__ gamma,
                  const double *__restrict__ total, float *__restrict__ dz, int dz_ld, int dz_off) {
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    if (!t.live) return;
    const int c = 4 * t.q;
    const bn_dz_quad q = bn_dz_quad_of(mean, invstd, gamma, total, M, C_real, 4 * C4, c);
    const float *gc = g + g_off + c, *zc = z + z_off + c;
    float *dc = dz + dz_off + c;
#pragma unroll 4
    for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
        const float4 gv = *reinterpret_cast<const float4 *>(gc + m * g_ld);
        const float4 zv = *reinterpret_cast<const float4 *>(zc + m * z_ld);
        const float gq[4] = {gv.x, gv.y, gv.z, gv.w}, zq[4] = {zv.x, zv.y, zv.z, zv.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = c + e < C_real ? bn_dz_of(q, e, gq[e], zq[e]) : 0.f;
        *reinterpret_cast<float4 *>(dc + m * dz_ld) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

}  // namespace

extern "C" size_t tsod_bn_train_workspace_bytes(int64_t M, int32_t C_pad) {
    if (M < 2 || C_pad <= 0 || (C_pad & 3)) return 0;
    return (size_t)(bn_row_blocks(M) + 1) * 2 * (size_t)C_pad * sizeof(double);
}

extern "C" int tsod_bn_stats_f32(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t ld, int32_t off,
                                 const float *gamma, const float *beta, double eps, double momentum, float *running_mean,
                                 float *running_var, int64_t *num_batches_tracked, float *mean, float *invstd, float *scale,
                                 float *shift, void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(z && gamma && beta && mean && invstd && scale && shift, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(C_pad > 0 && (C_pad & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(M >= 2 && C_real > 0 && C_real <= C_pad && bn_slice_ok(C_pad, ld, off) && eps >= 0., TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(bn_slice_aligned(z, ld, off), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= tsod_bn_train_workspace_bytes(M, C_pad),
                 TSOD_ERR_WORKSPACE);
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
    TSOD_REQUIRE(z && scale && shift && y, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(C_pad > 0 && (C_pad & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(M >= 1 && C_real > 0 && C_real <= C_pad && bn_slice_ok(C_pad, z_ld, z_off) && bn_slice_ok(C_pad, y_ld, y_off),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(act == TSOD_ACT_NONE || act == TSOD_ACT_RELU6, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(bn_slice_aligned(z, z_ld, z_off) && bn_slice_aligned(y, y_ld, y_off) && tsod_aligned16(scale) &&
                     tsod_aligned16(shift) && (amax_out == nullptr || (reinterpret_cast<uintptr_t>(amax_out) & 63u) == 0),
                 TSOD_ERR_ALIGNMENT);
    hipLaunchKernelGGL(bn_apply_kernel, bn_grid(M, C_pad / 4), dim3(kBnThreads), 0, tsod_stream(stream), z, (long)M, C_pad / 4,
                       C_real, z_ld, z_off, scale, shift, act == TSOD_ACT_RELU6 ? 1 : 0, y, y_ld, y_off, amax_out);
    return tsod_launch_status();
}

extern "C" int tsod_bn_train_grad_f32(const float *g, int32_t g_ld, int32_t g_off, const float *z, int32_t z_ld, int32_t z_off,
                                      int64_t M, int32_t C_real, int32_t C_pad, const float *mean, const float *invstd,
                                      const float *gamma, float *dz, int32_t dz_ld, int32_t dz_off, float *dgamma, float *dbeta,
                                      void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(g && z && mean && invstd && gamma && dz && dgamma && dbeta, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(C_pad > 0 && (C_pad & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(M >= 2 && C_real > 0 && C_real <= C_pad && bn_slice_ok(C_pad, g_ld, g_off) && bn_slice_ok(C_pad, z_ld, z_off) &&
                     bn_slice_ok(C_pad, dz_ld, dz_off), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(bn_slice_aligned(g, g_ld, g_off) && bn_slice_aligned(z, z_ld, z_off) && bn_slice_aligned(dz, dz_ld, dz_off) &&
                     tsod_aligned16(mean) && tsod_aligned16(invstd), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= tsod_bn_train_workspace_bytes(M, C_pad),
                 TSOD_ERR_WORKSPACE);
    const long B = bn_row_blocks(M);
    double *part = static_cast<double *>(workspace);
    double *total = part + B * 2 * (long)C_pad;
    hipStream_t st = tsod_stream(stream);
    const dim3 grid = bn_grid(M, C_pad / 4);
    hipLaunchKernelGGL(bn_grad_partial_kernel, grid, dim3(kBnThreads), 0, st, g, g_ld, g_off, z, z_ld, z_off, (long)M, C_pad / 4, mean,
                       invstd, part);
    hipLaunchKernelGGL(bn_sum_finish_kernel<2>, dim3((unsigned)tsod_cdiv(C_pad, kBnFinishChannels)), dim3(kBnThreads), 0, st,
                       (const double *)part, B, C_real, C_pad, total, dgamma, dbeta);
    hipLaunchKernelGGL(bn_grad_dz_kernel, grid, dim3(kBnThreads), 0, st, g, g_ld, g_off, z, z_ld, z_off, (long)M, C_pad / 4, C_real,
                       mean, invstd, gamma, (const double *)total, dz, dz_ld, dz_off);
    return tsod_launch_status();
}
