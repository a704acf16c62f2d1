// bn_prelu_train.hip -- what ResNet's Bottlenecks put behind a train-mode BatchNorm, on bn_train.hip's
// rows, grid and summation rules (bn_rows.h):
//
//   tsod_bn_apply_prelu_f32        y = prelu(scale * z + shift + R, slope), R nothing, a residual tensor r, or a second
//                                  normalised operand scale2 * z2 + shift2; the terms are added in f64 and rounded to f32 once,
//                                  the PReLU runs on that f32; the destination's range words
//   tsod_bn_prelu_train_grad_f32   tsod_prelu_grad_f32 and tsod_bn_train_grad_f32 as one group of three launches: g = dy * (y > 0
//                                  ? 1 : slope) is made from the saved output y where it is used and written out only on request
//                                  (g_out), the slope's sum dy * y * [y < 0] rides along with the BatchNorm's two sums
//
// The sums are f64 with no float atomics, in an order the shape alone fixes (bn_rows.h: in a workgroup, across them), and
//   the slope        the channels' f64 totals (real channels only) are added in ascending channel order by the first wave of the
//                    elementwise launch's workgroup (0, 0): 64 lanes take contiguous runs of ceil(C_pad / 64) channels ascending,
//                    lane 0 then merges the 64 runs ascending
#include "bn_rows.h"

namespace {

constexpr int kSlopeRuns = 64;

// ---------------------------------------------------------------------------------------------------------------- apply
// kR: 0 nothing, 1 the residual tensor r, 2 the second normalised operand
template <int kR>
__global__ void __launch_bounds__(kBnThreads)
bn_apply_prelu_kernel(const float *__restrict__ z, long M, int C4, int C_real, int z_ld, int z_off, const float *__restrict__ scale,
                      const float *__restrict__ shift, const float *__restrict__ r, int r_ld, int r_off,
                      const float *__restrict__ scale2, const float *__restrict__ shift2, float slope, float *__restrict__ y, int y_ld,
                      int y_off, unsigned *amax_out) {
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
            if (kR == 2) {
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
            if (kR != 0) {
                const float4 w = *reinterpret_cast<const float4 *>(res + m * r_ld);
                rq[0] = w.x; rq[1] = w.y; rq[2] = w.z; rq[3] = w.w;
            }
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double s = a[e] * (double)zq[e] + b[e];
                if (kR == 1) s += (double)rq[e];
                if (kR == 2) s += a2[e] * (double)rq[e] + b2[e];
                o[e] = (float)s;
                o[e] = o[e] > 0.f ? o[e] : slope * o[e];
                if (c + e >= C_real) o[e] = 0.f;
                amax = fmaxf(amax, fabsf(o[e]));
            }
            *reinterpret_cast<float4 *>(dst + m * y_ld) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    if (amax_out != nullptr) tsod_amax_commit(amax_out, amax, s_amax, threadIdx.x, kBnThreads);
}

// ----------------------------------------------------------------------------------------------------------------- grad
// part [B][3][C_pad] doubles: the workgroup's sum of g xhat, of g and of dy y [y < 0], per channel
__global__ void __launch_bounds__(kBnThreads)
bn_prelu_grad_partial_kernel(const float *__restrict__ y, int y_ld, int y_off, const float *__restrict__ dy, int dy_ld, int dy_off,
                             const float *__restrict__ z, int z_ld, int z_off, long M, int C4, const float *__restrict__ mean,
                             const float *__restrict__ invstd, float slope, double *__restrict__ part) {
    __shared__ double lds[12 * kBnThreads];
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    double s[12] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};  // [0, 4): sum g xhat, [4, 8): sum g, [8, 12): the slope's
    if (t.live) {
        const int c = 4 * t.q;
        double mu[4], iv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { mu[e] = (double)mean[c + e]; iv[e] = (double)invstd[c + e]; }
        const float *yc = y + y_off + c, *dc = dy + dy_off + c, *zc = z + z_off + c;
#pragma unroll 8
        for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
            const float4 yv = *reinterpret_cast<const float4 *>(yc + m * y_ld);
            const float4 dv = *reinterpret_cast<const float4 *>(dc + m * dy_ld);
            const float4 zv = *reinterpret_cast<const float4 *>(zc + m * z_ld);
            const float yq[4] = {yv.x, yv.y, yv.z, yv.w}, dq[4] = {dv.x, dv.y, dv.z, dv.w}, zq[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = yq[e] > 0.f ? dq[e] : slope * dq[e];
                s[e] += (double)g * (((double)zq[e] - mu[e]) * iv[e]);
                s[4 + e] += (double)g;
                s[8 + e] += yq[e] < 0.f ? (double)dq[e] * (double)yq[e] : 0.;
            }
        }
    }
    bn_block_sum<12>(s, lds, threadIdx.x, qx);
    if (t.live && t.ry == 0) {
        const long C_pad = 4L * C4;
        double *dst = part + (long)blockIdx.x * 3 * C_pad + 4 * t.q;
#pragma unroll
        for (int e = 0; e < 4; ++e) { dst[e] = s[e]; dst[C_pad + e] = s[4 + e]; dst[2 * C_pad + e] = s[8 + e]; }
    }
}

template <bool kGOut>
__global__ void __launch_bounds__(kBnThreads)
bn_prelu_grad_dz_kernel(const float *__restrict__ y, int y_ld, int y_off, const float *__restrict__ dy, int dy_ld, int dy_off,
                        const float *__restrict__ z, int z_ld, int z_off, long M, int C4, int C_real, const float *__restrict__ mean,
                        const float *__restrict__ invstd, const float *__restrict__ gamma, float slope,
                        const double *__restrict__ total, float *__restrict__ dz, int dz_ld, int dz_off, float *__restrict__ g_out,
                        int g_ld, int g_off, float *__restrict__ dslope_num) {
    __shared__ double s_runs[kSlopeRuns];
    const int C_pad = 4 * C4;
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
    const int qx = bn_quads_across(C4);
    const bn_lane t = bn_lane_of(M, C4, qx);
    if (!t.live) return;
    const int c = 4 * t.q;
    const bn_dz_quad q = bn_dz_quad_of(mean, invstd, gamma, total, M, C_real, C_pad, c);
    const float *yc = y + y_off + c, *dc = dy + dy_off + c, *zc = z + z_off + c;
    float *oc = dz + dz_off + c;
    float *gc = kGOut ? g_out + g_off + c : nullptr;
#pragma unroll 8
    for (long m = t.m0 + t.ry; m < t.m1; m += t.rows_step) {
        const float4 yv = *reinterpret_cast<const float4 *>(yc + m * y_ld);
        const float4 dv = *reinterpret_cast<const float4 *>(dc + m * dy_ld);
        const float4 zv = *reinterpret_cast<const float4 *>(zc + m * z_ld);
        const float yq[4] = {yv.x, yv.y, yv.z, yv.w}, dq[4] = {dv.x, dv.y, dv.z, dv.w}, zq[4] = {zv.x, zv.y, zv.z, zv.w};
        float o[4], gq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool real = c + e < C_real;
            const float g = yq[e] > 0.f ? dq[e] : slope * dq[e];
            o[e] = real ? bn_dz_of(q, e, g, zq[e]) : 0.f;
            gq[e] = real ? g : 0.f;
        }
        *reinterpret_cast<float4 *>(oc + m * dz_ld) = make_float4(o[0], o[1], o[2], o[3]);
        if (kGOut) *reinterpret_cast<float4 *>(gc + m * g_ld) = make_float4(gq[0], gq[1], gq[2], gq[3]);
    }
}

}  // namespace

extern "C" size_t tsod_bn_prelu_train_grad_workspace_bytes(int64_t M, int32_t C_pad) {
    if (M < 2 || C_pad <= 0 || (C_pad & 3)) return 0;
    return (size_t)(bn_row_blocks(M) + 1) * 3 * (size_t)C_pad * sizeof(double);
}

extern "C" int tsod_bn_apply_prelu_f32(const float *z, int64_t M, int32_t C_real, int32_t C_pad, int32_t z_ld, int32_t z_off,
                                       const float *scale, const float *shift, const float *r, int32_t r_ld, int32_t r_off,
                                       const float *z2, int32_t z2_ld, int32_t z2_off, const float *scale2, const float *shift2,
                                       float slope, float *y, int32_t y_ld, int32_t y_off, uint32_t *amax_out,
                                       tsod_stream_t stream) {
    TSOD_REQUIRE(z && scale && shift && y, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(!(r && z2) && (z2 == nullptr || (scale2 && shift2)), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(C_pad > 0 && (C_pad & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(M >= 1 && C_real > 0 && C_real <= C_pad && bn_slice_ok(C_pad, z_ld, z_off) && bn_slice_ok(C_pad, y_ld, y_off) &&
                     (r == nullptr || bn_slice_ok(C_pad, r_ld, r_off)) && (z2 == nullptr || bn_slice_ok(C_pad, z2_ld, z2_off)),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(bn_slice_aligned(z, z_ld, z_off) && bn_slice_aligned(y, y_ld, y_off) && tsod_aligned16(scale) &&
                     tsod_aligned16(shift) && (r == nullptr || bn_slice_aligned(r, r_ld, r_off)) &&
                     (z2 == nullptr || (bn_slice_aligned(z2, z2_ld, z2_off) && tsod_aligned16(scale2) && tsod_aligned16(shift2))) &&
                     (amax_out == nullptr || (reinterpret_cast<uintptr_t>(amax_out) & 63u) == 0),
                 TSOD_ERR_ALIGNMENT);
    const dim3 grid = bn_grid(M, C_pad / 4);
    hipStream_t st = tsod_stream(stream);
    if (z2 != nullptr)
        hipLaunchKernelGGL(bn_apply_prelu_kernel<2>, grid, dim3(kBnThreads), 0, st, z, (long)M, C_pad / 4, C_real, z_ld, z_off, scale,
                           shift, z2, z2_ld, z2_off, scale2, shift2, slope, y, y_ld, y_off, amax_out);
    else if (r != nullptr)
        hipLaunchKernelGGL(bn_apply_prelu_kernel<1>, grid, dim3(kBnThreads), 0, st, z, (long)M, C_pad / 4, C_real, z_ld, z_off, scale,
                           shift, r, r_ld, r_off, (const float *)nullptr, (const float *)nullptr, slope, y, y_ld, y_off, amax_out);
    else
        hipLaunchKernelGGL(bn_apply_prelu_kernel<0>, grid, dim3(kBnThreads), 0, st, z, (long)M, C_pad / 4, C_real, z_ld, z_off, scale,
                           shift, (const float *)nullptr, 0, 0, (const float *)nullptr, (const float *)nullptr, slope, y, y_ld,
                           y_off, amax_out);
    return tsod_launch_status();
}

extern "C" int tsod_bn_prelu_train_grad_f32(const float *y, int32_t y_ld, int32_t y_off, const float *dy, int32_t dy_ld,
                                            int32_t dy_off, const float *z, int32_t z_ld, int32_t z_off, int64_t M, int32_t C_real,
                                            int32_t C_pad, const float *mean, const float *invstd, const float *gamma, float slope,
                                            float *dz, int32_t dz_ld, int32_t dz_off, float *dgamma, float *dbeta,
                                            float *dslope_num, float *g_out, int32_t g_ld, int32_t g_off, void *workspace,
                                            size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(y && dy && z && mean && invstd && gamma && dz && dgamma && dbeta, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(C_pad > 0 && (C_pad & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(M >= 2 && C_real > 0 && C_real <= C_pad && bn_slice_ok(C_pad, y_ld, y_off) && bn_slice_ok(C_pad, dy_ld, dy_off) &&
                     bn_slice_ok(C_pad, z_ld, z_off) && bn_slice_ok(C_pad, dz_ld, dz_off) &&
                     (g_out == nullptr || bn_slice_ok(C_pad, g_ld, g_off)), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(bn_slice_aligned(y, y_ld, y_off) && bn_slice_aligned(dy, dy_ld, dy_off) && bn_slice_aligned(z, z_ld, z_off) &&
                     bn_slice_aligned(dz, dz_ld, dz_off) && (g_out == nullptr || bn_slice_aligned(g_out, g_ld, g_off)) &&
                     tsod_aligned16(mean) && tsod_aligned16(invstd), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= tsod_bn_prelu_train_grad_workspace_bytes(M, C_pad),
                 TSOD_ERR_WORKSPACE);
    const long B = bn_row_blocks(M);
    double *part = static_cast<double *>(workspace);
    double *total = part + B * 3 * (long)C_pad;
    hipStream_t st = tsod_stream(stream);
    const dim3 grid = bn_grid(M, C_pad / 4);
    hipLaunchKernelGGL(bn_prelu_grad_partial_kernel, grid, dim3(kBnThreads), 0, st, y, y_ld, y_off, dy, dy_ld, dy_off, z, z_ld, z_off,
                       (long)M, C_pad / 4, mean, invstd, slope, part);
    hipLaunchKernelGGL(bn_sum_finish_kernel<3>, dim3((unsigned)tsod_cdiv(C_pad, kBnFinishChannels)), dim3(kBnThreads), 0, st,
                       (const double *)part, B, C_real, C_pad, total, dgamma, dbeta);
    auto dz_kernel = g_out != nullptr ? &bn_prelu_grad_dz_kernel<true> : &bn_prelu_grad_dz_kernel<false>;
    hipLaunchKernelGGL(dz_kernel, grid, dim3(kBnThreads), 0, st, y, y_ld, y_off, dy, dy_ld, dy_off, z, z_ld, z_off, (long)M, C_pad / 4,
                       C_real, mean, invstd, gamma, slope, (const double *)total, dz, dz_ld, dz_off, g_out, g_ld, g_off, dslope_num);
    return tsod_launch_status();
}
