// pw_grads.hip -- the backward of a HarDNet 1x1 ConvLayer:
//
//   y[m][o] = relu6(scale[o] * sum_k w[o][k] x[m][k] + shift[o]),  x gathered from channel segments of an NHWC buffer
//
//   tsod_relu6_grad_mask_f32   g = dy * [0 < y < 6]                      (the standalone mask pass: transition layers)
//   tsod_pw_wgrad_f32          dWraw = g^T x_gathered on v_mfma_f32_32x32x2_f32 over M-slices, then one finishing launch:
//                              dW = scale * dWraw (pad rows / columns dropped), dscale = sum_k w * dWraw, dshift = sum_m g
//   tsod_pw_dgrad_f32          dx[seg] (+)= (g * scale) w[:, seg] on the same matrix cores, wanted segments only
//
// No float atomics.  The M-slices' partial tiles are added in slice order; slice count, in-workgroup trees and the k order of a
// row's dscale depend on the shape only, so results are bit-identical from run to run.
#include "grad_reduce.h"

namespace {

// gathered column k (over the padded segment widths, in segment order) -> channel of the buffer, or -1 past the end
__host__ __device__ inline int pw_buffer_column(const tsod_pw_segs &sg, int k) {
    int s0 = 0;
    for (int s = 0; s < sg.n_seg; ++s) {
        if (k < s0 + sg.len[s]) return sg.off[s] + (k - s0);
        s0 += sg.len[s];
    }
    return -1;
}
// gathered column k -> column of the dense [.., sum(real)] weight gradient, or -1 for a pad column
__device__ inline int pw_real_column(const tsod_pw_segs &sg, int k) {
    int s0 = 0, r0 = 0;
    for (int s = 0; s < sg.n_seg; ++s) {
        if (k < s0 + sg.len[s]) return k - s0 < sg.real[s] ? r0 + (k - s0) : -1;
        s0 += sg.len[s];
        r0 += sg.real[s];
    }
    return -1;
}

// ----------------------------------------------------------------------------------------------------------------- mask
__global__ void __launch_bounds__(256)
relu6_grad_mask_kernel(const float *__restrict__ y, long rows, int C4, int y_pitch, const float *__restrict__ dy, int dy_pitch,
                       int dy_off, float *__restrict__ g, int g_pitch) {
    const long total = rows * C4;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const long m = t / C4;
        const int c = 4 * (int)(t - m * C4);
        const float4 v = *reinterpret_cast<const float4 *>(y + m * y_pitch + c);
        const float4 d = *reinterpret_cast<const float4 *>(dy + m * dy_pitch + dy_off + c);
        *reinterpret_cast<float4 *>(g + m * g_pitch + c) = tsod_relu6_keep(d, v);
    }
}

// ---------------------------------------------------------------------------------------------------------------- wgrad
// grad_reduce.h's tile with a lane's 16-byte load of X going to the buffer channel its gathered k maps to; the slice count is
// also bounded by the operands (tsod_wgrad_plan_of's cap_by_operands).
__global__ void __launch_bounds__(kWgThreads)
pw_wgrad_partial_kernel(const float *__restrict__ g, long M, int N, int g_pitch, const float *__restrict__ x, int K, int x_pitch,
                        tsod_pw_segs sg, tsod_wgrad_plan sh, float *__restrict__ part, float *__restrict__ part_b) {
    __shared__ float lds[kWgLdsFloats];
    // segment widths are multiples of 4: a quad of gathered columns lies in one segment, or past K
    tsod_wgrad_tile(g, M, N, g_pitch, x, x_pitch, [&](int k) { return k < K ? pw_buffer_column(sg, k) : -1; }, sh, part, part_b,
                    lds);
}

// One workgroup per real output row o: grad_reduce.h's finish with the segments' pad columns dropped.
__global__ void __launch_bounds__(256)
pw_wgrad_finish_kernel(const float *__restrict__ part, const float *__restrict__ part_b, tsod_wgrad_plan sh, int K, int k_real,
                       tsod_pw_segs sg, const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ dw,
                       float *__restrict__ dscale, float *__restrict__ dshift) {
    __shared__ float lds[256];
    tsod_wgrad_finish_row(part, part_b, sh, K, k_real, [&](int k) { return pw_real_column(sg, k); }, w, scale, dw, dscale, dshift,
                          lds);
}

// ---------------------------------------------------------------------------------------------------------------- dgrad
// dx[m][col] (+)= sum_o (g[m][o] * scale[o]) * w[o][col] as D = A B on v_mfma_f32_32x32x2_f32: A = g * scale (32 m x 2 o: lane
// l holds row l & 31, o-half l >> 5), B = w (2 o x 32 columns: lane l holds column l & 31).  A workgroup of 4 waves owns 128
// rows x 128 columns of the WANTED segments' column space (segments nobody needs are not in it); a wave owns 32 rows and four
// 32-column accumulators.  Per 8 o: one 16-byte load of g and of scale per lane feeds 16 MFMAs (e = 0..3: o = o0 + 4 (l >> 5) +
// e), each with a 128-byte row segment of w per half wave; w stays in L2 (<= 4.3 MB).  No LDS.  o ascends, so an element's sum
// has one order; the old value is added last.  Pad columns of a segment are stored as exact zeros.
constexpr int kDgThreads = 256;
constexpr int kDgRows = 128, kDgCols = 128;

__global__ void __launch_bounds__(kDgThreads)
pw_dgrad_kernel(const float *__restrict__ g, long M, int N, int g_pitch, const float *__restrict__ w, int K,
                const float *__restrict__ scale, tsod_pw_segs sg, float *__restrict__ dx, int dx_pitch, int accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const long m0 = (long)blockIdx.y * kDgRows + 32 * wave;
    const int col0 = blockIdx.x * kDgCols;
    int wcol[4], dcol[4];
    bool pad[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + 32 * j + c;                              // in the wanted segments' column space
        wcol[j] = dcol[j] = -1;
        pad[j] = false;
        int k0 = 0, v0 = 0;
        for (int s = 0; s < sg.n_seg; ++s) {
            if (sg.want[s]) {
                if (col >= v0 && col < v0 + sg.len[s]) {
                    wcol[j] = k0 + (col - v0);
                    dcol[j] = sg.off[s] + (col - v0);
                    pad[j] = col - v0 >= sg.real[s];
                }
                v0 += sg.len[s];
            }
            k0 += sg.len[s];
        }
    }
    tsod_f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const long row = m0 + c;
    const bool row_ok = row < M;
    const float *grow = g + (row_ok ? row : 0) * g_pitch;
    for (int o0 = 0; o0 < N; o0 += 8) {
        const int oq = o0 + 4 * h;                                      // N % 4 == 0: the quad is all in or all out
        const bool o_ok = oq < N;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (o_ok && row_ok) {
            const float4 gq = *reinterpret_cast<const float4 *>(grow + oq);
            const float4 sq = *reinterpret_cast<const float4 *>(scale + oq);
            a[0] = gq.x * sq.x; a[1] = gq.y * sq.y; a[2] = gq.z * sq.z; a[3] = gq.w * sq.w;
        }
        float b[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) b[e][j] = (o_ok && wcol[j] >= 0) ? w[(long)(oq + e) * K + wcol[j]] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e][j], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (dcol[j] < 0) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long m = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m >= M) continue;
            float *dst = dx + m * dx_pitch + dcol[j];
            float v = acc[j][r];
            if (pad[j]) v = 0.f;
            else if (accumulate) v = *dst + v;
            *dst = v;
        }
    }
}

inline bool pw_segs_ok(const tsod_pw_segs *sg, int pitch, int *K, int *k_real, int *k_want) {
    if (!sg || sg->n_seg < 1 || sg->n_seg > TSOD_PW_MAX_SEGMENTS) return false;
    int k = 0, kr = 0, kw = 0;
    for (int s = 0; s < sg->n_seg; ++s) {
        if (sg->off[s] < 0 || sg->len[s] <= 0 || sg->real[s] <= 0 || sg->real[s] > sg->len[s]) return false;
        if (sg->off[s] + sg->len[s] > pitch) return false;
        k += sg->len[s];
        kr += sg->real[s];
        if (sg->want[s]) kw += sg->len[s];
    }
    *K = k; *k_real = kr; *k_want = kw;
    return true;
}
inline bool pw_segs_aligned(const tsod_pw_segs *sg) {
    for (int s = 0; s < sg->n_seg; ++s)
        if ((sg->off[s] & 3) || (sg->len[s] & 3)) return false;
    return true;
}

}  // namespace

extern "C" int tsod_relu6_grad_mask_f32(const float *y, int64_t rows, int32_t C, int32_t y_pitch, const float *dy,
                                        int32_t dy_pitch, int32_t dy_off, float *g, int32_t g_pitch, tsod_stream_t stream) {
    TSOD_REQUIRE(y && dy && g, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(rows > 0 && C > 0 && dy_off >= 0 && y_pitch >= C && dy_pitch >= dy_off + C && g_pitch >= C, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((C & 3) == 0 && (y_pitch & 3) == 0 && (dy_pitch & 3) == 0 && (dy_off & 3) == 0 && (g_pitch & 3) == 0,
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(y) && tsod_aligned16(dy) && tsod_aligned16(g), TSOD_ERR_ALIGNMENT);
    const long total = (long)rows * (C / 4);
    const unsigned blocks = (unsigned)(tsod_cdiv(total, 256) < 16384 ? tsod_cdiv(total, 256) : 16384);
    hipLaunchKernelGGL(relu6_grad_mask_kernel, dim3(blocks), dim3(256), 0, tsod_stream(stream), y, (long)rows, C / 4, y_pitch, dy,
                       dy_pitch, dy_off, g, g_pitch);
    return tsod_launch_status();
}

extern "C" size_t tsod_pw_wgrad_workspace_bytes(int64_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return tsod_wgrad_plan_bytes(tsod_wgrad_plan_of(M, N, K, true));
}

extern "C" int tsod_pw_wgrad_f32(const float *g, int64_t M, int32_t N, int32_t g_pitch, const float *x, int32_t x_pitch,
                                 const tsod_pw_segs *segs, const float *w, const float *scale, int32_t n_real, float *dw,
                                 float *dscale, float *dshift, void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(g && x && segs && w && scale && (dw || dscale || dshift), TSOD_ERR_INVALID_ARG);
    int K = 0, k_real = 0, k_want = 0;
    TSOD_REQUIRE(M > 0 && N > 0 && g_pitch >= N && n_real > 0 && n_real <= N && pw_segs_ok(segs, x_pitch, &K, &k_real, &k_want),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((x_pitch & 3) == 0 && pw_segs_aligned(segs) && tsod_aligned16(x), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= tsod_pw_wgrad_workspace_bytes(M, N, K),
                 TSOD_ERR_WORKSPACE);
    const tsod_wgrad_plan sh = tsod_wgrad_plan_of(M, N, K, true);
    TSOD_REQUIRE(sh.splits <= 65535, TSOD_ERR_UNSUPPORTED);
    float *part = static_cast<float *>(workspace);
    float *part_b = tsod_wgrad_plan_bias(sh, part);
    hipStream_t st = tsod_stream(stream);
    hipLaunchKernelGGL(pw_wgrad_partial_kernel, dim3(sh.n_tiles * sh.k_tiles, sh.splits), dim3(kWgThreads), 0, st, g, (long)M, N,
                       g_pitch, x, K, x_pitch, *segs, sh, part, part_b);
    hipLaunchKernelGGL(pw_wgrad_finish_kernel, dim3(n_real), dim3(256), 0, st, (const float *)part, (const float *)part_b, sh, K,
                       k_real, *segs, w, scale, dw, dscale, dshift);
    return tsod_launch_status();
}

extern "C" int tsod_pw_dgrad_f32(const float *g, int64_t M, int32_t N, int32_t g_pitch, const float *w, const float *scale,
                                 const tsod_pw_segs *segs, float *dx, int32_t dx_pitch, int32_t accumulate,
                                 tsod_stream_t stream) {
    TSOD_REQUIRE(g && w && scale && segs && dx, TSOD_ERR_INVALID_ARG);
    int K = 0, k_real = 0, k_want = 0;
    TSOD_REQUIRE(M > 0 && N > 0 && g_pitch >= N && pw_segs_ok(segs, dx_pitch, &K, &k_real, &k_want), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((N & 3) == 0 && (g_pitch & 3) == 0 && pw_segs_aligned(segs) && tsod_aligned16(g) && tsod_aligned16(scale),
                 TSOD_ERR_ALIGNMENT);
    if (k_want == 0) return TSOD_OK;                                     // nobody needs any segment: nothing is launched
    const long row_tiles = tsod_cdiv(M, kDgRows);
    TSOD_REQUIRE(row_tiles <= 65535, TSOD_ERR_UNSUPPORTED);
    hipLaunchKernelGGL(pw_dgrad_kernel, dim3((unsigned)tsod_cdiv(k_want, kDgCols), (unsigned)row_tiles), dim3(kDgThreads), 0,
                       tsod_stream(stream), g, (long)M, N, g_pitch, w, K, scale, *segs, dx, dx_pitch, accumulate ? 1 : 0);
    return tsod_launch_status();
}
