// conv_grads.hip -- what a ResNet Bottleneck's backward needs beside pw_grads.hip's 1x1 kernels:
//
//   y = prelu(z) with one slope a > 0, z = scale[o] * conv(x, w) + shift[o]   (the mask is taken from the saved y: sign(y) = sign(z))
//
//   tsod_prelu_grad_f32             g = dy * (y > 0 ? 1 : a), and the slope gradient's numerator sum dy * y * [y < 0]
//                                   (d a = that sum / a, because y = a z where z < 0)
//   tsod_conv3x3_dense_wgrad_f32    dWraw = g^T patches(x) of a dense 3x3 conv, pad 1, stride 1: grad_reduce.h's tile a third time,
//                                   the K = 9 C columns gathered from the nine shifted rows; then grad_reduce.h's finish:
//                                   dW = scale * dWraw, dscale = sum_k w * dWraw, dshift = sum_m g
//
//
// and what a projection Bottleneck (a stride on the 3x3, a strided 1x1 shortcut) adds to that:
//
//   (tsod_conv3x3_strided_wgrad_f32, the 3x3's wgrad over the output grid at stride 1 or 2, is conv_strided_grads.hip)
//   tsod_prelu_grad_d2s_f32         tsod_prelu_grad_f32 whose dy is gathered from the phase-stacked image P [N,OH+1,OW+1,4C] that
//                                   the forward conv library makes of g and the 2x2 phase pack (the stride-2 3x3's dx, never
//                                   written out): dy[n,ih,iw,c] = P[n, (ih>>1)+1, (iw>>1)+1, ((ih&1) 2 + (iw&1)) C + c]
//   tsod_pixel_subsample_f32        xs[n,oh,ow,:] = x[n, s oh, s ow, :]: the rows a strided 1x1 conv reads, for pw_grads.hip's wgrad
//   tsod_pixel_upsample_add_f32     dx[n, s oh, s ow, :] = dx[...] + d[n,oh,ow,:]: that conv's dx, added where it belongs
//
// The 3x3 conv's dx has no kernel here: it is the forward conv library run on g with the rotated, scaled weights.
// No float atomics; every order of additions is grad_reduce.h's and depends on the shape only.
#include "grad_reduce.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- PReLU
constexpr int kPreluMaxBlocks = 1024;

inline unsigned prelu_blocks(long rows, int C) {
    const long b = tsod_cdiv(rows * (C / 4), 256);
    return (unsigned)(b < kPreluMaxBlocks ? b : kPreluMaxBlocks);
}

// The body of both PReLU kernels.  dy_at(m, c): where the quad of dy that belongs to columns c .. c + 3 of y's row m lies.
// kSum: also this workgroup's part of sum dy * y * [y < 0] (grad_reduce.h: tsod_strided_sum_256), to partial[blockIdx.x].
// Index: unsigned where rows * C4 and the grid's stride fit 32 bits (one 32-bit division per quad), else long; the elements a
// thread visits and their order are the same.
template <bool kSum, class Index, class DyAt>
__device__ __forceinline__ void prelu_grad_body(const float *__restrict__ y, long rows, int C4, int y_pitch, DyAt dy_at, float slope,
                                                float *__restrict__ g, int g_pitch, float *__restrict__ partial, float *lds) {
    const Index total = (Index)(rows * C4), step = (Index)gridDim.x * 256;
    float sum = 0.f;
    for (Index t = (Index)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const Index mi = t / (Index)C4;
        const long m = (long)mi;
        const int c = 4 * (int)(t - mi * (Index)C4);
        const float4 v = *reinterpret_cast<const float4 *>(y + m * y_pitch + c);
        const float4 d = *reinterpret_cast<const float4 *>(dy_at(m, c));
        float4 o;
        o.x = v.x > 0.f ? d.x : slope * d.x;
        o.y = v.y > 0.f ? d.y : slope * d.y;
        o.z = v.z > 0.f ? d.z : slope * d.z;
        o.w = v.w > 0.f ? d.w : slope * d.w;
        *reinterpret_cast<float4 *>(g + m * g_pitch + c) = o;
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

template <bool kSum, class Index>
__global__ void __launch_bounds__(256)
prelu_grad_kernel(const float *__restrict__ y, long rows, int C4, int y_pitch, const float *__restrict__ dy, int dy_pitch,
                  int dy_off, float slope, float *__restrict__ g, int g_pitch, float *__restrict__ partial) {
    __shared__ float lds[256];
    prelu_grad_body<kSum, Index>(y, rows, C4, y_pitch, [=](long m, int c) { return dy + m * dy_pitch + dy_off + c; }, slope, g,
                                 g_pitch, partial, lds);
}

// y's row m is pixel (n, ih, iw) of [N,H,W]; its dy is the depth-to-space read of p [N,PH,PW,p_pitch] (PH = (H - 1) / 2 + 2, PW
// likewise): pixel ((ih >> 1) + 1, (iw >> 1) + 1), channels ((ih & 1) 2 + (iw & 1)) C + c.  (ih, iw) come from the row number by
// division; no shifted row number is ever tested against a range.  C % 4 == 0: a quad lies in one phase.
template <bool kSum, class Index>
__global__ void __launch_bounds__(256)
prelu_grad_d2s_kernel(const float *__restrict__ y, long rows, int C4, int y_pitch, int H, int W, const float *__restrict__ p,
                      int p_pitch, float slope, float *__restrict__ g, int g_pitch, float *__restrict__ partial) {
    __shared__ float lds[256];
    const int PH = (H - 1) / 2 + 2, PW = (W - 1) / 2 + 2, C = 4 * C4;
    prelu_grad_body<kSum, Index>(
        y, rows, C4, y_pitch,
        [=](long m, int c) {
            const unsigned mu = (unsigned)m;                          // rows < 2^31
            const unsigned row = mu / (unsigned)W, n = row / (unsigned)H;
            const int iw = (int)(mu - row * (unsigned)W), ih = (int)(row - n * (unsigned)H);
            const long pr = ((long)n * PH + (ih >> 1) + 1) * PW + (iw >> 1) + 1;
            return p + pr * p_pitch + ((ih & 1) * 2 + (iw & 1)) * C + c;
        },
        slope, g, g_pitch, partial, lds);
}

__global__ void __launch_bounds__(256)
prelu_grad_finish_kernel(const float *__restrict__ partial, int count, float *__restrict__ out) {
    __shared__ float lds[256];
    float sum = 0.f;
    for (int i = threadIdx.x; i < count; i += 256) sum += partial[i];
    const float s = tsod_tree_sum_256(sum, lds, threadIdx.x);
    if (threadIdx.x == 0) *out = s;
}

// ------------------------------------------------------------------------------------------------------- dense 3x3 wgrad
// Column k = (kh * 3 + kw) * C + c of dY's row m = (n, oh, ow) is channel c of pixel (n, oh + kh - 1, ow + kw - 1): row
// m + (kh - 1) W + (kw - 1) of x where that pixel is inside image n, else a zero.  The test is made on (oh, ow), never on the
// shifted row number: a shifted row that leaves the image is some other pixel's row, or another image's.  C % 4 == 0, so a
// lane's quad of columns lies in one tap.
__global__ void __launch_bounds__(kWgThreads)
conv3x3_dense_wgrad_partial_kernel(const float *__restrict__ g, int M, int Cout, int g_pitch, const float *__restrict__ x, int C,
                                   int x_pitch, int H, int W, tsod_wgrad_plan sh, float *__restrict__ part,
                                   float *__restrict__ part_b) {
    __shared__ float lds[kWgLdsFloats];
    const int K = 9 * C;
    tsod_wgrad_tile(
        g, (long)M, Cout, g_pitch, x, x_pitch, [=](int k) { return k < K ? k % C : -1; }, sh, part, part_b, lds,
        [=](long m, int k, long &mx) -> bool {                    // (asked for k < K only)
            const int tap = k / C;
            const int kh = tap / 3, kw = tap - 3 * kh;
            const unsigned mu = (unsigned)m;                      // m < M < 2^31
            const unsigned row = mu / (unsigned)W;
            const int ow = (int)(mu - row * (unsigned)W), oh = (int)(row % (unsigned)H);
            const int ih = oh + kh - 1, iw = ow + kw - 1;
            mx = m + (kh - 1) * W + (kw - 1);
            return (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
        });
}

// One workgroup per output channel: grad_reduce.h's finish, every column real.
__global__ void __launch_bounds__(256)
conv3x3_dense_wgrad_finish_kernel(const float *__restrict__ part, const float *__restrict__ part_b, tsod_wgrad_plan sh, int K,
                                  const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ dw,
                                  float *__restrict__ dscale, float *__restrict__ dshift) {
    __shared__ float lds[256];
    tsod_wgrad_finish_row(part, part_b, sh, K, K, [](int k) { return k; }, w, scale, dw, dscale, dshift, lds);
}

// ------------------------------------------------------------------------------------------------ strided pixel rows
// big [N,H,W,big_pitch], small [N,OH,OW,small_pitch] with OH = (H - 1) / s + 1: quad c of small's pixel (n, oh, ow) and of big's
// pixel (n, s oh, s ow).  kAdd false: small = big (the rows a strided 1x1 conv reads); true: big = big + small, big the first
// operand, every touched element added to once (that conv's dx into the block's dx).  One 16-byte access per operand.
template <bool kAdd, class Index>
__global__ void __launch_bounds__(256)
pixel_stride_kernel(float *__restrict__ big, int H, int W, int big_pitch, int stride, float *__restrict__ small, long rows, int OH,
                    int OW, int C4, int small_pitch) {
    const Index total = (Index)(rows * C4), step = (Index)gridDim.x * 256;
    for (Index t = (Index)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const Index mi = t / (Index)C4;
        const int c = 4 * (int)(t - mi * (Index)C4);
        const unsigned mu = (unsigned)mi;                             // rows < 2^31
        const unsigned row = mu / (unsigned)OW, n = row / (unsigned)OH;
        const int ow = (int)(mu - row * (unsigned)OW), oh = (int)(row - n * (unsigned)OH);
        float4 *b = reinterpret_cast<float4 *>(big + (((long)n * H + (long)stride * oh) * W + (long)stride * ow) * big_pitch + c);
        float4 *s = reinterpret_cast<float4 *>(small + (long)mi * small_pitch + c);
        if (kAdd) {
            const float4 u = *b, v = *s;
            *b = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
        } else {
            *s = *b;
        }
    }
}

template <bool kAdd>
int pixel_stride_launch(float *big, int N, int H, int W, int C, int big_pitch, int stride, float *small, int small_pitch,
                        tsod_stream_t stream) {
    TSOD_REQUIRE(big && small, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && stride > 0 && big_pitch >= C && small_pitch >= C, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((C & 3) == 0 && (big_pitch & 3) == 0 && (small_pitch & 3) == 0 && tsod_aligned16(big) && tsod_aligned16(small),
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE((long)N * H * W <= 0x7fffffffL, TSOD_ERR_UNSUPPORTED);
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const long rows = (long)N * OH * OW;
    const unsigned blocks = prelu_blocks(rows, C);
    const bool narrow = rows * (C / 4) < 0x7fffffffL;
    auto kernel = narrow ? &pixel_stride_kernel<kAdd, unsigned> : &pixel_stride_kernel<kAdd, long>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, tsod_stream(stream), big, H, W, big_pitch, stride, small, rows, OH, OW,
                       C / 4, small_pitch);
    return tsod_launch_status();
}

inline bool dense_shape_ok(int N, int H, int W, int C, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Cout <= 0 || (C & 3) || (Cout & 3)) return false;
    return (long)N * H * W <= 0x7fffffffL && C <= 0x7fffffff / 9;
}

}  // namespace

extern "C" size_t tsod_prelu_grad_workspace_bytes(int64_t rows, int32_t C) {
    if (rows <= 0 || C <= 0 || (C & 3)) return 0;
    return (size_t)prelu_blocks((long)rows, C) * sizeof(float);
}

extern "C" int tsod_prelu_grad_f32(const float *y, int64_t rows, int32_t C, int32_t y_pitch, const float *dy, int32_t dy_pitch,
                                   int32_t dy_off, float slope, float *g, int32_t g_pitch, float *dslope_num, void *workspace,
                                   size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(y && dy && g, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(rows > 0 && C > 0 && dy_off >= 0 && y_pitch >= C && dy_pitch >= dy_off + C && g_pitch >= C, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((C & 3) == 0 && (y_pitch & 3) == 0 && (dy_pitch & 3) == 0 && (dy_off & 3) == 0 && (g_pitch & 3) == 0,
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(y) && tsod_aligned16(dy) && tsod_aligned16(g), TSOD_ERR_ALIGNMENT);
    const unsigned blocks = prelu_blocks((long)rows, C);
    hipStream_t st = tsod_stream(stream);
    // (t + the grid's stride must not wrap: total + 1024 * 256 < 2^32)
    const bool narrow = (long)rows * (C / 4) < 0x7fffffffL;
    if (!dslope_num) {                                                  // no reduction, no workspace
        auto mask = narrow ? &prelu_grad_kernel<false, unsigned> : &prelu_grad_kernel<false, long>;
        hipLaunchKernelGGL(mask, dim3(blocks), dim3(256), 0, st, y, (long)rows, C / 4, y_pitch, dy, dy_pitch, dy_off, slope, g, g_pitch,
                           (float *)nullptr);
        return tsod_launch_status();
    }
    TSOD_REQUIRE(workspace && workspace_bytes >= tsod_prelu_grad_workspace_bytes(rows, C), TSOD_ERR_WORKSPACE);
    float *partial = static_cast<float *>(workspace);
    auto mask_sum = narrow ? &prelu_grad_kernel<true, unsigned> : &prelu_grad_kernel<true, long>;
    hipLaunchKernelGGL(mask_sum, dim3(blocks), dim3(256), 0, st, y, (long)rows, C / 4, y_pitch, dy, dy_pitch, dy_off, slope, g, g_pitch,
                       partial);
    hipLaunchKernelGGL(prelu_grad_finish_kernel, dim3(1), dim3(256), 0, st, (const float *)partial, (int)blocks, dslope_num);
    return tsod_launch_status();
}

extern "C" size_t tsod_conv3x3_dense_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout) {
    if (!dense_shape_ok(N, H, W, C, Cout)) return 0;
    return tsod_wgrad_plan_bytes(tsod_wgrad_plan_of((long)N * H * W, Cout, 9 * C, true));
}

extern "C" int tsod_conv3x3_dense_wgrad_f32(const float *g, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t g_pitch,
                                            const float *x, int32_t C, int32_t x_pitch, const float *w, const float *scale,
                                            int32_t stride, float *dw, float *dscale, float *dshift, void *workspace,
                                            size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(g && x && w && scale && (dw || dscale || dshift), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && Cout > 0 && g_pitch >= Cout && x_pitch >= C, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(stride == 1, TSOD_ERR_UNSUPPORTED);                    // (the stride-2 3x3 of a projection block: not built)
    TSOD_REQUIRE((C & 3) == 0 && (Cout & 3) == 0 && (x_pitch & 3) == 0 && (g_pitch & 3) == 0 && tsod_aligned16(x) && tsod_aligned16(g),
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(dense_shape_ok(N, H, W, C, Cout), TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) &&
                     workspace_bytes >= tsod_conv3x3_dense_wgrad_workspace_bytes(N, H, W, C, Cout),
                 TSOD_ERR_WORKSPACE);
    const long M = (long)N * H * W;
    const int K = 9 * C;
    const tsod_wgrad_plan sh = tsod_wgrad_plan_of(M, Cout, K, true);
    TSOD_REQUIRE(sh.splits <= 65535, TSOD_ERR_UNSUPPORTED);
    float *part = static_cast<float *>(workspace);
    float *part_b = tsod_wgrad_plan_bias(sh, part);
    hipStream_t st = tsod_stream(stream);
    hipLaunchKernelGGL(conv3x3_dense_wgrad_partial_kernel, dim3(sh.n_tiles * sh.k_tiles, sh.splits), dim3(kWgThreads), 0, st, g,
                       (int)M, Cout, g_pitch, x, C, x_pitch, H, W, sh, part, part_b);
    hipLaunchKernelGGL(conv3x3_dense_wgrad_finish_kernel, dim3(Cout), dim3(256), 0, st, (const float *)part, (const float *)part_b,
                       sh, K, w, scale, dw, dscale, dshift);
    return tsod_launch_status();
}

extern "C" size_t tsod_prelu_grad_d2s_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || (long)N * H * W > 0x7fffffffL) return 0;
    return (size_t)prelu_blocks((long)N * H * W, C) * sizeof(float);
}

extern "C" int tsod_prelu_grad_d2s_f32(const float *y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t y_pitch, const float *p,
                                       int32_t p_pitch, float slope, float *g, int32_t g_pitch, float *dslope_num, void *workspace,
                                       size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(y && p && g, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && y_pitch >= C && g_pitch >= C && C <= 0x7fffffff / 4 && p_pitch >= 4 * C,
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((C & 3) == 0 && (y_pitch & 3) == 0 && (p_pitch & 3) == 0 && (g_pitch & 3) == 0, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(y) && tsod_aligned16(p) && tsod_aligned16(g), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE((long)N * H * W <= 0x7fffffffL, TSOD_ERR_UNSUPPORTED);
    const long rows = (long)N * H * W;
    const unsigned blocks = prelu_blocks(rows, C);
    hipStream_t st = tsod_stream(stream);
    const bool narrow = rows * (C / 4) < 0x7fffffffL;
    if (!dslope_num) {                                                  // no reduction, no workspace
        auto mask = narrow ? &prelu_grad_d2s_kernel<false, unsigned> : &prelu_grad_d2s_kernel<false, long>;
        hipLaunchKernelGGL(mask, dim3(blocks), dim3(256), 0, st, y, rows, C / 4, y_pitch, H, W, p, p_pitch, slope, g, g_pitch,
                           (float *)nullptr);
        return tsod_launch_status();
    }
    TSOD_REQUIRE(workspace && workspace_bytes >= tsod_prelu_grad_d2s_workspace_bytes(N, H, W, C), TSOD_ERR_WORKSPACE);
    float *partial = static_cast<float *>(workspace);
    auto mask_sum = narrow ? &prelu_grad_d2s_kernel<true, unsigned> : &prelu_grad_d2s_kernel<true, long>;
    hipLaunchKernelGGL(mask_sum, dim3(blocks), dim3(256), 0, st, y, rows, C / 4, y_pitch, H, W, p, p_pitch, slope, g, g_pitch, partial);
    hipLaunchKernelGGL(prelu_grad_finish_kernel, dim3(1), dim3(256), 0, st, (const float *)partial, (int)blocks, dslope_num);
    return tsod_launch_status();
}

extern "C" int tsod_pixel_subsample_f32(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t x_pitch, int32_t stride,
                                        float *xs, int32_t xs_pitch, tsod_stream_t stream) {
    return pixel_stride_launch<false>(const_cast<float *>(x), N, H, W, C, x_pitch, stride, xs, xs_pitch, stream);
}

extern "C" int tsod_pixel_upsample_add_f32(float *dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dx_pitch, int32_t stride,
                                           const float *d, int32_t d_pitch, tsod_stream_t stream) {
    return pixel_stride_launch<true>(dx, N, H, W, C, dx_pitch, stride, const_cast<float *>(d), d_pitch, stream);
}
