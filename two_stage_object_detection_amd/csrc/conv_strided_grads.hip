// conv_strided_grads.hip -- the parameter gradients of a dense 3x3 conv at stride 1 or 2, pad 1: what a projection Bottleneck's
// conv2 needs.
//
//   tsod_conv3x3_strided_wgrad_f32  conv_grads.hip's tsod_conv3x3_dense_wgrad_f32 with dY's rows over the OUTPUT grid: grad_reduce.h's
//                                   tile a fourth time and its finish; at stride 1 the bits of the dense entry point
//
// A file of its own, not a part of conv_grads.hip: a second instantiation of the tile in that translation unit changes the
// compiler's instruction selection for the dense kernel there (three address instructions of its wave tree), and that kernel's
// code is kept as it was measured.  No float atomics; every order of additions is grad_reduce.h's and depends on the shape only.
#include "grad_reduce.h"

namespace {

// dY's rows m = (n, oh, ow) run over the OUTPUT grid [N,OH,OW] of a 3x3 at stride s, pad 1.  Column k = (kh * 3 + kw) * C + c of
// row m is channel c of pixel (n, s oh + kh - 1, s ow + kw - 1): row (n H + ih) W + iw of x where (ih, iw) is inside the image,
// else a zero.  Validity is decided on (ih, iw), never on a shifted row number.  C % 4 == 0: a lane's quad lies in one tap.
// With s = 1 the rows, the plan and every operand are conv_grads.hip's dense kernel's: the same bits.
__global__ void __launch_bounds__(kWgThreads)
conv3x3_strided_wgrad_partial_kernel(const float *__restrict__ g, int M, int Cout, int g_pitch, const float *__restrict__ x, int C,
                                     int x_pitch, int H, int W, int OH, int OW, int stride, tsod_wgrad_plan sh,
                                     float *__restrict__ part, float *__restrict__ part_b) {
    __shared__ float lds[kWgLdsFloats];
    const int K = 9 * C;
    tsod_wgrad_tile(
        g, (long)M, Cout, g_pitch, x, x_pitch, [=](int k) { return k < K ? k % C : -1; }, sh, part, part_b, lds,
        [=](long m, int k, long &mx) -> bool {                    // (asked for k < K only)
            const int tap = k / C;
            const int kh = tap / 3, kw = tap - 3 * kh;
            const unsigned mu = (unsigned)m;                      // m < M < 2^31
            const unsigned row = mu / (unsigned)OW, n = row / (unsigned)OH;
            const int ow = (int)(mu - row * (unsigned)OW), oh = (int)(row - n * (unsigned)OH);
            const int ih = stride * oh + kh - 1, iw = stride * ow + kw - 1;
            mx = ((long)n * H + ih) * W + iw;
            return (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
        });
}

// One workgroup per output channel: grad_reduce.h's finish, every column real.
__global__ void __launch_bounds__(256)
conv3x3_strided_wgrad_finish_kernel(const float *__restrict__ part, const float *__restrict__ part_b, tsod_wgrad_plan sh, int K,
                                    const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ dw,
                                    float *__restrict__ dscale, float *__restrict__ dshift) {
    __shared__ float lds[256];
    tsod_wgrad_finish_row(part, part_b, sh, K, K, [](int k) { return k; }, w, scale, dw, dscale, dshift, lds);
}

inline bool strided_shape_ok(int N, int H, int W, int C, int Cout, int stride) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Cout <= 0 || (C & 3) || (Cout & 3) || (stride != 1 && stride != 2)) return false;
    return (long)N * H * W <= 0x7fffffffL && C <= 0x7fffffff / 9;
}

}  // namespace

extern "C" size_t tsod_conv3x3_strided_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout,
                                                             int32_t stride) {
    if (!strided_shape_ok(N, H, W, C, Cout, stride)) return 0;
    const long M = (long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    return tsod_wgrad_plan_bytes(tsod_wgrad_plan_of(M, Cout, 9 * C, true));
}

extern "C" int tsod_conv3x3_strided_wgrad_f32(const float *g, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t g_pitch,
                                              const float *x, int32_t C, int32_t x_pitch, const float *w, const float *scale,
                                              int32_t stride, float *dw, float *dscale, float *dshift, void *workspace,
                                              size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(g && x && w && scale && (dw || dscale || dshift), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && Cout > 0 && g_pitch >= Cout && x_pitch >= C, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(stride == 1 || stride == 2, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE((C & 3) == 0 && (Cout & 3) == 0 && (x_pitch & 3) == 0 && (g_pitch & 3) == 0 && tsod_aligned16(x) && tsod_aligned16(g),
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(strided_shape_ok(N, H, W, C, Cout, stride), TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) &&
                     workspace_bytes >= tsod_conv3x3_strided_wgrad_workspace_bytes(N, H, W, C, Cout, stride),
                 TSOD_ERR_WORKSPACE);
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const long M = (long)N * OH * OW;
    const int K = 9 * C;
    const tsod_wgrad_plan sh = tsod_wgrad_plan_of(M, Cout, K, true);
    TSOD_REQUIRE(sh.splits <= 65535, TSOD_ERR_UNSUPPORTED);
    float *part = static_cast<float *>(workspace);
    float *part_b = tsod_wgrad_plan_bias(sh, part);
    hipStream_t st = tsod_stream(stream);
    hipLaunchKernelGGL(conv3x3_strided_wgrad_partial_kernel, dim3(sh.n_tiles * sh.k_tiles, sh.splits), dim3(kWgThreads), 0, st, g,
                       (int)M, Cout, g_pitch, x, C, x_pitch, H, W, OH, OW, stride, sh, part, part_b);
    hipLaunchKernelGGL(conv3x3_strided_wgrad_finish_kernel, dim3(Cout), dim3(256), 0, st, (const float *)part, (const float *)part_b,
                       sh, K, w, scale, dw, dscale, dshift);
    return tsod_launch_status();
}
