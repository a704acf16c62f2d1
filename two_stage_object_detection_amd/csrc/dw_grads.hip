// dw_grads.hip -- the backward of the HarDNet tail's two layer kinds:
//
//   tsod_dwconv3x3_grad_f32       y = relu?(scale * dwconv3x3(x, w) + shift)   (pool_layout.hip: dwconv3x3_kernel)
//   tsod_dwconv3x3_grad_act_f32   the same, dx masked by the ReLU6 window of x (x = a 1x1 ConvLayer's output: section 4.18)
//   tsod_gconv1x1_pair_grad_f32   out[g] = w[g][0] in[2g] + w[g][1] in[2g+1] + bias[g]   (gconv1x1_pair_kernel)
//
// NHWC f32, one float4 of channels (one group of the pair conv) per lane.  No float atomics: the parameter gradients are
// sums over pixels, computed as [pixel slice][quantity][channel] partials (a slice = one workgroup's share of the pixels,
// summed inside the workgroup by a fixed tree) which a second launch adds in slice order; the input gradient is a gather
// with a fixed tap order.  Slice count and tree depend on the shape only, so results are bit-identical from run to run.
#include "grad_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;          // workgroups of a reduction launch (slices x channel blocks), about 4 per CU
constexpr int kPixelsPerThread = 4;       // a slice is not split further once its threads have this few pixels each
constexpr int kDwQuantities = 11;         // 9 taps of dw, dscale, dshift

// A workgroup is QL channel lanes x PL = 256 / QL pixel lanes (thread = p * QL + q): QL = the power of two covering
// min(lanes, 64), so that a wave reads 64 consecutive float4s of one pixel when the tensor is that wide and several
// pixels when it is narrower.  S slices of `chunk` consecutive pixels each, QB channel blocks.
struct red_geom {
    int QL, PL, QB, S;
    long chunk;
};
inline red_geom reduction_geometry(long pixels, int lanes) {
    red_geom g;
    g.QL = 1;
    while (g.QL < lanes && g.QL < 64) g.QL <<= 1;
    g.PL = kThreads / g.QL;
    g.QB = (lanes + g.QL - 1) / g.QL;
    const long per_block = (long)g.PL * kPixelsPerThread;
    long S = (pixels + per_block - 1) / per_block;
    const long cap = kMaxBlocks / g.QB > 1 ? kMaxBlocks / g.QB : 1;
    if (S > cap) S = cap;
    if (S < 1) S = 1;
    g.chunk = (pixels + S - 1) / S;
    g.S = (int)((pixels + g.chunk - 1) / g.chunk);
    return g;
}

// Sum of `v` over the PL pixel lanes of each channel lane: a binary tree over p (p += PL/2, PL/4, ... 1), the same for
// every launch of a shape.  Every thread of the workgroup calls it; threads p == 0 (tid < QL) get the sum.
__device__ __forceinline__ float4 block_tree_sum(float4 v, float4 *lds, int tid, int QL) {
    __syncthreads();                                             // (the previous call's result has been read)
    lds[tid] = v;
    __syncthreads();
    for (int s = kThreads / 2; s >= QL; s >>= 1) {
        if (tid < s) {
            float4 a = lds[tid];
            const float4 b = lds[tid + s];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            lds[tid] = a;
        }
        __syncthreads();
    }
    return lds[tid];
}

__device__ __forceinline__ void fma4(float4 &acc, const float4 a, const float4 b) {
    acc.x += a.x * b.x; acc.y += a.y * b.y; acc.z += a.z * b.z; acc.w += a.w * b.w;
}

// Pass 1 of the depthwise backward: one thread walks the output pixels p, p + PL, ... of its slice for one channel quad.
// It recomputes the forward's accumulator (taps in ascending (dh, dw) order, padding taps as zeros: the forward's value,
// so the ReLU mask is the forward's), masks dy into g, optionally stores g for the dx gather, and accumulates
// g * x_tap (9), g * conv and g.
template <int STRIDE>
__global__ void __launch_bounds__(kThreads)
dwconv3x3_grad_reduce_kernel(const float *__restrict__ x, int N, int H, int W, int C4, int in_pitch, int in_off,
                             const float *__restrict__ w, const float *__restrict__ scale, const float *__restrict__ shift,
                             int relu, const float *__restrict__ dy, int dy_pitch, int dy_off, int OH, int OW,
                             float *__restrict__ g_out, float *__restrict__ partials, int QL, long chunk) {
    __shared__ float4 lds[kThreads];
    const int tid = threadIdx.x;
    const int q = tid % QL, p = tid / QL, PL = kThreads / QL;
    const int c4 = blockIdx.y * QL + q;
    const bool active = c4 < C4;
    const int C = C4 * 4;
    const long pixels = (long)N * OH * OW;
    const long lo = (long)blockIdx.x * chunk;
    const long hi = lo + chunk < pixels ? lo + chunk : pixels;

    float4 acc[kDwQuantities];
#pragma unroll
    for (int i = 0; i < kDwQuantities; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        float4 k[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i] = *reinterpret_cast<const float4 *>(w + i * C + 4 * c4);
        float4 s = make_float4(1.f, 1.f, 1.f, 1.f), b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (scale) s = *reinterpret_cast<const float4 *>(scale + 4 * c4);
        if (shift) b = *reinterpret_cast<const float4 *>(shift + 4 * c4);
        const float *xb = x + in_off + 4 * c4;
        for (long px = lo + p; px < hi; px += PL) {
            const int ow = (int)(px % OW);
            const long u = px / OW;
            const int oh = (int)(u % OH);
            const int n = (int)(u / OH);
            float4 xv[9];
            float4 conv = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int dh = 0; dh < 3; ++dh) {
                const int ih = oh * STRIDE - 1 + dh;
#pragma unroll
                for (int dw = 0; dw < 3; ++dw) {
                    const int iw = ow * STRIDE - 1 + dw;
                    const bool ok = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
                    xv[dh * 3 + dw] = ok ? *reinterpret_cast<const float4 *>(xb + (((long)n * H + ih) * W + iw) * in_pitch)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
                    fma4(conv, xv[dh * 3 + dw], k[dh * 3 + dw]);
                }
            }
            float4 g = *reinterpret_cast<const float4 *>(dy + px * dy_pitch + dy_off + 4 * c4);
            if (relu) {
                g.x = conv.x * s.x + b.x > 0.f ? g.x : 0.f;
                g.y = conv.y * s.y + b.y > 0.f ? g.y : 0.f;
                g.z = conv.z * s.z + b.z > 0.f ? g.z : 0.f;
                g.w = conv.w * s.w + b.w > 0.f ? g.w : 0.f;
            }
            if (g_out) *reinterpret_cast<float4 *>(g_out + px * C + 4 * c4) = g;
#pragma unroll
            for (int i = 0; i < 9; ++i) fma4(acc[i], g, xv[i]);
            fma4(acc[9], g, conv);
            acc[10].x += g.x; acc[10].y += g.y; acc[10].z += g.z; acc[10].w += g.w;
        }
    }
#pragma unroll
    for (int i = 0; i < kDwQuantities; ++i) {
        const float4 r = block_tree_sum(acc[i], lds, tid, QL);
        if (p == 0 && active)
            *reinterpret_cast<float4 *>(partials + ((long)blockIdx.x * kDwQuantities + i) * C + 4 * c4) = r;
    }
}

// Pass 2: one thread per (quantity, channel) adds the S partials in slice order; dw takes the forward's scale.
__global__ void __launch_bounds__(kThreads)
dwconv3x3_grad_combine_kernel(const float *__restrict__ partials, int S, int C, const float *__restrict__ scale,
                              float *__restrict__ dw, float *__restrict__ dscale, float *__restrict__ dshift) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= kDwQuantities * C) return;
    const int i = t / C, c = t % C;
    const float sum = tsod_sum_in_slice_order(partials + (long)i * C + c, (long)kDwQuantities * C, S);
    if (i < 9) dw[i * C + c] = scale ? sum * scale[c] : sum;
    else if (i == 9) { if (dscale) dscale[c] = sum; }
    else dshift[c] = sum;
}

// dx: the thread that owns an input pixel's channel quad adds w[dh][dw] * g[oh][ow] over the outputs that read it
// (ih = oh * STRIDE - 1 + dh), dh then dw ascending, then takes the scale.  `xact` (tsod_dwconv3x3_grad_act_f32): x is the
// ReLU6 output of the layer before, and the thread keeps its sum only where 0 < x < 6 (that layer's masked gradient).
template <int STRIDE>
__global__ void __launch_bounds__(kThreads)
dwconv3x3_grad_input_kernel(const float *__restrict__ g, int g_pitch, int g_off, int N, int H, int W, int C4, int OH, int OW,
                            const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ dx,
                            int dx_pitch, int dx_off, int accumulate, const float *__restrict__ xact, int x_pitch, int x_off) {
    const long total = (long)N * H * W * C4;
    const int C = C4 * 4;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(t % C4);
        long u = t / C4;
        const int iw = (int)(u % W);
        u /= W;
        const int ih = (int)(u % H);
        const int n = (int)(u / H);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
            const int th = ih + 1 - dh;
            if (th < 0 || th % STRIDE != 0 || th / STRIDE >= OH) continue;
            const int oh = th / STRIDE;
#pragma unroll
            for (int dw = 0; dw < 3; ++dw) {
                const int tw = iw + 1 - dw;
                if (tw < 0 || tw % STRIDE != 0 || tw / STRIDE >= OW) continue;
                const int ow = tw / STRIDE;
                const float4 gv = *reinterpret_cast<const float4 *>(g + (((long)n * OH + oh) * OW + ow) * g_pitch + g_off + 4 * c4);
                const float4 kk = *reinterpret_cast<const float4 *>(w + (dh * 3 + dw) * C + 4 * c4);
                fma4(acc, gv, kk);
            }
        }
        if (scale) {
            const float4 s = *reinterpret_cast<const float4 *>(scale + 4 * c4);
            acc.x *= s.x; acc.y *= s.y; acc.z *= s.z; acc.w *= s.w;
        }
        if (xact) {
            const float4 v = *reinterpret_cast<const float4 *>(xact + (((long)n * H + ih) * W + iw) * x_pitch + x_off + 4 * c4);
            acc = tsod_relu6_keep(acc, v);
        }
        float4 *dst = reinterpret_cast<float4 *>(dx + (((long)n * H + ih) * W + iw) * dx_pitch + dx_off + 4 * c4);
        if (accumulate) {
            const float4 old = *dst;
            acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w;
        }
        *dst = acc;
    }
}

// The pair conv's backward in one pass over the pixels: d_in is elementwise, (dw[g][0], dw[g][1], dbias[g]) ride in one
// float4 through the same slice reduction.
__global__ void __launch_bounds__(kThreads)
gconv1x1_pair_grad_kernel(const float *__restrict__ in, long pixels, int G, int in_pitch, const float *__restrict__ w,
                          const float *__restrict__ d_out, int d_out_pitch, float *__restrict__ d_in, int d_in_pitch,
                          float *__restrict__ partials, int QL, long chunk) {
    __shared__ float4 lds[kThreads];
    const int tid = threadIdx.x;
    const int q = tid % QL, p = tid / QL, PL = kThreads / QL;
    const int g = blockIdx.y * QL + q;
    const bool active = g < G;
    const long lo = (long)blockIdx.x * chunk;
    const long hi = lo + chunk < pixels ? lo + chunk : pixels;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        const float2 k = *reinterpret_cast<const float2 *>(w + 2 * g);
        for (long px = lo + p; px < hi; px += PL) {
            const float2 v = *reinterpret_cast<const float2 *>(in + px * in_pitch + 2 * g);
            const float d = d_out[px * d_out_pitch + g];
            if (d_in) *reinterpret_cast<float2 *>(d_in + px * d_in_pitch + 2 * g) = make_float2(k.x * d, k.y * d);
            acc.x += d * v.x;
            acc.y += d * v.y;
            acc.z += d;
        }
    }
    const float4 r = block_tree_sum(acc, lds, tid, QL);
    if (p == 0 && active) {
        float *dst = partials + (long)blockIdx.x * 3 * G;
        dst[g] = r.x;
        dst[G + g] = r.y;
        dst[2 * G + g] = r.z;
    }
}

__global__ void __launch_bounds__(kThreads)
gconv1x1_pair_grad_combine_kernel(const float *__restrict__ partials, int S, int G, float *__restrict__ dw,
                                  float *__restrict__ dbias) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * G) return;
    const int i = t / G, g = t % G;
    const float sum = tsod_sum_in_slice_order(partials + (long)i * G + g, 3L * G, S);
    if (i < 2) { if (dw) dw[2 * g + i] = sum; }
    else if (dbias) dbias[g] = sum;
}

inline bool dw_grad_shape_ok(int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride) {
    return N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && (stride == 1 || stride == 2);
}

}  // namespace

extern "C" size_t tsod_dwconv3x3_grad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t stride, int32_t relu_dx) {
    if (!dw_grad_shape_ok(N, H, W, C, stride)) return 0;
    const long pixels = (long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    const red_geom g = reduction_geometry(pixels, C / 4);
    const size_t partials = tsod_align_up((size_t)g.S * kDwQuantities * C * sizeof(float), 256);
    return partials + (relu_dx ? (size_t)pixels * C * sizeof(float) : 0);    // [partials | g = masked dy, for the dx gather]
}

// both entry points; `act_dx`: the dx gather masks with the ReLU6 window of the x pixel it owns
static int dwconv3x3_grad(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch, int32_t in_off,
                          const float *w, const float *scale, const float *shift, int32_t stride, int32_t relu, const float *dy,
                          int32_t dy_pitch, int32_t dy_off, float *dx, int32_t dx_pitch, int32_t dx_off, int32_t accumulate,
                          float *dw, float *dscale, float *dshift, void *workspace, size_t workspace_bytes,
                          tsod_stream_t stream, bool act_dx) {
    TSOD_REQUIRE(x && w && dy, TSOD_ERR_INVALID_ARG);
    // the parameter gradients come together (dscale optional), or not at all: then only dx is computed
    const bool params = dw != nullptr;
    TSOD_REQUIRE((dw != nullptr) == (dshift != nullptr) && (params || dscale == nullptr) && (params || dx != nullptr),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && (stride == 1 || stride == 2), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(scale != nullptr || dscale == nullptr, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((C & 3) == 0 && (in_pitch & 3) == 0 && (dy_pitch & 3) == 0 && (in_off & 3) == 0 && (dy_off & 3) == 0,
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(in_off >= 0 && dy_off >= 0 && in_pitch >= in_off + C && dy_pitch >= dy_off + C, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(tsod_aligned16(x) && tsod_aligned16(dy) && tsod_aligned16(w) && tsod_aligned16(dw) && tsod_aligned16(dshift) &&
                     tsod_aligned16(dscale),
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE((!scale || tsod_aligned16(scale)) && (!shift || tsod_aligned16(shift)), TSOD_ERR_ALIGNMENT);
    if (dx) {
        TSOD_REQUIRE((dx_pitch & 3) == 0 && (dx_off & 3) == 0 && tsod_aligned16(dx), TSOD_ERR_ALIGNMENT);
        TSOD_REQUIRE(dx_off >= 0 && dx_pitch >= dx_off + C, TSOD_ERR_INVALID_ARG);
    }
    const bool reduce = params || relu;                          // (dx alone behind a ReLU: the pass still makes g)
    TSOD_REQUIRE(!reduce || (workspace && tsod_aligned16(workspace) &&
                             workspace_bytes >= tsod_dwconv3x3_grad_workspace_bytes(N, H, W, C, stride, relu && dx)),
                 TSOD_ERR_WORKSPACE);
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const long pixels = (long)N * OH * OW;
    const red_geom geo = reduction_geometry(pixels, C / 4);
    TSOD_REQUIRE(geo.QB <= 65535, TSOD_ERR_UNSUPPORTED);
    float *partials = static_cast<float *>(workspace);
    float *g_ws = (relu && dx) ? reinterpret_cast<float *>(static_cast<char *>(workspace) +
                                                           tsod_align_up((size_t)geo.S * kDwQuantities * C * sizeof(float), 256))
                               : nullptr;
    hipStream_t st = tsod_stream(stream);
    const dim3 rgrid((unsigned)geo.S, (unsigned)geo.QB);
    if (reduce && stride == 1)
        hipLaunchKernelGGL(dwconv3x3_grad_reduce_kernel<1>, rgrid, dim3(kThreads), 0, st, x, N, H, W, C / 4, in_pitch, in_off, w,
                           scale, shift, relu, dy, dy_pitch, dy_off, OH, OW, g_ws, partials, geo.QL, geo.chunk);
    else if (reduce)
        hipLaunchKernelGGL(dwconv3x3_grad_reduce_kernel<2>, rgrid, dim3(kThreads), 0, st, x, N, H, W, C / 4, in_pitch, in_off, w,
                           scale, shift, relu, dy, dy_pitch, dy_off, OH, OW, g_ws, partials, geo.QL, geo.chunk);
    if (params)
        hipLaunchKernelGGL(dwconv3x3_grad_combine_kernel, dim3((unsigned)((kDwQuantities * C + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, partials, geo.S, C, scale, dw, dscale, dshift);
    if (dx) {
        const float *xact = act_dx ? x : nullptr;
        const float *g = g_ws ? g_ws : dy;
        const int g_pitch = g_ws ? C : dy_pitch, g_off = g_ws ? 0 : dy_off;
        const long total = (long)N * H * W * (C / 4);
        const unsigned blocks = (unsigned)((total + kThreads - 1) / kThreads < 16384 ? (total + kThreads - 1) / kThreads : 16384);
        if (stride == 1)
            hipLaunchKernelGGL(dwconv3x3_grad_input_kernel<1>, dim3(blocks), dim3(kThreads), 0, st, g, g_pitch, g_off, N, H, W,
                               C / 4, OH, OW, w, scale, dx, dx_pitch, dx_off, accumulate, xact, in_pitch, in_off);
        else
            hipLaunchKernelGGL(dwconv3x3_grad_input_kernel<2>, dim3(blocks), dim3(kThreads), 0, st, g, g_pitch, g_off, N, H, W,
                               C / 4, OH, OW, w, scale, dx, dx_pitch, dx_off, accumulate, xact, in_pitch, in_off);
    }
    return tsod_launch_status();
}

extern "C" int tsod_dwconv3x3_grad_f32(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch,
                                       int32_t in_off, const float *w, const float *scale, const float *shift,
                                       int32_t stride, int32_t relu, const float *dy, int32_t dy_pitch, int32_t dy_off,
                                       float *dx, int32_t dx_pitch, int32_t dx_off, int32_t accumulate, float *dw,
                                       float *dscale, float *dshift, void *workspace, size_t workspace_bytes,
                                       tsod_stream_t stream) {
    return dwconv3x3_grad(x, N, H, W, C, in_pitch, in_off, w, scale, shift, stride, relu, dy, dy_pitch, dy_off, dx, dx_pitch,
                          dx_off, accumulate, dw, dscale, dshift, workspace, workspace_bytes, stream, false);
}

extern "C" int tsod_dwconv3x3_grad_act_f32(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_pitch,
                                           int32_t in_off, const float *w, const float *scale, const float *shift,
                                           int32_t stride, int32_t relu, const float *dy, int32_t dy_pitch, int32_t dy_off,
                                           float *dx, int32_t dx_pitch, int32_t dx_off, int32_t accumulate, float *dw,
                                           float *dscale, float *dshift, void *workspace, size_t workspace_bytes,
                                           tsod_stream_t stream) {
    return dwconv3x3_grad(x, N, H, W, C, in_pitch, in_off, w, scale, shift, stride, relu, dy, dy_pitch, dy_off, dx, dx_pitch,
                          dx_off, accumulate, dw, dscale, dshift, workspace, workspace_bytes, stream, true);
}

extern "C" size_t tsod_gconv1x1_pair_grad_workspace_bytes(int64_t pixels, int32_t G) {
    if (pixels <= 0 || G <= 0) return 0;
    const red_geom g = reduction_geometry((long)pixels, G);
    return tsod_align_up((size_t)g.S * 3 * G * sizeof(float), 256);
}

extern "C" int tsod_gconv1x1_pair_grad_f32(const float *in, int64_t pixels, int32_t G, int32_t in_pitch, const float *w,
                                           const float *d_out, int32_t d_out_pitch, float *d_in, int32_t d_in_pitch,
                                           float *dw, float *dbias, void *workspace, size_t workspace_bytes,
                                           tsod_stream_t stream) {
    TSOD_REQUIRE(in && w && d_out, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(pixels > 0 && G > 0 && in_pitch >= 2 * G && d_out_pitch >= G, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((in_pitch & 1) == 0 && (reinterpret_cast<uintptr_t>(in) & 7u) == 0 && (reinterpret_cast<uintptr_t>(w) & 7u) == 0,
                 TSOD_ERR_ALIGNMENT);
    if (d_in) {
        TSOD_REQUIRE(d_in_pitch >= 2 * G, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE((d_in_pitch & 1) == 0 && (reinterpret_cast<uintptr_t>(d_in) & 7u) == 0, TSOD_ERR_ALIGNMENT);
    }
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= tsod_gconv1x1_pair_grad_workspace_bytes(pixels, G),
                 TSOD_ERR_WORKSPACE);
    const red_geom geo = reduction_geometry((long)pixels, G);
    TSOD_REQUIRE(geo.QB <= 65535, TSOD_ERR_UNSUPPORTED);
    float *partials = static_cast<float *>(workspace);
    hipStream_t st = tsod_stream(stream);
    hipLaunchKernelGGL(gconv1x1_pair_grad_kernel, dim3((unsigned)geo.S, (unsigned)geo.QB), dim3(kThreads), 0, st, in, (long)pixels, G,
                       in_pitch, w, d_out, d_out_pitch, d_in, d_in_pitch, partials, geo.QL, geo.chunk);
    if (dw || dbias)
        hipLaunchKernelGGL(gconv1x1_pair_grad_combine_kernel, dim3((unsigned)((3 * G + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           st, partials, geo.S, G, dw, dbias);
    return tsod_launch_status();
}
