// optim.hip -- the reference's optimizer step (train/train.py: torch.optim.AdamW(...).step()) as ONE launch
// over any number of tensors.
//
//   adamw_update                 the update of one element, written once for host and device: torch's single-tensor AdamW
//                                (decoupled weight decay, amsgrad=False, maximize=False) operation by operation
//   adamw_multi_tensor_kernel    workgroup c takes chunks[c] = (tensor, piece): TSOD_ADAMW_CHUNK elements of one tensor of
//                                the table, so a 16-element bias costs one workgroup and a 747 520-element weight is spread
//                                over 365; the step's scalars ride in the kernel arguments
// Compiled with -ffp-contract=off: no operation pair below becomes an fma, on the host or on the device; divide and sqrtf
// are the correctly rounded ones.
#include "tsod_internal.h"
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = TSOD_ADAMW_CHUNK;
static_assert(kChunk % (4 * kThreads) == 0, "whole float4 rounds per chunk");

typedef __attribute__((address_space(1))) float gfloat;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 gfloat4;

struct adamw_groups {
    tsod_adamw_group g[TSOD_ADAMW_MAX_GROUPS];
};

__host__ __device__ inline void adamw_update(float &p, float g, float &m, float &v, const tsod_adamw_group &h) {
    p = p * h.decay;
    const float w = h.one_minus_beta1, d = g - m;
    m = w < 0.5f ? m + d * w : g - d * (1.f - w);          // at::lerp_ (|weight| < 0.5 picks the form; weight >= 0 here)
    v = v * h.beta2;
    v = v + (h.one_minus_beta2 * g) * g;                   // addcmul_: the scalar goes into g first
    const float denom = sqrtf(v) / h.bias2_sqrt + h.eps;
    p = p + ((-h.step_size) * m) / denom;                  // addcdiv_: scalar times m, then the division
}

__global__ void __launch_bounds__(kThreads)
adamw_multi_tensor_kernel(const tsod_adamw_tensor *__restrict__ table, int n_tensors,
                          const tsod_adamw_chunk *__restrict__ chunks, adamw_groups groups, int n_groups, int zero_grad) {
    const tsod_adamw_chunk c = chunks[blockIdx.x];
    if (c.tensor < 0 || c.tensor >= n_tensors || c.piece < 0) return;
    const tsod_adamw_tensor t = table[c.tensor];
    const int gi = __builtin_amdgcn_readfirstlane(t.group);
    if (gi < 0 || gi >= n_groups) return;
    const tsod_adamw_group h = groups.g[gi];
    const int64_t first = (int64_t)c.piece * kChunk;
    if (first >= t.n) return;
    const int64_t left = t.n - first;
    const int n = left < kChunk ? (int)left : kChunk;
    // pointers read from the table carry no address space: say "global", or every access below is a flat_ one
    gfloat *__restrict__ P = (gfloat *)t.param + first;
    gfloat *__restrict__ G = (gfloat *)t.grad + first;
    gfloat *__restrict__ M = (gfloat *)t.exp_avg + first;
    gfloat *__restrict__ V = (gfloat *)t.exp_avg_sq + first;
    int done = 0;
    if ((((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V) & 15u) == 0) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += kThreads) {
            const f32x4 p4 = ((gfloat4 *)P)[i], m4 = ((gfloat4 *)M)[i], v4 = ((gfloat4 *)V)[i], g4 = ((gfloat4 *)G)[i];
            float p[4] = {p4.x, p4.y, p4.z, p4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
            const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) adamw_update(p[k], g[k], m[k], v[k], h);
            ((gfloat4 *)P)[i] = f32x4{p[0], p[1], p[2], p[3]};
            ((gfloat4 *)M)[i] = f32x4{m[0], m[1], m[2], m[3]};
            ((gfloat4 *)V)[i] = f32x4{v[0], v[1], v[2], v[3]};
            if (zero_grad) ((gfloat4 *)G)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += kThreads) {          // unaligned chunks and the last 1..3 elements
        float p = P[i], m = M[i], v = V[i];
        adamw_update(p, G[i], m, v, h);
        P[i] = p;
        M[i] = m;
        V[i] = v;
        if (zero_grad) G[i] = 0.f;
    }
}

}  // namespace

extern "C" int tsod_adamw_step_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks,
                                   int64_t n_chunks, const tsod_adamw_group *groups, int32_t n_groups, int32_t zero_grad,
                                   tsod_stream_t stream) {
    TSOD_REQUIRE(table && chunks && groups, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && n_chunks <= INT32_MAX && n_groups >= 1, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_groups <= TSOD_ADAMW_MAX_GROUPS, TSOD_ERR_UNSUPPORTED);
    if (n_tensors == 0 || n_chunks == 0) return TSOD_OK;
    adamw_groups by_value = {};
    for (int i = 0; i < n_groups; ++i) by_value.g[i] = groups[i];
    adamw_multi_tensor_kernel<<<dim3((unsigned)n_chunks), dim3(kThreads), 0, tsod_stream(stream)>>>(
        table, n_tensors, chunks, by_value, n_groups, zero_grad != 0);
    return tsod_launch_status();
}

extern "C" int tsod_adamw_step_host_f32(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                        const tsod_adamw_group *group, int32_t zero_grad) {
    TSOD_REQUIRE(param && grad && exp_avg && exp_avg_sq && group && n >= 0, TSOD_ERR_INVALID_ARG);
    for (int64_t i = 0; i < n; ++i) {
        adamw_update(param[i], grad[i], exp_avg[i], exp_avg_sq[i], *group);
        if (zero_grad) grad[i] = 0.f;
    }
    return TSOD_OK;
}
