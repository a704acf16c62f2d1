// optim.hip -- the reference's optimizer step (train/train.py: torch.optim.AdamW(...).step()) as ONE launch
// over any number of tensors.
//
//   adamw_update                 the update of one element, written once for host and device: torch's single-tensor AdamW
//                                (decoupled weight decay, amsgrad=False, maximize=False) operation by operation
//   adamw_multi_tensor_kernel    workgroup c takes chunks[c] = (tensor, piece): TSOD_ADAMW_CHUNK elements of one tensor of
//                                the table, so a 16-element bias costs one workgroup and a 747 520-element weight is spread
//                                over 365; the step's scalars ride in the kernel arguments
//   adamw_clipped_multi_tensor_kernel  the same with g' = g * clip->coef in front of the update (the coefficient is read from
//                                device memory) and g' (or 0 with zero_grad) stored into the gradient
//   grad_norm_partial_kernel     workgroup c: the f64 sum of squares of chunks[c], one partial per chunk
//   grad_norm_finish_kernel      one workgroup: the partials in a fixed order, the norm and the clip coefficient
//   grad_scale_kernel            g = g * clip->coef over the same work list (optim.clip_grad_norm_)
// The norm's orders (include/tsod.h, grad_reduce.h) depend on the element counts only: no atomics, no tickets.
// Compiled with -ffp-contract=off: no operation pair below becomes an fma, on the host or on the device; divide and sqrtf
// are the correctly rounded ones.
#include "grad_reduce.h"
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

typedef __attribute__((address_space(1))) const float cgfloat;
typedef __attribute__((address_space(1))) const f32x4 cgfloat4;

// the body of both step kernels; kClip: g' = g * coef goes into the update and back into the gradient
template <bool kClip>
__device__ __forceinline__ void adamw_chunk_body(const tsod_adamw_tensor *__restrict__ table, int n_tensors,
                                                 const tsod_adamw_chunk *__restrict__ chunks, const adamw_groups &groups,
                                                 int n_groups, int zero_grad, float coef) {
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
            float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (kClip) g[k] = g[k] * coef;
                adamw_update(p[k], g[k], m[k], v[k], h);
            }
            ((gfloat4 *)P)[i] = f32x4{p[0], p[1], p[2], p[3]};
            ((gfloat4 *)M)[i] = f32x4{m[0], m[1], m[2], m[3]};
            ((gfloat4 *)V)[i] = f32x4{v[0], v[1], v[2], v[3]};
            if (zero_grad) ((gfloat4 *)G)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            else if (kClip) ((gfloat4 *)G)[i] = f32x4{g[0], g[1], g[2], g[3]};
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += kThreads) {          // unaligned chunks and the last 1..3 elements
        float p = P[i], m = M[i], v = V[i], g = G[i];
        if (kClip) g = g * coef;
        adamw_update(p, g, m, v, h);
        P[i] = p;
        M[i] = m;
        V[i] = v;
        if (zero_grad) G[i] = 0.f;
        else if (kClip) G[i] = g;
    }
}

__global__ void __launch_bounds__(kThreads)
adamw_multi_tensor_kernel(const tsod_adamw_tensor *__restrict__ table, int n_tensors,
                          const tsod_adamw_chunk *__restrict__ chunks, adamw_groups groups, int n_groups, int zero_grad) {
    adamw_chunk_body<false>(table, n_tensors, chunks, groups, n_groups, zero_grad, 1.f);
}

__global__ void __launch_bounds__(kThreads)
adamw_clipped_multi_tensor_kernel(const tsod_adamw_tensor *__restrict__ table, int n_tensors,
                                  const tsod_adamw_chunk *__restrict__ chunks, adamw_groups groups, int n_groups,
                                  int zero_grad, const tsod_grad_norm_result *__restrict__ clip) {
    adamw_chunk_body<true>(table, n_tensors, chunks, groups, n_groups, zero_grad, clip->coef);
}

// ---------------------------------------------------------------------------------------------------------- the norm
// The chunk's gradient slice, or n = 0 for a record that points outside the table (the step kernel's rule).
struct grad_slice {
    gfloat *g;
    int n;
};
__device__ __forceinline__ grad_slice grad_slice_of(const tsod_adamw_tensor *__restrict__ table, int n_tensors,
                                                    const tsod_adamw_chunk c) {
    grad_slice s = {nullptr, 0};
    if (c.tensor < 0 || c.tensor >= n_tensors || c.piece < 0) return s;
    const int64_t total = table[c.tensor].n;
    const int64_t first = (int64_t)c.piece * kChunk;
    if (first >= total) return s;
    const int64_t left = total - first;
    s.g = (gfloat *)table[c.tensor].grad + first;
    s.n = left < kChunk ? (int)left : kChunk;
    return s;
}

// (double)g * (double)g is exact; the sum is rounded once per add
__host__ __device__ inline void add_square(double &acc, float g) { acc = acc + (double)g * (double)g; }

// sum, norm and coefficient from the sum of squares; empty: no gradient at all
__host__ __device__ inline tsod_grad_norm_result grad_norm_record(double sum_sq, float max_norm, bool empty) {
    tsod_grad_norm_result r;
    if (empty) {
        r.sum_sq = 0.0;
        r.norm = 0.f;
        r.coef = 1.f;
        return r;
    }
    r.sum_sq = sum_sq;
    r.norm = (float)sqrt(sum_sq);
    const float c = max_norm / (r.norm + 1e-6f);
    r.coef = c > 1.f ? 1.f : c;                                        // a NaN stays (the comparison is false), inf / inf too
    return r;
}

// Thread t owns quads t, t + 256, ... of its chunk (quads counted from the chunk's first element, whatever its address), the
// elements of a quad in ascending order, a last short quad included; then tsod_tree_sum_256_f64.
__global__ void __launch_bounds__(kThreads)
grad_norm_partial_kernel(const tsod_adamw_tensor *__restrict__ table, int n_tensors,
                         const tsod_adamw_chunk *__restrict__ chunks, double *__restrict__ partials) {
    __shared__ double lds[kThreads];
    const grad_slice s = grad_slice_of(table, n_tensors, chunks[blockIdx.x]);
    cgfloat *__restrict__ G = (cgfloat *)s.g;
    const int n = s.n, n4 = n >> 2;
    double acc = 0.0;
    if (((uintptr_t)G & 15u) == 0) {
        for (int q = threadIdx.x; q < n4; q += kThreads) {
            const f32x4 g4 = ((cgfloat4 *)G)[q];
            add_square(acc, g4.x);
            add_square(acc, g4.y);
            add_square(acc, g4.z);
            add_square(acc, g4.w);
        }
    } else {
        for (int q = threadIdx.x; q < n4; q += kThreads) {
            const float g0 = G[4 * q], g1 = G[4 * q + 1], g2 = G[4 * q + 2], g3 = G[4 * q + 3];
            add_square(acc, g0);
            add_square(acc, g1);
            add_square(acc, g2);
            add_square(acc, g3);
        }
    }
    if ((n & 3) && (int)threadIdx.x == (n4 & (kThreads - 1)))          // the short quad n4 belongs to thread n4 % 256: its last
        for (int i = n4 << 2; i < n; ++i) add_square(acc, G[i]);
    const double sum = tsod_tree_sum_256_f64(acc, lds, threadIdx.x);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// one workgroup: thread t adds partials t, t + 256, ... ascending, then the same tree; thread 0 writes the record
__global__ void __launch_bounds__(kThreads)
grad_norm_finish_kernel(const double *__restrict__ partials, int n_partials, float max_norm,
                        tsod_grad_norm_result *__restrict__ result) {
    __shared__ double lds[kThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += kThreads) acc = acc + partials[i];
    const double sum = tsod_tree_sum_256_f64(acc, lds, threadIdx.x);
    if (threadIdx.x == 0) *result = grad_norm_record(sum, max_norm, n_partials == 0);
}

__global__ void __launch_bounds__(kThreads)
grad_scale_kernel(const tsod_adamw_tensor *__restrict__ table, int n_tensors, const tsod_adamw_chunk *__restrict__ chunks,
                  const tsod_grad_norm_result *__restrict__ clip) {
    const float coef = clip->coef;
    const grad_slice s = grad_slice_of(table, n_tensors, chunks[blockIdx.x]);
    gfloat *__restrict__ G = s.g;
    const int n = s.n;
    int done = 0;
    if (((uintptr_t)G & 15u) == 0) {
        const int n4 = n >> 2;
        for (int i = threadIdx.x; i < n4; i += kThreads) {
            const f32x4 g = ((gfloat4 *)G)[i];
            ((gfloat4 *)G)[i] = f32x4{g.x * coef, g.y * coef, g.z * coef, g.w * coef};
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += kThreads) G[i] = G[i] * coef;
}

// what the three entry points that walk the work list share
inline int check_work_list(const void *table, int32_t n_tensors, const void *chunks, int64_t n_chunks) {
    TSOD_REQUIRE(table && chunks, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && n_chunks <= INT32_MAX, TSOD_ERR_INVALID_ARG);
    return TSOD_OK;
}

// one host thread of the norm: the quads it owns of one chunk (`g`: the chunk's n elements), in the kernel's order
inline double host_thread_sum(const float *g, int n, int t) {
    const int n4 = n >> 2;
    double acc = 0.0;
    for (int q = t; q < n4; q += kThreads)
        for (int k = 0; k < 4; ++k) add_square(acc, g[4 * q + k]);
    if ((n & 3) && t == (n4 & (kThreads - 1)))
        for (int i = n4 << 2; i < n; ++i) add_square(acc, g[i]);
    return acc;
}

// tsod_tree_sum_256_f64 on the host: v[0] has the sum
inline double host_tree_sum_256(double *v) {
    for (int st = kThreads / 2; st >= 1; st >>= 1)
        for (int t = 0; t < st; ++t) v[t] = v[t] + v[t + st];
    return v[0];
}

}  // namespace

extern "C" int tsod_adamw_step_clipped_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks,
                                           int64_t n_chunks, const tsod_adamw_group *groups, int32_t n_groups,
                                           int32_t zero_grad, const tsod_grad_norm_result *clip, tsod_stream_t stream) {
    TSOD_REQUIRE(table && chunks && groups, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && n_chunks <= INT32_MAX && n_groups >= 1, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_groups <= TSOD_ADAMW_MAX_GROUPS, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(((uintptr_t)clip & 7u) == 0, TSOD_ERR_ALIGNMENT);
    if (n_tensors == 0 || n_chunks == 0) return TSOD_OK;
    adamw_groups by_value = {};
    for (int i = 0; i < n_groups; ++i) by_value.g[i] = groups[i];
    if (clip)
        adamw_clipped_multi_tensor_kernel<<<dim3((unsigned)n_chunks), dim3(kThreads), 0, tsod_stream(stream)>>>(
            table, n_tensors, chunks, by_value, n_groups, zero_grad != 0, clip);
    else
        adamw_multi_tensor_kernel<<<dim3((unsigned)n_chunks), dim3(kThreads), 0, tsod_stream(stream)>>>(
            table, n_tensors, chunks, by_value, n_groups, zero_grad != 0);
    return tsod_launch_status();
}

extern "C" int tsod_adamw_step_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks,
                                   int64_t n_chunks, const tsod_adamw_group *groups, int32_t n_groups, int32_t zero_grad,
                                   tsod_stream_t stream) {
    return tsod_adamw_step_clipped_f32(table, n_tensors, chunks, n_chunks, groups, n_groups, zero_grad, nullptr, stream);
}

extern "C" size_t tsod_grad_norm_workspace_bytes(int64_t n_chunks) {
    return n_chunks > 0 && n_chunks <= INT32_MAX ? (size_t)n_chunks * sizeof(double) : 0;
}

extern "C" int tsod_grad_norm_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks,
                                  int64_t n_chunks, float max_norm, tsod_grad_norm_result *result, void *workspace,
                                  size_t workspace_bytes, tsod_stream_t stream) {
    const int rc = check_work_list(table, n_tensors, chunks, n_chunks);
    if (rc != TSOD_OK) return rc;
    TSOD_REQUIRE(result && workspace, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(max_norm >= 0.f, TSOD_ERR_INVALID_ARG);                                  // false for a NaN too
    TSOD_REQUIRE(workspace_bytes >= tsod_grad_norm_workspace_bytes(n_chunks), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((((uintptr_t)workspace | (uintptr_t)result) & 7u) == 0, TSOD_ERR_ALIGNMENT);
    double *partials = (double *)workspace;
    int n_partials = 0;
    if (n_tensors > 0 && n_chunks > 0) {
        n_partials = (int)n_chunks;
        grad_norm_partial_kernel<<<dim3((unsigned)n_chunks), dim3(kThreads), 0, tsod_stream(stream)>>>(table, n_tensors, chunks,
                                                                                                     partials);
    }
    grad_norm_finish_kernel<<<dim3(1), dim3(kThreads), 0, tsod_stream(stream)>>>(partials, n_partials, max_norm, result);
    return tsod_launch_status();
}

extern "C" int tsod_grad_scale_f32(const tsod_adamw_tensor *table, int32_t n_tensors, const tsod_adamw_chunk *chunks,
                                   int64_t n_chunks, const tsod_grad_norm_result *clip, tsod_stream_t stream) {
    const int rc = check_work_list(table, n_tensors, chunks, n_chunks);
    if (rc != TSOD_OK) return rc;
    TSOD_REQUIRE(clip, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(((uintptr_t)clip & 7u) == 0, TSOD_ERR_ALIGNMENT);
    if (n_tensors == 0 || n_chunks == 0) return TSOD_OK;
    grad_scale_kernel<<<dim3((unsigned)n_chunks), dim3(kThreads), 0, tsod_stream(stream)>>>(table, n_tensors, chunks, clip);
    return tsod_launch_status();
}

extern "C" int tsod_grad_norm_host_f32(const float *const *grads, const int64_t *numels, int32_t n_tensors, float max_norm,
                                       tsod_grad_norm_result *result) {
    TSOD_REQUIRE(grads && numels && result && n_tensors >= 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(max_norm >= 0.f, TSOD_ERR_INVALID_ARG);
    int64_t n_chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        TSOD_REQUIRE(numels[i] >= 0 && (grads[i] || numels[i] == 0), TSOD_ERR_INVALID_ARG);
        n_chunks += tsod_cdiv(numels[i], kChunk);
    }
    TSOD_REQUIRE(n_chunks <= INT32_MAX, TSOD_ERR_INVALID_ARG);
    // the work list of hip_ops.adamw_chunks: tensor by tensor, pieces ascending, no chunk for an empty tensor
    // (partial k goes to the finish's thread k % 256 as it is made: every thread gets its partials in ascending order)
    double v[kThreads], fin[kThreads] = {};
    int64_t k = 0;
    for (int i = 0; i < n_tensors; ++i)
        for (int64_t first = 0; first < numels[i]; first += kChunk, ++k) {
            const int64_t left = numels[i] - first;
            const int n = left < kChunk ? (int)left : kChunk;
            for (int t = 0; t < kThreads; ++t) v[t] = host_thread_sum(grads[i] + first, n, t);
            double &acc = fin[k & (kThreads - 1)];
            acc = acc + host_tree_sum_256(v);
        }
    *result = grad_norm_record(host_tree_sum_256(fin), max_norm, n_chunks == 0);
    return TSOD_OK;
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
