// tsod_internal.h -- helpers shared by the HIP translation units of libtsod.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tsod.h"

#define TSOD_WAVE 64

static inline hipStream_t tsod_stream(tsod_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

static inline int tsod_launch_status() {
    return hipGetLastError() == hipSuccess ? TSOD_OK : TSOD_ERR_LAUNCH;
}

static inline bool tsod_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static inline int64_t tsod_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

static inline size_t tsod_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#define TSOD_REQUIRE(cond, code) \
    do {                         \
        if (!(cond)) return (code); \
    } while (0)


// ---- range words (include/tsod.h "Range words"): the abs-max of a tensor as TSOD_AMAX_WORDS u32 words, TSOD_AMAX_STRIDE bytes
// apart (the bit pattern of a non-negative float orders like the float); the tensor's abs-max is the largest word.  A producer
// adds ONE no-return agent-scope atomicMax per workgroup, to word (block % TSOD_AMAX_WORDS): measured on MI355X
// (scripts/micro/amax_atomics.hip) 64 words at a 64-byte stride cost a launch of 1 024 / 4 096 / 16 384 workgroups that all end
// together -0.1 / +0.6 / +0.6 us, ONE word +10.6 / +45 / +178 us (11.5 ns per serialised atomic), 4-byte stride +3.8 / +18 / +68 us.
#ifdef __HIPCC__
#define TSOD_AMAX_STRIDE_WORDS (TSOD_AMAX_STRIDE / 4)
__device__ __forceinline__ float tsod_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// max over a 4-wave workgroup through LDS (`scr`: 4 floats; two barriers); every thread gets it
__device__ __forceinline__ float tsod_block_max(float v, float *scr, int tid) {
    v = tsod_wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) scr[tid >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(scr[0], scr[1]), fmaxf(scr[2], scr[3]));
}
// Every thread of the workgroup calls this (uniformly) with the largest |value| it stored (>= 0; fmaxf drops NaN, a NaN output
// shows up in the consumer's range flag instead).  `smem`: >= blockDim.x / 64 floats of LDS; other waves may still be using
// OTHER parts of the array it belongs to - the first barrier makes the words free, the second publishes them.
__device__ __forceinline__ void tsod_amax_commit(unsigned *amax, float mx, float *smem, int tid, int nthreads) {
    mx = tsod_wave_max(mx);
    __syncthreads();
    if ((tid & 63) == 0) smem[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < nthreads / 64; ++w) mx = fmaxf(mx, smem[w]);
        atomicMax(amax + (blockIdx.x % TSOD_AMAX_WORDS) * TSOD_AMAX_STRIDE_WORDS, __float_as_uint(mx));
    }
}
// wave-uniform largest word (bits of the tensor's abs-max so far); every lane of a full wave calls it
__device__ __forceinline__ unsigned tsod_amax_reduce_bits(unsigned mine) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned other = (unsigned)__shfl_xor((int)mine, o); mine = other > mine ? other : mine; }
    return (unsigned)__builtin_amdgcn_readfirstlane((int)mine);
}
static_assert(TSOD_AMAX_WORDS == 64, "one word per lane of a wave");
// utils/loc_bbox_iou.py:29-61 (loc2bbox) for one box, op for op (the library is built with -ffp-contract=off): the one decode
// of tsod_rpn_decode_f32, tsod_proposal_decode_f32, tsod_loc2bbox_f32, tsod_detections_f32 and tsod_roi_losses_f32
struct tsod_box { float x1, y1, x2, y2; };
__device__ __forceinline__ tsod_box tsod_decode_box(float ax1, float ay1, float ax2, float ay2,
                                                    float dx, float dy, float dw, float dh) {
    const float w = ax2 - ax1;
    const float h = ay2 - ay1;
    const float cx = ax1 + 0.5f * w;
    const float cy = ay1 + 0.5f * h;
    const float ncx = dx * w + cx;
    const float ncy = dy * h + cy;
    const float nw = expf(dw) * w;
    const float nh = expf(dh) * h;
    tsod_box o;
    o.x1 = ncx - 0.5f * nw;
    o.y1 = ncy - 0.5f * nh;
    o.x2 = ncx + 0.5f * nw;
    o.y2 = ncy + 0.5f * nh;
    return o;
}
// Arg-max / max of one row of n_class logits by one full wave, in torch.max's order (quirk Q11): a NaN is larger than every
// number, equal values (two NaNs included) go to the lower column.  Every lane returns the same (best, bi): the one rule of
// tsod_detections_f32 and tsod_roi_losses_f32.
__device__ __forceinline__ bool tsod_argmax_takes(float v, int c, float best, int bi) {
    if (c == 0x7fffffff) return false;                           // the other lane held no column
    if (bi == 0x7fffffff) return true;
    const bool vn = v != v, bn = best != best;
    if (vn || bn) return vn && (!bn || c < bi);
    return v > best || (v == best && c < bi);
}
__device__ __forceinline__ void tsod_wave_argmax(const float *s, int n_class, int lane, float &best, int &bi) {
    best = -INFINITY;
    bi = 0x7fffffff;
    for (int c = lane; c < n_class; c += 64) {
        const float v = s[c];
        if (tsod_argmax_takes(v, c, best, bi)) { best = v; bi = c; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (tsod_argmax_takes(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
}
// ---- RoI geometry of roi_pool.hip's forward kernels and feature_grads.hip's backward: one definition, so that the two cannot
// disagree about which pixels a bin reads.
// nets/classify.py:35-36: a RoI in image coordinates -> feature-map coordinates (divide by the image side, multiply by the map's)
__device__ __forceinline__ float4 tsod_roi_to_map(float4 rr, float img_h, float img_w, int Hf, int Wf) {
    return make_float4(rr.x / img_w * (float)Wf, rr.y / img_h * (float)Hf, rr.z / img_w * (float)Wf, rr.w / img_h * (float)Hf);
}
// torchvision RoIPool: round() half away from zero, +1 extents
struct tsod_pool_geom {
    int b, sw, sh, rw, rh;
};
__device__ __forceinline__ tsod_pool_geom tsod_roi_pool_geom(float bidx, float x1, float y1, float x2, float y2, float scale) {
    tsod_pool_geom g;
    g.b = (int)bidx;
    g.sw = (int)roundf(x1 * scale);
    g.sh = (int)roundf(y1 * scale);
    const int ew = (int)roundf(x2 * scale);
    const int eh = (int)roundf(y2 * scale);
    g.rw = max(ew - g.sw + 1, 1);
    g.rh = max(eh - g.sh + 1, 1);
    return g;
}
// bin p of a float bin size: [lo, hi) = [floor(p bin), ceil((p+1) bin)) + start, clamped to [0, limit]
__device__ __forceinline__ void tsod_bin_range(int p, float bin, int start, int limit, int &lo, int &hi) {
    lo = (int)floorf((float)p * bin) + start;
    hi = (int)ceilf((float)(p + 1) * bin) + start;
    lo = min(max(lo, 0), limit);
    hi = min(max(hi, 0), limit);
}
// torchvision.ops.roi_align (ops/cpu/roi_align_kernel.cpp + roi_align_common.h)
struct tsod_align_geom {
    int b, grid_h, grid_w;
    float start_h, start_w, bin_h, bin_w, count;
};
__device__ __forceinline__ tsod_align_geom tsod_roi_align_geom(float bidx, float x1, float y1, float x2, float y2, float scale,
                                                               int PH, int PW, int sampling_ratio, int aligned) {
    tsod_align_geom g;
    g.b = (int)bidx;
    const float offset = aligned ? 0.5f : 0.f;
    g.start_w = x1 * scale - offset;
    g.start_h = y1 * scale - offset;
    const float end_w = x2 * scale - offset, end_h = y2 * scale - offset;
    float rw = end_w - g.start_w, rh = end_h - g.start_h;
    if (!aligned) { rw = fmaxf(rw, 1.f); rh = fmaxf(rh, 1.f); }
    g.bin_h = rh / (float)PH;
    g.bin_w = rw / (float)PW;
    g.grid_h = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)PH);
    g.grid_w = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / (float)PW);
    g.count = (float)max(g.grid_h * g.grid_w, 1);
    return g;
}
// The sample rule as macros, not functions: they expand to the forward's original statements, so roi_pool.hip's kernels keep
// their instruction stream (a function boundary here changes the register allocation of roi_align_kernel).
// Coordinate of sample i of bin p along one axis:
#define TSOD_ALIGN_SAMPLE(start, bin, grid, p, i) ((start) + (float)(p) * (bin) + ((float)(i) + .5f) * (bin) / (float)(grid))
// The bilinear rule of the sample (yy, xx): `continue` when it lies outside [-1, H] x [-1, W] (it contributes 0); else clamp
// at 0, low = (int), high = low + 1 (both H - 1 / W - 1 at the border, where the coordinate becomes low) and ly / lx =
// coordinate - low (the weight of high; 1 - it is the weight of low).  Declares y_low, y_high, x_low, x_high, ly, lx.
#define TSOD_ALIGN_BILINEAR_OR_CONTINUE(yy, xx, Hf, Wf)                                                          \
    float y = (yy), x = (xx);                                                                                 \
    if (y < -1.f || y > (float)(Hf) || x < -1.f || x > (float)(Wf)) continue;                                 \
    if (y <= 0.f) y = 0.f;                                                                                    \
    if (x <= 0.f) x = 0.f;                                                                                    \
    int y_low = (int)y, x_low = (int)x, y_high, x_high;                                                       \
    if (y_low >= (Hf) - 1) { y_high = y_low = (Hf) - 1; y = (float)y_low; } else y_high = y_low + 1;          \
    if (x_low >= (Wf) - 1) { x_high = x_low = (Wf) - 1; x = (float)x_low; } else x_high = x_low + 1;          \
    const float ly = y - (float)y_low, lx = x - (float)x_low
// utils/loc_bbox_iou.py:4-27 (bbox_iou, eps in the denominator, no +1) for one pair, op for op: the one expression of
// tsod_bbox_iou_f32 and tsod_eval_match_f32 (bit-equal under -ffp-contract=off)
__device__ __forceinline__ float tsod_bbox_iou(const float4 A, const float4 Bx, float eps) {
    const float tlx = fmaxf(A.x, Bx.x), tly = fmaxf(A.y, Bx.y);
    const float brx = fminf(A.z, Bx.z), bry = fminf(A.w, Bx.w);
    const float w = fmaxf(brx - tlx, 0.f), h = fmaxf(bry - tly, 0.f);
    const float ai = w * h;
    const float aa = (A.z - A.x) * (A.w - A.y);
    const float ab = (Bx.z - Bx.x) * (Bx.w - Bx.y);
    return ai / (aa + ab - ai + eps);
}
__device__ __forceinline__ float tsod_prelu(float v, float a) { return fmaxf(v, 0.f) + a * fminf(v, 0.f); }

// ---- fp16x2 (TSOD_PREC_FP16X2) pieces, shared by the conv library and the fused stem / bottleneck kernels
typedef float tsod_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 tsod_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int tsod_u32x4 __attribute__((ext_vector_type(4)));
// two elements as fp16 pieces of sc * x: hi = rne_f16(sc x), lo = rne_f16(sc x - hi) (the product by a power of two and the
// subtraction are exact in f32, so each piece is ONE rounding of an exact value).  Four instructions per pair on the
// mixed-precision FMA (v_fma_mixlo/mixhi_f16: f32 x f32 + f16 -> f16, written into one half of the destination): no separate
// scale multiply, no conversion of hi back to f32, no pack - the form with v_cvt_pk_f16_f32 / v_cvt_f32_f16 / v_sub_f32 took
// eight, and the split is what the fp16x2 K loops are short of issue slots for (`sc` wave-uniform).
__device__ __forceinline__ void tsod_split2_pair(float x0, float x1, float sc, unsigned &h, unsigned &l) {
    asm("v_fma_mixlo_f16 %0, %2, %4, 0\n\t"
        "v_fma_mixhi_f16 %0, %3, %4, 0\n\t"
        "v_fma_mixlo_f16 %1, %2, %4, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %3, %4, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(h), "=&v"(l) : "v"(x0), "v"(x1), "s"(sc));
}
// three piece products, smallest first: lo*hi, hi*lo, hi*hi
__device__ __forceinline__ void tsod_mfma3(tsod_f32x16 &acc, const tsod_u32x4 &wh, const tsod_u32x4 &wl, const tsod_u32x4 &ah,
                                           const tsod_u32x4 &al) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(tsod_f16x8, wl), __builtin_bit_cast(tsod_f16x8, ah), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(tsod_f16x8, wh), __builtin_bit_cast(tsod_f16x8, al), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(tsod_f16x8, wh), __builtin_bit_cast(tsod_f16x8, ah), acc, 0, 0, 0);
}
// fp16x2 activation exponent for a tensor whose abs-max has these bits: 2^e * absmax < 2^15 (fp16 ends at 65504), e in [-24, 24]
// (zero / subnormal abs-max: 24; inf: -24 - the range flag of the launch then reports the non-finite input)
__device__ __forceinline__ int tsod_fp16x2_exp_from_bits(unsigned bits) {
    const int e = 141 - (int)(bits >> 23);                 // 14 - (biased exponent - 127)
    return e < -24 ? -24 : (e > 24 ? 24 : e);
}
#endif
