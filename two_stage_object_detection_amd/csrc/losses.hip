// losses.hip -- the four losses of the ground-truth-conditioned forward and the head's per-RoI predictions.
// Latency-bound reductions over a few thousand rows per image, no MFMA.
//
// Replaces (reference file:line)
//   nets/frcnn_training.py:220-238   _fast_rcnn_loc_loss (smooth L1 over the positives, divided by 4 * n_pos)
//   nets/frcnn_training.py:262-274   the RPN side: loc loss at sigma = rpn_sigma, F.cross_entropy(ignore_index=-1)
//   nets/frcnn_training.py:300-331   the head side: the gt class's offsets, loc2bbox, max over the raw logits, loc loss
//                                    at sigma = roi_sigma, F.cross_entropy over all n_class logits
//
// Deterministic by construction: one workgroup per image, every thread sums a fixed strided subset of the rows, the
// workgroup combines the partials in a fixed order (no atomics).  Sums are accumulated in f64 from the f32 inputs (the
// differences, the smooth L1 terms, log-sum-exp), so each loss is one f32 rounding from the exact value of the
// reference's formula whatever the summation order.  Torch's empty-set semantics are kept: no positive -> loc loss
// 0/0 = NaN, every anchor ignored -> cls loss NaN.  A label the reference would index out of bounds with is counted in
// status[b] and never used as an index.
#include "tsod_internal.h"
#include <math.h>

namespace {

constexpr int kRpnThreads = 512;
constexpr int kRoiThreads = 256;

__device__ __forceinline__ double smooth_l1(double d, double sigma2) {
    return d < 1.0 / sigma2 ? 0.5 * sigma2 * d * d : d - 0.5 / sigma2;
}

struct Partial {
    double loc, ce;
    int n_pos, n_ce, bad;
};

// Fixed-order tree over the workgroup (blockDim.x a power of two); thread 0 returns the total.
template <int N>
__device__ __forceinline__ Partial block_sum(Partial p, Partial *lds) {
    const int tid = threadIdx.x;
    lds[tid] = p;
    __syncthreads();
#pragma unroll
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) {
            Partial a = lds[tid];
            const Partial b = lds[tid + s];
            a.loc += b.loc;
            a.ce += b.ce;
            a.n_pos += b.n_pos;
            a.n_ce += b.n_ce;
            a.bad += b.bad;
            lds[tid] = a;
        }
        __syncthreads();
    }
    return lds[0];
}

// One workgroup per image.  Anchor t = pixel * A + a (quirk Q9): loc at row[4a..4a+3], (bg, fg) logits at row[4A+2a..].
__global__ void __launch_bounds__(kRpnThreads)
rpn_losses_kernel(const float *__restrict__ fused, int pitch, int A, long n_pix, const float *__restrict__ gt_loc,
                  const int64_t *__restrict__ gt_label, double sigma2, float *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ Partial lds[kRpnThreads];
    const int b = blockIdx.x;
    const long n = n_pix * A;
    const float *img = fused + (long)b * n_pix * pitch;
    const float4 *g4 = reinterpret_cast<const float4 *>(gt_loc) + (long)b * n;
    const int64_t *lab = gt_label + (long)b * n;
    Partial p = {0.0, 0.0, 0, 0, 0};
    for (long t = threadIdx.x; t < n; t += kRpnThreads) {
        const int64_t l = lab[t];
        if (l == -1) continue;                                   // ignore_index
        if (l != 0 && l != 1) { ++p.bad; continue; }             // F.cross_entropy raises IndexError
        const long pix = t / A;
        const int a = (int)(t - pix * A);
        const float *row = img + pix * pitch;
        const double s0 = row[4 * A + 2 * a], s1 = row[4 * A + 2 * a + 1];
        const double m = fmax(s0, s1);
        p.ce += m + log(exp(s0 - m) + exp(s1 - m)) - (l == 1 ? s1 : s0);
        ++p.n_ce;
        if (l == 1) {
            const float4 g = g4[t];
            p.loc += smooth_l1(fabs((double)g.x - (double)row[4 * a + 0]), sigma2) +
                     smooth_l1(fabs((double)g.y - (double)row[4 * a + 1]), sigma2) +
                     smooth_l1(fabs((double)g.z - (double)row[4 * a + 2]), sigma2) +
                     smooth_l1(fabs((double)g.w - (double)row[4 * a + 3]), sigma2);
            ++p.n_pos;
        }
    }
    const Partial s = block_sum<kRpnThreads>(p, lds);
    if (threadIdx.x == 0) {
        out[2 * b + 0] = (float)(s.loc / (4.0 * (double)s.n_pos));   // 0 / 0 = NaN without a positive, as the reference
        out[2 * b + 1] = (float)(s.ce / (double)s.n_ce);             // NaN when every anchor is ignored, as torch
        status[b] = s.bad;
    }
}

// One workgroup per image, one wave per RoI row (rows w, w + waves, ...): first-max arg-max over the raw logits (quirk
// Q11, tsod_wave_argmax: the rule of tsod_detections_f32; a NaN logit wins, as in torch.max, and makes the row's CE NaN),
// log-sum-exp in f64, then lane 0 gathers the gt class's offsets and decodes them.
__global__ void __launch_bounds__(kRoiThreads)
roi_losses_kernel(const float *__restrict__ cls_locs, int loc_pitch, const float *__restrict__ scores, int score_pitch,
                  const float *__restrict__ sample_roi, const float *__restrict__ gt_roi_loc,
                  const int64_t *__restrict__ gt_roi_label, int S, int n_class, double sigma2,
                  float *__restrict__ anchors_pred, int64_t *__restrict__ classes_pred, float *__restrict__ classes_score_pred,
                  float *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ Partial lds[kRoiThreads];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int kWaves = kRoiThreads / 64;
    Partial p = {0.0, 0.0, 0, 0, 0};
    for (int r = wave; r < S; r += kWaves) {
        const long k = (long)b * S + r;
        const float *s = scores + k * score_pitch;
        float best;
        int bi;
        tsod_wave_argmax(s, n_class, lane, best, bi);
        // every lane holds the same (best, bi); the xor butterfly below leaves the same f64 sum in every lane too
        double e = 0.0;
        for (int c = lane; c < n_class; c += 64) e += exp((double)s[c] - (double)best);
        for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
        if (lane == 0) {
            classes_pred[k] = bi;
            classes_score_pred[k] = best;
            const int64_t g = gt_roi_label[k];
            float *ap = anchors_pred + k * 4;
            if (g < 0 || g >= n_class) {                     // the reference's indexing raises IndexError: nothing is read
                ++p.bad;
                ap[0] = ap[1] = ap[2] = ap[3] = NAN;
                continue;
            }
            const float *l = cls_locs + k * loc_pitch + 4 * g;
            const float *roi = sample_roi + k * 4;
            const tsod_box o = tsod_decode_box(roi[0], roi[1], roi[2], roi[3], l[0], l[1], l[2], l[3]);
            ap[0] = o.x1; ap[1] = o.y1; ap[2] = o.x2; ap[3] = o.y2;
            p.ce += (double)best + log(e) - (double)s[g];
            ++p.n_ce;
            if (g > 0) {
                const float *t = gt_roi_loc + k * 4;
                for (int j = 0; j < 4; ++j) p.loc += smooth_l1(fabs((double)t[j] - (double)l[j]), sigma2);
                ++p.n_pos;
            }
        }
    }
    const Partial sum = block_sum<kRoiThreads>(p, lds);
    if (threadIdx.x == 0) {
        out[2 * b + 0] = (float)(sum.loc / (4.0 * (double)sum.n_pos));
        out[2 * b + 1] = (float)(sum.ce / (double)sum.n_ce);
        status[b] = sum.bad;
    }
}

}  // namespace

extern "C" int tsod_rpn_losses_f32(const float *rpn_out, int32_t pitch, int32_t A, int32_t B, int32_t n_pix,
                                   const float *gt_loc, const int64_t *gt_label, float sigma, float *out, int32_t *status,
                                   tsod_stream_t stream) {
    TSOD_REQUIRE(rpn_out && gt_loc && gt_label && out && status, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(A > 0 && B > 0 && n_pix > 0 && pitch >= 6 * A && sigma > 0.f, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(tsod_aligned16(gt_loc), TSOD_ERR_ALIGNMENT);
    hipLaunchKernelGGL(rpn_losses_kernel, dim3(B), dim3(kRpnThreads), 0, tsod_stream(stream), rpn_out, pitch, A,
                       (long)n_pix, gt_loc, gt_label, (double)sigma * (double)sigma, out, status);
    return tsod_launch_status();
}

extern "C" int tsod_roi_losses_f32(const float *cls_locs, int32_t loc_pitch, const float *scores, int32_t score_pitch,
                                   const float *sample_roi, const float *gt_roi_loc, const int64_t *gt_roi_label, int32_t B,
                                   int32_t S, int32_t n_class, float sigma, float *anchors_pred, int64_t *classes_pred,
                                   float *classes_score_pred, float *out, int32_t *status, tsod_stream_t stream) {
    TSOD_REQUIRE(cls_locs && scores && sample_roi && gt_roi_loc && gt_roi_label && anchors_pred && classes_pred &&
                 classes_score_pred && out && status, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && S > 0 && n_class > 0 && loc_pitch >= 4 * n_class && score_pitch >= n_class && sigma > 0.f,
                 TSOD_ERR_INVALID_ARG);
    hipLaunchKernelGGL(roi_losses_kernel, dim3(B), dim3(kRoiThreads), 0, tsod_stream(stream), cls_locs, loc_pitch, scores,
                       score_pitch, sample_roi, gt_roi_loc, gt_roi_label, S, n_class, (double)sigma * (double)sigma,
                       anchors_pred, classes_pred, classes_score_pred, out, status);
    return tsod_launch_status();
}
