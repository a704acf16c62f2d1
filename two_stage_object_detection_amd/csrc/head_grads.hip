// head_grads.hip -- the backward of FasterRCNNTrainer's four losses into the eight head parameters (frozen backbone).
//
// Replaces what autograd does behind the reference's `losses[-1].backward()` (nets/frcnn_training.py:179-342) for the
// parameters of rpn.loc / rpn.score (nets/rpn.py:86-88) and head.cls_loc / head.score (nets/classify.py:13,15):
//   tsod_rpn_losses_grad_f32   d loss / d (fused RPN output): smooth-L1 over label > 0 / (4 n_pos), cross-entropy with
//                              ignore_index = -1 / n_counted                                        (:220-238, :262-274)
//   tsod_roi_losses_grad_f32   d loss / d (fused head output) and d loss / d sample_roi through the regression TARGET
//                              bbox2loc(sample_roi, gt) (utils/loc_bbox_iou.py:63-88)              (:300-331, :165-168)
//   tsod_rpn_roi_scatter_f32   d sample_roi -> the proposal row (keep_index) -> the NMS keep with its 0,1,2,... padding (Q4)
//                              -> the sorted row -> the anchor; clamp mask (Q1 bounds, inclusive) and loc2bbox backward
//                              (nets/rpn.py:45-69, utils/loc_bbox_iou.py:29-61), added into d rpn_out
//   tsod_wgrad_f32             dW (+)= dY^T X, db (+)= sum_M dY on v_mfma_f32_32x32x2_f32, M split across workgroups
//
// Upstream gradients: `up` [5] on the device = d out / d (rpn_loc, rpn_cls, roi_loc, roi_cls, total); loss k receives
// up[k] + up[4], times inv_B (the batch mean).  Nothing synchronises with the host.
// Determinism: no float atomics anywhere.  Loss gradients are elementwise after per-image counts; the scatter sums the
// sample rows that reach one anchor (padded duplicates) in ascending sample order in ONE thread; the weight gradient sums
// its M-slices in slice order in a second launch.
// Empty sets follow torch's autograd: no positive -> the loc term gives zero gradients (the NaN loss has an empty
// regression_diff); no counted row -> the CE term gives zero; |d| == 0 -> abs's zero subgradient.
#include "grad_reduce.h"
#include <math.h>

namespace {

constexpr float kF32Eps = 1.1920928955078125e-07f;   // torch.finfo(torch.float32).eps (utils/loc_bbox_iou.py:77)

__device__ __forceinline__ double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// d smooth_l1(|t - p|) / d p, sigma2 = sigma^2 (torch.where picks one branch; abs' subgradient at 0 is 0)
__device__ __forceinline__ double smooth_l1_dp(double t, double p, double sigma2) {
    const double d = t - p, ad = fabs(d);
    return -sgn(d) * (ad < 1.0 / sigma2 ? sigma2 * ad : 1.0);
}

__device__ __forceinline__ double upstream(const float *up, int k, float inv_B) {
    return ((double)up[k] + (double)up[4]) * (double)inv_B;
}

// ---------------------------------------------------------------------------------------------------------------- RPN
constexpr int kCountThreads = 512;

// per image: n_rows[b] = (positives, counted rows) of gt_label [B][n] (labels outside {-1,0,1} count nowhere)
__global__ void __launch_bounds__(kCountThreads)
rpn_count_kernel(const int64_t *__restrict__ gt_label, long n, int32_t *__restrict__ n_rows) {
    __shared__ int s_pos[kCountThreads / 64], s_ce[kCountThreads / 64];
    const int b = blockIdx.x;
    const int64_t *lab = gt_label + (long)b * n;
    int pos = 0, ce = 0;
    for (long t = threadIdx.x; t < n; t += kCountThreads) {
        const int64_t l = lab[t];
        pos += l == 1;
        ce += l == 0 || l == 1;
    }
    for (int o = 32; o > 0; o >>= 1) { pos += __shfl_xor(pos, o); ce += __shfl_xor(ce, o); }
    if ((threadIdx.x & 63) == 0) { s_pos[threadIdx.x >> 6] = pos; s_ce[threadIdx.x >> 6] = ce; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kCountThreads / 64; ++w) { pos += s_pos[w]; ce += s_ce[w]; }
        n_rows[2 * b] = pos;
        n_rows[2 * b + 1] = ce;
    }
}

// one thread per (pixel row, column) of d rpn_out [B*n_pix][d_pitch]: loc columns [0,4A), logits [4A,6A), zeros after
__global__ void __launch_bounds__(256)
rpn_grad_kernel(const float *__restrict__ fused, int pitch, int A, long n_pix, int B, const float *__restrict__ gt_loc,
                const int64_t *__restrict__ gt_label, double sigma2, const float *__restrict__ up, float inv_B,
                const int32_t *__restrict__ n_rows, float *__restrict__ d_out, int d_pitch) {
    const long total = (long)B * n_pix * d_pitch;
    const long n = n_pix * A;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / d_pitch;
        const int c = (int)(i - row * d_pitch);
        const int b = (int)(row / n_pix);
        const long pix = row - (long)b * n_pix;
        const float *r = fused + row * pitch;
        double g = 0.0;
        if (c < 4 * A) {
            const int a = c >> 2, j = c & 3;
            const long t = pix * A + a;
            const int np = n_rows[2 * b];
            if (gt_label[(long)b * n + t] == 1 && np > 0)
                g = smooth_l1_dp(gt_loc[((long)b * n + t) * 4 + j], r[c], sigma2) * upstream(up, 0, inv_B) / (4.0 * np);
        } else if (c < 6 * A) {
            const int a = (c - 4 * A) >> 1, j = (c - 4 * A) & 1;
            const int64_t l = gt_label[(long)b * n + pix * A + a];
            const int nc = n_rows[2 * b + 1];
            if ((l == 0 || l == 1) && nc > 0) {
                const double s0 = r[4 * A + 2 * a], s1 = r[4 * A + 2 * a + 1];
                const double m = fmax(s0, s1);
                const double e0 = exp(s0 - m), e1 = exp(s1 - m);
                const double p = (j ? e1 : e0) / (e0 + e1);
                g = (p - (l == j ? 1.0 : 0.0)) * upstream(up, 1, inv_B) / (double)nc;
            }
        }
        d_out[i] = (float)g;
    }
}

// ---------------------------------------------------------------------------------------------------------------- RoI
constexpr int kRoiThreads = 256;

// Grid (S / 4, B): every workgroup counts its image's rows (S labels), then each of its waves takes one sample row: softmax in
// f64 over the n_class logits, the gt class's four offsets, d sample_roi of positive rows through bbox2loc's target.
__global__ void __launch_bounds__(kRoiThreads)
roi_grad_kernel(const float *__restrict__ cls_locs, int loc_pitch, const float *__restrict__ scores, int score_pitch,
                const float *__restrict__ sample_roi, const float *__restrict__ gt_roi_loc,
                const int64_t *__restrict__ gt_roi_label, int S, int n_class, double sigma2, const float *__restrict__ up,
                float inv_B, float *__restrict__ d_both, int d_pitch, float *__restrict__ d_sample_roi) {
    __shared__ int s_cnt[2 * (kRoiThreads / 64)];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int kWaves = kRoiThreads / 64;
    int pos = 0, ce = 0;
    for (int r = threadIdx.x; r < S; r += kRoiThreads) {
        const int64_t g = gt_roi_label[(long)b * S + r];
        ce += g >= 0 && g < n_class;
        pos += g > 0 && g < n_class;
    }
    for (int o = 32; o > 0; o >>= 1) { pos += __shfl_xor(pos, o); ce += __shfl_xor(ce, o); }
    if (lane == 0) { s_cnt[2 * wave] = pos; s_cnt[2 * wave + 1] = ce; }
    __syncthreads();
    pos = ce = 0;
    for (int w = 0; w < kWaves; ++w) { pos += s_cnt[2 * w]; ce += s_cnt[2 * w + 1]; }
    const double g_loc = pos > 0 ? upstream(up, 2, inv_B) / (4.0 * pos) : 0.0;
    const double g_ce = ce > 0 ? upstream(up, 3, inv_B) / (double)ce : 0.0;
    for (int r = blockIdx.x * kWaves + wave; r < S; r += gridDim.x * kWaves) {
        const long k = (long)b * S + r;
        const float *s = scores + k * score_pitch;
        const float *lp = cls_locs + k * loc_pitch;
        float *d = d_both + k * d_pitch;
        const int64_t g = gt_roi_label[k];
        const bool valid = g >= 0 && g < n_class;
        double m = -INFINITY;
        for (int c = lane; c < n_class; c += 64) m = fmax(m, (double)s[c]);
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        double e = 0.0;
        for (int c = lane; c < n_class; c += 64) e += exp((double)s[c] - m);
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
        double dl[4] = {0.0, 0.0, 0.0, 0.0};
        const bool positive = valid && g > 0;
        if (positive) {
            const float *t = gt_roi_loc + k * 4;
            for (int j = 0; j < 4; ++j) dl[j] = smooth_l1_dp(t[j], lp[4 * g + j], sigma2) * g_loc;
        }
        for (int c = lane; c < d_pitch; c += 64) {
            double v = 0.0;
            if (c < 4 * n_class) {
                if (positive && (c >> 2) == g) v = dl[c & 3];
            } else if (c < 5 * n_class) {
                const int q = c - 4 * n_class;
                if (valid) v = (exp((double)s[q] - m) / e - (q == g ? 1.0 : 0.0)) * g_ce;
            }
            d[c] = (float)v;
        }
        if (lane == 0) {
            // gt_roi_loc = bbox2loc(sample_roi, gt): d t = -d pred.  With w' = max(w, eps): d cx = -g_x / w',
            // d w' = -(g_x t_x + g_w) / w' (t_x = (bcx - cx) / w', t_w = log(bw / w')); torch.maximum passes all of the
            // gradient to w when w > eps, half of it at w == eps, none below.
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (positive) {
                const float4 sr = reinterpret_cast<const float4 *>(sample_roi)[k];
                const float4 t = reinterpret_cast<const float4 *>(gt_roi_loc)[k];
                const double w = (double)(sr.z - sr.x), h = (double)(sr.w - sr.y);
                const double wp = fmax(w, (double)kF32Eps), hp = fmax(h, (double)kF32Eps);
                const double mw = w > kF32Eps ? 1.0 : (w == kF32Eps ? 0.5 : 0.0);
                const double mh = h > kF32Eps ? 1.0 : (h == kF32Eps ? 0.5 : 0.0);
                const double gx = -dl[0], gy = -dl[1], gw = -dl[2], gh = -dl[3];
                const double dcx = -gx / wp, dcy = -gy / hp;
                const double dw = -(gx * t.x + gw) / wp * mw + 0.5 * dcx;
                const double dh = -(gy * t.y + gh) / hp * mh + 0.5 * dcy;
                o = make_float4((float)(dcx - dw), (float)(dcy - dh), (float)dw, (float)dh);
            }
            reinterpret_cast<float4 *>(d_sample_roi)[k] = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- scatter
constexpr int kScatterThreads = 256;
constexpr int kMaxScatterRows = 1024;

// One workgroup per image.  Phase 1: sample row r -> proposal row p = sample_src (< R) -> sorted row q = keep_idx[p] ->
// anchor a = sort_idx[q]; the unclamped box is re-decoded with tsod_decode_box (the forward's one decode) and the clamp's
// mask (lo <= v <= hi, torch.clamp's inclusive pass-through) and loc2bbox's backward give the row's d (dx, dy, dw, dh).
// Phase 2: the FIRST sample row of every anchor sums all rows of that anchor in ascending order and adds the sum to
// d rpn_out - distinct anchors are distinct addresses, so no two threads touch one word.
__global__ void __launch_bounds__(kScatterThreads)
scatter_kernel(const float *__restrict__ d_sample_roi, const int32_t *__restrict__ sample_src, int S, int R,
               const int32_t *__restrict__ keep_idx, const int32_t *__restrict__ sort_idx, int n_pre,
               const float *__restrict__ fused, int pitch, const float *__restrict__ anchors, int A, long n_pix,
               float clamp_x, float clamp_y, float *__restrict__ d_out, int d_pitch) {
    __shared__ int s_anchor[kMaxScatterRows];
    __shared__ float4 s_d[kMaxScatterRows];
    const int b = blockIdx.x;
    const long n = n_pix * A;
    for (int r = threadIdx.x; r < S; r += kScatterThreads) {
        const long k = (long)b * S + r;
        const float4 ds = reinterpret_cast<const float4 *>(d_sample_roi)[k];
        const int p = sample_src[k];
        int a = -1;
        float4 dl = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((ds.x != 0.f || ds.y != 0.f || ds.z != 0.f || ds.w != 0.f) && p >= 0 && p < R) {
            const int q = keep_idx[(long)b * R + p];
            const int t = (q >= 0 && q < n_pre) ? sort_idx[(long)b * n_pre + q] : -1;
            if (t >= 0 && t < n) {
                a = t;
                const float4 an = reinterpret_cast<const float4 *>(anchors)[t];
                const long pix = t / A;
                const int ai = (int)(t - pix * A);
                const float *l = fused + ((long)b * n_pix + pix) * pitch + 4 * ai;
                const tsod_box o = tsod_decode_box(an.x, an.y, an.z, an.w, l[0], l[1], l[2], l[3]);
                const float gx1 = (o.x1 >= 0.f && o.x1 <= clamp_x) ? ds.x : 0.f;
                const float gy1 = (o.y1 >= 0.f && o.y1 <= clamp_y) ? ds.y : 0.f;
                const float gx2 = (o.x2 >= 0.f && o.x2 <= clamp_x) ? ds.z : 0.f;
                const float gy2 = (o.y2 >= 0.f && o.y2 <= clamp_y) ? ds.w : 0.f;
                const float w = an.z - an.x, h = an.w - an.y;             // as tsod_decode_box computes them
                const float nw = expf(l[2]) * w, nh = expf(l[3]) * h;
                dl = make_float4((gx1 + gx2) * w, (gy1 + gy2) * h, 0.5f * (gx2 - gx1) * nw, 0.5f * (gy2 - gy1) * nh);
            }
        }
        s_anchor[r] = a;
        s_d[r] = dl;
    }
    __syncthreads();
    for (int r = threadIdx.x; r < S; r += kScatterThreads) {
        const int a = s_anchor[r];
        if (a < 0) continue;
        bool first = true;
        for (int j = 0; j < r && first; ++j) first = s_anchor[j] != a;
        if (!first) continue;
        float4 sum = s_d[r];
        for (int j = r + 1; j < S; ++j) {
            if (s_anchor[j] != a) continue;
            const float4 v = s_d[j];
            sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
        }
        const long pix = a / A;
        const int ai = (int)(a - pix * A);
        float *d = d_out + ((long)b * n_pix + pix) * d_pitch + 4 * ai;
        d[0] += sum.x; d[1] += sum.y; d[2] += sum.z; d[3] += sum.w;
    }
}

// ---------------------------------------------------------------------------------------------------------------- wgrad
// grad_reduce.h's tile with X read as it lies: gathered column k is column k.  wgrad_combine_kernel adds the slices' slabs in
// slice order: bit-identical results run to run.
__global__ void __launch_bounds__(kWgThreads)
wgrad_partial_kernel(const float *__restrict__ dy, long M, int N, int dy_pitch, const float *__restrict__ x, int K, int x_pitch,
                     tsod_wgrad_plan sh, float *__restrict__ part, float *__restrict__ part_b) {
    __shared__ float lds[kWgLdsFloats];
    // K % 4 == 0: a quad is all in or all out
    tsod_wgrad_tile(dy, M, N, dy_pitch, x, x_pitch, [K](int k) { return k < K ? k : -1; }, sh, part, part_b, lds);
}

// dW rows [0, n0) -> dw0 / db0, rows [n0, n0 + n1) -> dw1 / db1 (row pitch K); the slabs are summed in slice order.
__global__ void __launch_bounds__(256)
wgrad_combine_kernel(const float *__restrict__ part, const float *__restrict__ part_b, tsod_wgrad_plan sh, int K, int n0, int n1,
                     float *__restrict__ dw0, float *__restrict__ db0, float *__restrict__ dw1, float *__restrict__ db1,
                     int accumulate) {
    const long per_row = (long)K + 1;                                  // K weights + the bias
    const long total = (long)(n0 + n1) * per_row;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / per_row);
        const int k = (int)(i - (long)n * per_row);
        float s;
        float *dst;
        if (k < K) {
            s = tsod_sum_in_slice_order(part + (long)n * sh.k_pad + k, sh.n_pad * sh.k_pad, sh.splits);
            dst = n < n0 ? dw0 + (long)n * K + k : dw1 + (long)(n - n0) * K + k;
        } else {
            s = tsod_sum_in_slice_order(part_b + n, sh.n_pad, sh.splits);
            dst = n < n0 ? (db0 ? db0 + n : nullptr) : (db1 ? db1 + (n - n0) : nullptr);
            if (dst == nullptr) continue;
        }
        *dst = accumulate ? *dst + s : s;
    }
}

}  // namespace

extern "C" int tsod_rpn_losses_grad_f32(const float *rpn_out, int32_t pitch, int32_t A, int32_t B, int32_t n_pix,
                                        const float *gt_loc, const int64_t *gt_label, float sigma, const float *up, float inv_B,
                                        int32_t *n_rows, float *d_rpn_out, int32_t d_pitch, tsod_stream_t stream) {
    TSOD_REQUIRE(rpn_out && gt_loc && gt_label && up && n_rows && d_rpn_out, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(A > 0 && B > 0 && n_pix > 0 && pitch >= 6 * A && d_pitch >= 6 * A && sigma > 0.f, TSOD_ERR_INVALID_ARG);
    hipStream_t s = tsod_stream(stream);
    hipLaunchKernelGGL(rpn_count_kernel, dim3(B), dim3(kCountThreads), 0, s, gt_label, (long)n_pix * A, n_rows);
    const long total = (long)B * n_pix * d_pitch;
    const int blocks = (int)(tsod_cdiv(total, 256) < 8192 ? tsod_cdiv(total, 256) : 8192);
    hipLaunchKernelGGL(rpn_grad_kernel, dim3(blocks), dim3(256), 0, s, rpn_out, pitch, A, (long)n_pix, B, gt_loc, gt_label,
                       (double)sigma * (double)sigma, up, inv_B, (const int32_t *)n_rows, d_rpn_out, d_pitch);
    return tsod_launch_status();
}

extern "C" int tsod_roi_losses_grad_f32(const float *cls_locs, int32_t loc_pitch, const float *scores, int32_t score_pitch,
                                        const float *sample_roi, const float *gt_roi_loc, const int64_t *gt_roi_label,
                                        int32_t B, int32_t S, int32_t n_class, float sigma, const float *up, float inv_B,
                                        float *d_both, int32_t d_pitch, float *d_sample_roi, tsod_stream_t stream) {
    TSOD_REQUIRE(cls_locs && scores && sample_roi && gt_roi_loc && gt_roi_label && up && d_both && d_sample_roi,
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && S > 0 && n_class > 0 && loc_pitch >= 4 * n_class && score_pitch >= n_class &&
                 d_pitch >= 5 * n_class && sigma > 0.f, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(tsod_aligned16(sample_roi) && tsod_aligned16(gt_roi_loc) && tsod_aligned16(d_sample_roi), TSOD_ERR_ALIGNMENT);
    hipLaunchKernelGGL(roi_grad_kernel, dim3((S + kRoiThreads / 64 - 1) / (kRoiThreads / 64), B), dim3(kRoiThreads), 0, tsod_stream(stream), cls_locs, loc_pitch, scores,
                       score_pitch, sample_roi, gt_roi_loc, gt_roi_label, S, n_class, (double)sigma * (double)sigma, up, inv_B,
                       d_both, d_pitch, d_sample_roi);
    return tsod_launch_status();
}

extern "C" int tsod_rpn_roi_scatter_f32(const float *d_sample_roi, const int32_t *sample_src, int32_t B, int32_t S, int32_t R,
                                        const int32_t *keep_idx, const int32_t *sort_idx, int32_t n_pre, const float *rpn_out,
                                        int32_t pitch, const float *anchors, int32_t A, int32_t n_pix, float clamp_x,
                                        float clamp_y, float *d_rpn_out, int32_t d_pitch, tsod_stream_t stream) {
    TSOD_REQUIRE(d_sample_roi && sample_src && keep_idx && sort_idx && rpn_out && anchors && d_rpn_out, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && S > 0 && S <= kMaxScatterRows && R > 0 && n_pre > 0 && A > 0 && n_pix > 0 && pitch >= 4 * A &&
                 d_pitch >= 4 * A, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(tsod_aligned16(d_sample_roi) && tsod_aligned16(anchors), TSOD_ERR_ALIGNMENT);
    hipLaunchKernelGGL(scatter_kernel, dim3(B), dim3(kScatterThreads), 0, tsod_stream(stream), d_sample_roi, sample_src, S, R,
                       keep_idx, sort_idx, n_pre, rpn_out, pitch, anchors, A, (long)n_pix, clamp_x, clamp_y, d_rpn_out, d_pitch);
    return tsod_launch_status();
}

extern "C" size_t tsod_wgrad_workspace_bytes(int64_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return tsod_wgrad_plan_bytes(tsod_wgrad_plan_of(M, N, K, false));
}

extern "C" int tsod_wgrad_f32(const float *dy, int64_t M, int32_t N, int32_t dy_pitch, const float *x, int32_t K,
                              int32_t x_pitch, int32_t n0, float *dw0, float *db0, int32_t n1, float *dw1, float *db1,
                              int32_t accumulate, void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(dy && x && dw0 && (n1 == 0 || dw1), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(M > 0 && N > 0 && K > 0 && dy_pitch >= N && x_pitch >= K && n0 > 0 && n1 >= 0 && n0 + n1 <= N &&
                 (K & 3) == 0 && (x_pitch & 3) == 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(tsod_aligned16(x), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && workspace_bytes >= tsod_wgrad_workspace_bytes(M, N, K) && tsod_aligned16(workspace),
                 TSOD_ERR_WORKSPACE);
    const tsod_wgrad_plan sh = tsod_wgrad_plan_of(M, N, K, false);
    float *part = static_cast<float *>(workspace);
    float *part_b = tsod_wgrad_plan_bias(sh, part);
    hipStream_t s = tsod_stream(stream);
    hipLaunchKernelGGL(wgrad_partial_kernel, dim3(sh.n_tiles * sh.k_tiles, sh.splits), dim3(kWgThreads), 0, s,
                       dy, (long)M, N, dy_pitch, x, K, x_pitch, sh, part, part_b);
    const long total = (long)(n0 + n1) * (K + 1);
    const int blocks = (int)(tsod_cdiv(total, 256) < 4096 ? tsod_cdiv(total, 256) : 4096);
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(blocks), dim3(256), 0, s, (const float *)part, (const float *)part_b, sh, K,
                       n0, n1, dw0, db0, dw1, db1, accumulate ? 1 : 0);
    return tsod_launch_status();
}
