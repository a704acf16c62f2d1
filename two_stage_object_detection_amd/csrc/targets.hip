// targets.hip -- training-side box ops: IoU arg-max assignment of anchors / proposals to ground-truth boxes.
// HBM / latency-bound integer + f32 box work on wave-level reductions, no MFMA.  -ffp-contract=off: the IoU
// expression rounds exactly like utils/loc_bbox_iou.py:17-26 (and tsod_bbox_iou_f32), so every threshold
// decision and every arg-max is the reference's.
//
// Replaces (reference file:line)
//   nets/frcnn_training.py:19-103   AnchorTargetCreator   (_calc_ious :43-68, _create_label :70-103, __call__ :28-41)
//   nets/frcnn_training.py:105-177  ProposalTargetCreator (__call__ :123-177)
//   utils/loc_bbox_iou.py:63-88     bbox2loc
// Both creators are deterministic in the reference ("first n by index"), and both are restated with their indexing
// quirks (oracle/targets.py T1-T4):
//   T1  anchor negatives are only touched when n_neg < 1, and then ALL of them are disabled (len() of a 1-tuple)
//   T2  the kept proposal labels are zeroed at positions equal to the ORIGINAL indices of the sampled negatives;
//       an original index >= the kept length is the reference's IndexError -> status word
//   T4  first maximum wins in both arg-max directions; the last ground-truth box claiming an anchor wins the override
#include "tsod_internal.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr float kF32Eps = 1.1920928955078125e-07f;   // torch.finfo(torch.float32).eps (utils/loc_bbox_iou.py:77)

__device__ __forceinline__ float iou_eps(const float4 A, const float4 B, float eps) {
    const float tlx = fmaxf(A.x, B.x), tly = fmaxf(A.y, B.y);
    const float brx = fminf(A.z, B.z), bry = fminf(A.w, B.w);
    const float w = fmaxf(brx - tlx, 0.f), h = fmaxf(bry - tly, 0.f);
    const float ai = w * h;
    const float aa = (A.z - A.x) * (A.w - A.y);
    const float ab = (B.z - B.x) * (B.w - B.y);
    return ai / (aa + ab - ai + eps);
}

__device__ __forceinline__ float4 bbox2loc_dev(const float4 s, const float4 d) {
    float w = s.z - s.x, h = s.w - s.y;
    const float cx = s.x + 0.5f * w, cy = s.y + 0.5f * h;
    const float bw = d.z - d.x, bh = d.w - d.y;
    const float bcx = d.x + 0.5f * bw, bcy = d.y + 0.5f * bh;
    w = fmaxf(w, kF32Eps);
    h = fmaxf(h, kF32Eps);
    return make_float4((bcx - cx) / w, (bcy - cy) / h, logf(bw / w), logf(bh / h));
}

// One kernel per step, for one image or a batch: the image index rides on blockIdx.y (or, for the two one-workgroup
// steps, on blockIdx.x), the kernel offsets its pointers by it, takes the image's box count from image_gt_count() and calls
// the step's __device__ ..._image() body, which sees ONE image's pointers and indexes with blockIdx.x only.  A single image is
// a batch of one whose count is passed by value (gt_counts == nullptr).  A workgroup never straddles two images, so every
// __syncthreads() below is reached by all threads of its workgroup with the same per-image trip count.

// row-wise torch.max(ious, dim=1): first maximum wins.  One thread per candidate box; the G ground-truth boxes are
// walked through LDS in chunks of 256.  cand = concat(a [na], b [nb]) (ProposalTargetCreator appends the gt boxes).
__device__ __forceinline__ void
rowmax_image(const float4 *__restrict__ a, int na, const float4 *__restrict__ b, int nb,
             const float4 *__restrict__ gt, int G, float eps, float *__restrict__ max_iou, int *__restrict__ argmax) {
    __shared__ float4 s_gt[256];
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int N = na + nb;
    const float4 box = n < na ? a[n] : (n < N ? b[n - na] : make_float4(0.f, 0.f, 0.f, 0.f));
    float best = G > 0 ? -INFINITY : 0.f;          // len(bbox) == 0: zeros (nets/frcnn_training.py:47-48, 140-143)
    int bi = 0;
    for (int g0 = 0; g0 < G; g0 += 256) {
        __syncthreads();
        if (g0 + (int)threadIdx.x < G) s_gt[threadIdx.x] = gt[g0 + threadIdx.x];
        __syncthreads();
        const int lim = min(256, G - g0);
        for (int j = 0; j < lim; ++j) {
            const float v = iou_eps(box, s_gt[j], eps);
            if (v > best) { best = v; bi = g0 + j; }
        }
    }
    if (n < N) { max_iou[n] = best; argmax[n] = bi; }
}

// image b's box count: gt_counts[b] clamped to [0, Gmax], or Gmax itself when gt_counts == nullptr (the single-image entry
// points: the count by value).  Gmax == 0: gt_counts is not read.
__device__ __forceinline__ int image_gt_count(const int *__restrict__ gt_counts, int b, int Gmax) {
    return gt_counts != nullptr && Gmax > 0 ? min(max(gt_counts[b], 0), Gmax) : Gmax;
}

// grid (ceil((na + Gmax) / 256) or ceil(na / 256), B).  Image b's candidates are concat(a + b * a_stride [na], gt[b][:G] when
// append_gt); its row maxima go to max_iou + b * max_stride bytes, its arg-maxima to argmax + b * arg_stride bytes.  A workgroup
// past this image's candidates leaves as a whole, before any barrier.
__global__ void __launch_bounds__(256)
rowmax_kernel(const float4 *__restrict__ a, int na, size_t a_stride, int append_gt, const float4 *__restrict__ gt,
              const int *__restrict__ gt_counts, int Gmax, float eps, char *__restrict__ max_iou, size_t max_stride,
              char *__restrict__ argmax, size_t arg_stride) {
    const int b = blockIdx.y;
    const int G = image_gt_count(gt_counts, b, Gmax);
    const int nb = append_gt ? G : 0;
    if ((int)blockIdx.x * 256 >= na + nb) return;
    const float4 *g = gt + (size_t)b * Gmax;
    rowmax_image(a + b * a_stride, na, g, nb, g, G, eps, reinterpret_cast<float *>(max_iou + b * max_stride),
                 reinterpret_cast<int *>(argmax + b * arg_stride));
}

// column-wise ious.argmax(dim=0): for every gt box the FIRST anchor of maximal IoU.  One workgroup per gt box.
__device__ __forceinline__ void
colargmax_image(const float4 *__restrict__ anchor, int A, const float4 *__restrict__ gt, float eps, int *__restrict__ gt_argmax) {
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const float4 g = gt[blockIdx.x];
    float best = -INFINITY;
    int bi = INT_MAX;
    for (int n = threadIdx.x; n < A; n += 256) {
        const float v = iou_eps(anchor[n], g, eps);
        if (v > best) { best = v; bi = n; }                          // n ascending per thread: strict > keeps the first
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (s_v[w] > best || (s_v[w] == best && s_i[w] < bi)) { best = s_v[w]; bi = s_i[w]; }
        gt_argmax[blockIdx.x] = bi == INT_MAX ? 0 : bi;
    }
}

// grid (Gmax, B): the surplus workgroups of an image (blockIdx.x >= its count) leave before touching memory
__global__ void __launch_bounds__(256)
colargmax_kernel(const float4 *__restrict__ anchor, int A, const float4 *__restrict__ gt, const int *__restrict__ gt_counts,
                 int Gmax, float eps, int *__restrict__ gt_argmax, size_t ws_stride /* ints */) {
    const int b = blockIdx.y;
    if ((int)blockIdx.x >= image_gt_count(gt_counts, b, Gmax)) return;
    colargmax_image(anchor, A, gt + (size_t)b * Gmax, eps, gt_argmax + b * ws_stride);
}

// exclusive prefix of one int per thread over a 1024-thread workgroup (wave shuffles + 16 wave totals in LDS);
// returns the exclusive prefix, *total gets the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int *s_wave /* [17] */, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    __syncthreads();
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < 16; ++w) { const int t = s_wave[w]; s_wave[w] = run; run += t; }
        s_wave[16] = run;
    }
    __syncthreads();
    *total = s_wave[16];
    return s_wave[wave] + inc - v;
}

// _create_label (:70-103) + the override loop of _calc_ious (:61-63).  ONE workgroup per image: the positive cap is a prefix
// count over all anchors in index order.
__device__ __forceinline__ void
anchor_label_image(const float *__restrict__ max_iou, int *__restrict__ argmax, const int *__restrict__ gt_argmax, int A, int G,
                   float pos_thr, float neg_thr, int n_pos, int n_sample, long long *__restrict__ label, int *__restrict__ flag) {
    __shared__ int s_wave[17];
    const int tid = threadIdx.x;
    const int chunk = (A + 1023) / 1024;
    const int lo = min(A, tid * chunk), hi = min(A, lo + chunk);
    for (int n = tid; n < A; n += 1024) {
        const float m = max_iou[n];
        long long l = -1;
        if (m < neg_thr) l = 0;
        if (m >= pos_thr) l = 1;
        label[n] = l;
    }
    __threadfence_block();
    __syncthreads();
    for (int g = tid; g < G; g += 1024) {
        const int a = gt_argmax[g];
        label[a] = 1;                                                  // label[gt_argmax_ious] = 1 (:84-85)
        bool last = true;                                              // T4: argmax_ious[gt_argmax_ious[i]] = i in gt order
        for (int g2 = g + 1; g2 < G; ++g2) last = last && gt_argmax[g2] != a;
        if (last) argmax[a] = g;
    }
    __threadfence_block();
    __syncthreads();
    int cnt = 0;
    for (int n = lo; n < hi; ++n) cnt += label[n] == 1;
    int total_pos;
    int rank = block_exclusive_scan(cnt, s_wave, &total_pos);
    if (total_pos > n_pos) {                                           // keep the first n_pos positives by index (:88-93)
        for (int n = lo; n < hi; ++n)
            if (label[n] == 1) { if (rank >= n_pos) label[n] = -1; ++rank; }
    }
    const int pos_length = min(total_pos, n_pos);
    const int n_neg = n_sample - pos_length;
    if (1 > n_neg) {                                                   // T1: len(neg_index) is the tuple's length, 1 (:96-99)
        for (int n = lo; n < hi; ++n)
            if (label[n] == 0) label[n] = -1;
    }
    if (tid == 0) *flag = pos_length > 0 ? 1 : 0;                      // (label > 0).any() (:33)
}

// grid (B): workgroup b owns image b.  ws = this call's workspace, ws_stride bytes per image: max_iou [A], gt_argmax at
// gt_argmax_off, flag at flag_off (the single-image layout, once per image).
__global__ void __launch_bounds__(1024)
anchor_label_kernel(char *__restrict__ ws, size_t ws_stride, size_t gt_argmax_off, size_t flag_off, int *__restrict__ argmax,
                    int A, const int *__restrict__ gt_counts, int Gmax, float pos_thr, float neg_thr, int n_pos, int n_sample,
                    long long *__restrict__ label) {
    const int b = blockIdx.x;
    char *w = ws + b * ws_stride;
    anchor_label_image(reinterpret_cast<const float *>(w), argmax + (size_t)b * A, reinterpret_cast<const int *>(w + gt_argmax_off), A,
                       image_gt_count(gt_counts, b, Gmax), pos_thr, neg_thr, n_pos, n_sample, label + (size_t)b * A,
                       reinterpret_cast<int *>(w + flag_off));
}

__device__ __forceinline__ void
anchor_loc_image(const float4 *__restrict__ anchor, int A, const float4 *__restrict__ gt, const int *__restrict__ argmax,
                 const int *__restrict__ flag, float4 *__restrict__ loc) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= A) return;
    loc[n] = *flag ? bbox2loc_dev(anchor[n], gt[argmax[n]]) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// grid (ceil(A / 256), B).  A flag of 1 means the image has a positive, hence ground truth: gt is read only then.
__global__ void __launch_bounds__(256)
anchor_loc_kernel(const float4 *__restrict__ anchor, int A, const float4 *__restrict__ gt, int Gmax,
                  const int *__restrict__ argmax, const char *__restrict__ ws, size_t ws_stride, size_t flag_off,
                  float4 *__restrict__ loc) {
    const int b = blockIdx.y;
    anchor_loc_image(anchor, A, gt + (size_t)b * Gmax, argmax + (size_t)b * A,
                     reinterpret_cast<const int *>(ws + b * ws_stride + flag_off), loc + (size_t)b * A);
}

// ProposalTargetCreator.__call__ after the row maxima: thresholds, "first n by index" selection, gathers, bbox2loc,
// labels and quirk T2.  ONE workgroup per image (the selection is a prefix count in index order).  Returns S, the rows kept
// (the same value in every thread).
__device__ __forceinline__ int
proposal_select_image(const float4 *__restrict__ roi, int R, const float4 *__restrict__ gt, int G,
                      const long long *__restrict__ gt_label, const float *__restrict__ max_iou, const int *__restrict__ assign,
                      int n_sample, int pos_per_image, float pos_thr, float neg_hi, float neg_lo,
                      float4 *__restrict__ sample_roi, float4 *__restrict__ gt_roi_loc, long long *__restrict__ gt_roi_label,
                      int *__restrict__ neg_orig /* [n_sample] scratch */, int *__restrict__ counts /* [4] */,
                      int *__restrict__ sample_src /* [n_sample] or nullptr: the candidate each slot came from */) {
    __shared__ int s_wave[17];
    const int tid = threadIdx.x;
    const int N = R + G;
    const int chunk = (N + 1023) / 1024;
    const int lo = min(N, tid * chunk), hi = min(N, lo + chunk);
    int cp = 0, cn = 0;
    for (int n = lo; n < hi; ++n) {
        const float m = max_iou[n];
        cp += m >= pos_thr;
        cn += (m < neg_hi) && (m >= neg_lo);
    }
    int total_pos, total_neg;
    int rp = block_exclusive_scan(cp, s_wave, &total_pos);
    int rn = block_exclusive_scan(cn, s_wave, &total_neg);
    const int pos_len = min(total_pos, pos_per_image);
    const int neg_len = max(0, min(total_neg, n_sample - pos_len));
    const int S = pos_len + neg_len;
    for (int n = lo; n < hi; ++n) {
        const float m = max_iou[n];
        const bool is_pos = m >= pos_thr, is_neg = (m < neg_hi) && (m >= neg_lo);
        int slots[2] = {-1, -1};
        if (is_pos) { if (rp < pos_len) slots[0] = rp; ++rp; }
        if (is_neg) { if (rn < neg_len) { slots[1] = pos_len + rn; neg_orig[rn] = n; } ++rn; }
        for (int q = 0; q < 2; ++q) {
            const int slot = slots[q];
            if (slot < 0) continue;
            const float4 box = n < R ? roi[n] : gt[n - R];
            sample_roi[slot] = box;
            if (sample_src != nullptr) sample_src[slot] = n;
            if (G > 0) {
                const int g = assign[n];
                gt_roi_loc[slot] = bbox2loc_dev(box, gt[g]);
                gt_roi_label[slot] = gt_label[g] + 1;
            } else {
                gt_roi_loc[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
                gt_roi_label[slot] = 0;
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    int bad = 0;
    if (G > 0) {                                                       // T2: gt_roi_label[neg_index] = 0 on the KEPT list
        for (int j = tid; j < neg_len; j += 1024) {
            const int v = neg_orig[j];
            if (v >= S) bad = 1; else gt_roi_label[v] = 0;
        }
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) { counts[0] = S; counts[1] = pos_len; counts[2] = neg_len; counts[3] = bad ? 1 : 0; }
    return S;
}

// grid (B): workgroup b owns image b.  ws_stride bytes of workspace per image: max_iou, assign at assign_off, neg_orig at
// neg_off (the single-image layout at R + Gmax candidates).  fill_rest != 0 (the batched call alone) defines the rows the image
// did not fill: zeros (-1 in sample_src) from S to n_sample; no other thread writes those rows, so no barrier is needed before
// them.  fill_rest == 0 (the single-image calls) leaves them untouched.
__global__ void __launch_bounds__(1024)
proposal_select_kernel(const float4 *__restrict__ roi, int R, const float4 *__restrict__ gt, const int *__restrict__ gt_counts,
                       int Gmax, const long long *__restrict__ gt_label, char *__restrict__ ws, size_t ws_stride,
                       size_t assign_off, size_t neg_off, int n_sample, int pos_per_image, float pos_thr, float neg_hi,
                       float neg_lo, float4 *__restrict__ sample_roi, float4 *__restrict__ gt_roi_loc,
                       long long *__restrict__ gt_roi_label, int *__restrict__ counts, int *__restrict__ sample_src, int fill_rest) {
    const int b = blockIdx.x;
    char *w = ws + b * ws_stride;
    const size_t row = (size_t)b * n_sample;
    int *src = sample_src != nullptr ? sample_src + row : nullptr;
    const int S = proposal_select_image(roi + (size_t)b * R, R, gt + (size_t)b * Gmax, image_gt_count(gt_counts, b, Gmax),
                                        gt_label + (size_t)b * Gmax, reinterpret_cast<const float *>(w),
                                        reinterpret_cast<const int *>(w + assign_off), n_sample, pos_per_image, pos_thr, neg_hi,
                                        neg_lo, sample_roi + row, gt_roi_loc + row, gt_roi_label + row,
                                        reinterpret_cast<int *>(w + neg_off), counts + 4 * b, src);
    if (!fill_rest) return;
    for (int j = S + (int)threadIdx.x; j < n_sample; j += 1024) {
        sample_roi[row + j] = make_float4(0.f, 0.f, 0.f, 0.f);
        gt_roi_loc[row + j] = make_float4(0.f, 0.f, 0.f, 0.f);
        gt_roi_label[row + j] = 0;
        if (src != nullptr) src[j] = -1;
    }
}

// utils/loc_bbox_iou.py:63-88 as a stand-alone op: one thread per box pair
__global__ void __launch_bounds__(256)
bbox2loc_kernel(const float4 *__restrict__ src, const float4 *__restrict__ dst, long n, float4 *__restrict__ out) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x)
        out[t] = bbox2loc_dev(src[t], dst[t]);
}

}  // namespace

extern "C" size_t tsod_anchor_targets_workspace_bytes(int32_t A, int32_t G) {
    if (A <= 0 || G < 0) return 0;
    return tsod_align_up((size_t)A * 4, 16) + tsod_align_up((size_t)(G > 0 ? G : 1) * 4, 16) + 16;
}

// The four launches (three when Gmax == 0) of both anchor entry points, for B images whose workspaces - the single-image layout
// at Gmax boxes: max_iou [A], gt_argmax, flag - lie back to back.  gt_counts == nullptr: every image has Gmax boxes (the
// single-image call, B = 1).  No argument checks: those are the entry points'.
static int launch_anchor_targets(const float *anchor, int32_t A, const float *bbox, const int32_t *gt_counts, int32_t B, int32_t Gmax,
                                 float pos_iou_thresh, float neg_iou_thresh, int32_t n_pos, int32_t n_sample, float *loc,
                                 int64_t *label, int32_t *argmax, void *workspace, tsod_stream_t stream) {
    char *ws = static_cast<char *>(workspace);
    const size_t stride = tsod_anchor_targets_workspace_bytes(A, Gmax);
    const size_t gt_argmax_off = tsod_align_up((size_t)A * 4, 16);
    const size_t flag_off = gt_argmax_off + tsod_align_up((size_t)(Gmax > 0 ? Gmax : 1) * 4, 16);
    hipStream_t s = tsod_stream(stream);
    const float4 *a4 = reinterpret_cast<const float4 *>(anchor), *g4 = reinterpret_cast<const float4 *>(bbox);
    hipLaunchKernelGGL(rowmax_kernel, dim3((A + 255) / 256, B), dim3(256), 0, s, a4, A, (size_t)0, 0, g4, gt_counts, Gmax, 1e-8f, ws,
                       stride, reinterpret_cast<char *>(argmax), (size_t)A * 4);
    if (Gmax > 0)
        hipLaunchKernelGGL(colargmax_kernel, dim3(Gmax, B), dim3(256), 0, s, a4, A, g4, gt_counts, Gmax, 1e-8f,
                           reinterpret_cast<int *>(ws + gt_argmax_off), stride / 4);
    hipLaunchKernelGGL(anchor_label_kernel, dim3(B), dim3(1024), 0, s, ws, stride, gt_argmax_off, flag_off, argmax, A, gt_counts,
                       Gmax, pos_iou_thresh, neg_iou_thresh, n_pos, n_sample, reinterpret_cast<long long *>(label));
    hipLaunchKernelGGL(anchor_loc_kernel, dim3((A + 255) / 256, B), dim3(256), 0, s, a4, A, g4, Gmax, argmax, ws, stride, flag_off,
                       reinterpret_cast<float4 *>(loc));
    return tsod_launch_status();
}

extern "C" int tsod_anchor_targets_f32(const float *anchor, int32_t A, const float *bbox, int32_t G, float pos_iou_thresh,
                                       float neg_iou_thresh, int32_t n_pos, int32_t n_sample, float *loc, int64_t *label,
                                       int32_t *argmax, void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(anchor && loc && label && argmax && (bbox || G == 0), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(A > 0 && G >= 0 && n_pos >= 0 && n_sample >= 0, TSOD_ERR_INVALID_ARG);
    // without ground truth max_iou = 0 everywhere: with pos_iou_thresh <= 0 it would be all positives and the offsets would
    // read a box that does not exist (the reference's bbox[argmax_ious] raises there).  With G > 0 every box exists: legal.
    TSOD_REQUIRE(G > 0 || pos_iou_thresh > 0.f, TSOD_ERR_INVALID_ARG);
    // n_pos > n_sample (pos_ratio > 1) can make n_sample - pos_length negative, where the reference's i[n_neg:] disables
    // only the last |n_neg| negatives; the label kernel does not restate that accident
    TSOD_REQUIRE(n_pos <= n_sample, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(tsod_aligned16(anchor) && tsod_aligned16(loc) && (G == 0 || tsod_aligned16(bbox)), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && workspace_bytes >= tsod_anchor_targets_workspace_bytes(A, G) && tsod_aligned16(workspace),
                 TSOD_ERR_WORKSPACE);
    return launch_anchor_targets(anchor, A, bbox, nullptr, 1, G, pos_iou_thresh, neg_iou_thresh, n_pos, n_sample, loc, label, argmax,
                                 workspace, stream);
}

extern "C" size_t tsod_proposal_targets_workspace_bytes(int32_t R, int32_t G, int32_t n_sample) {
    if (R < 0 || G < 0 || R + G <= 0 || n_sample <= 0) return 0;
    return 2 * tsod_align_up((size_t)(R + G) * 4, 16) + tsod_align_up((size_t)n_sample * 4, 16);
}

// The two launches of all three proposal entry points, for B images whose workspaces - the single-image layout at R + Gmax
// candidates: max_iou, assign, neg_orig - lie back to back.  gt_counts == nullptr: every image has Gmax boxes (the single-image
// calls, B = 1); sample_src may be nullptr; fill_rest: see proposal_select_kernel.  No argument checks.
static int launch_proposal_targets(const float *roi, int32_t R, const float *bbox, const int64_t *gt_label, const int32_t *gt_counts,
                                   int32_t B, int32_t Gmax, int32_t n_sample, int32_t pos_per_image, float pos_iou_thresh,
                                   float neg_iou_thresh_high, float neg_iou_thresh_low, float *sample_roi, float *gt_roi_loc,
                                   int64_t *gt_roi_label, int32_t *counts, int32_t *sample_src, int fill_rest, void *workspace,
                                   tsod_stream_t stream) {
    const int Nmax = R + Gmax;
    char *ws = static_cast<char *>(workspace);
    const size_t stride = tsod_proposal_targets_workspace_bytes(R, Gmax, n_sample);
    const size_t assign_off = tsod_align_up((size_t)Nmax * 4, 16), neg_off = 2 * assign_off;
    hipStream_t s = tsod_stream(stream);
    const float4 *r4 = reinterpret_cast<const float4 *>(roi), *g4 = reinterpret_cast<const float4 *>(bbox);
    // roi = torch.cat((roi, bbox)) (:133) is never materialised: candidate n >= R is gt box n - R
    hipLaunchKernelGGL(rowmax_kernel, dim3((Nmax + 255) / 256, B), dim3(256), 0, s, r4, R, (size_t)R, 1, g4, gt_counts, Gmax, 1e-8f,
                       ws, stride, ws + assign_off, stride);
    hipLaunchKernelGGL(proposal_select_kernel, dim3(B), dim3(1024), 0, s, r4, R, g4, gt_counts, Gmax,
                       reinterpret_cast<const long long *>(gt_label), ws, stride, assign_off, neg_off, n_sample, pos_per_image,
                       pos_iou_thresh, neg_iou_thresh_high, neg_iou_thresh_low, reinterpret_cast<float4 *>(sample_roi),
                       reinterpret_cast<float4 *>(gt_roi_loc), reinterpret_cast<long long *>(gt_roi_label), counts, sample_src,
                       fill_rest);
    return tsod_launch_status();
}

// the checks of both single-image proposal entry points; the rows behind counts[0] stay untouched
static int proposal_targets(const float *roi, int32_t R, const float *bbox, int32_t G, const int64_t *gt_label,
                            int32_t n_sample, int32_t pos_per_image, float pos_iou_thresh,
                            float neg_iou_thresh_high, float neg_iou_thresh_low, float *sample_roi,
                            float *gt_roi_loc, int64_t *gt_roi_label, int32_t *counts, void *workspace,
                            size_t workspace_bytes, int32_t *sample_src, tsod_stream_t stream) {
    TSOD_REQUIRE(sample_roi && gt_roi_loc && gt_roi_label && counts, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(R >= 0 && G >= 0 && R + G > 0 && n_sample > 0 && pos_per_image >= 0, TSOD_ERR_INVALID_ARG);
    // pos_per_image > n_sample (pos_ratio > 1): the reference's i[:n_sample - pos_length] takes a negative bound and drops only
    // the last negatives; the select kernel clamps neg_len at 0 instead, so the arguments are refused
    TSOD_REQUIRE(pos_per_image <= n_sample, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((roi || R == 0) && ((bbox && gt_label) || G == 0), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((R == 0 || tsod_aligned16(roi)) && (G == 0 || tsod_aligned16(bbox)) && tsod_aligned16(sample_roi) &&
                     tsod_aligned16(gt_roi_loc), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && workspace_bytes >= tsod_proposal_targets_workspace_bytes(R, G, n_sample) &&
                     tsod_aligned16(workspace), TSOD_ERR_WORKSPACE);
    return launch_proposal_targets(roi, R, bbox, gt_label, nullptr, 1, G, n_sample, pos_per_image, pos_iou_thresh,
                                   neg_iou_thresh_high, neg_iou_thresh_low, sample_roi, gt_roi_loc, gt_roi_label, counts, sample_src,
                                   0, workspace, stream);
}

extern "C" int tsod_proposal_targets_f32(const float *roi, int32_t R, const float *bbox, int32_t G, const int64_t *gt_label,
                                         int32_t n_sample, int32_t pos_per_image, float pos_iou_thresh,
                                         float neg_iou_thresh_high, float neg_iou_thresh_low, float *sample_roi,
                                         float *gt_roi_loc, int64_t *gt_roi_label, int32_t *counts, void *workspace,
                                         size_t workspace_bytes, tsod_stream_t stream) {
    return proposal_targets(roi, R, bbox, G, gt_label, n_sample, pos_per_image, pos_iou_thresh, neg_iou_thresh_high,
                            neg_iou_thresh_low, sample_roi, gt_roi_loc, gt_roi_label, counts, workspace, workspace_bytes,
                            nullptr, stream);
}

// the same, and sample_src[slot] = the row of cat(roi, bbox) the slot was taken from (keep_index, :165): < R a proposal,
// >= R the ground-truth box n - R.  What the backward of the RoI-head regression loss maps each sample back with.
extern "C" int tsod_proposal_targets_src_f32(const float *roi, int32_t R, const float *bbox, int32_t G, const int64_t *gt_label,
                                             int32_t n_sample, int32_t pos_per_image, float pos_iou_thresh,
                                             float neg_iou_thresh_high, float neg_iou_thresh_low, float *sample_roi,
                                             float *gt_roi_loc, int64_t *gt_roi_label, int32_t *counts, int32_t *sample_src,
                                             void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(sample_src, TSOD_ERR_INVALID_ARG);
    return proposal_targets(roi, R, bbox, G, gt_label, n_sample, pos_per_image, pos_iou_thresh, neg_iou_thresh_high,
                            neg_iou_thresh_low, sample_roi, gt_roi_loc, gt_roi_label, counts, workspace, workspace_bytes,
                            sample_src, stream);
}

constexpr int kMaxBatch = 65535;                     // the image index rides on gridDim.y

extern "C" size_t tsod_anchor_targets_batch_workspace_bytes(int32_t B, int32_t A, int32_t Gmax) {
    if (B <= 0 || B > kMaxBatch) return 0;
    return (size_t)B * tsod_anchor_targets_workspace_bytes(A, Gmax);
}

extern "C" int tsod_anchor_targets_batch_f32(const float *anchor, int32_t A, const float *bbox, const int32_t *gt_counts,
                                             int32_t B, int32_t Gmax, float pos_iou_thresh, float neg_iou_thresh, int32_t n_pos,
                                             int32_t n_sample, float *loc, int64_t *label, int32_t *argmax, void *workspace,
                                             size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(anchor && loc && label && argmax && ((bbox && gt_counts) || Gmax == 0), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && B <= kMaxBatch && A > 0 && Gmax >= 0 && n_pos >= 0 && n_sample >= 0, TSOD_ERR_INVALID_ARG);
    // an image without ground truth has max_iou = 0 everywhere: with pos_iou_thresh <= 0 it would be all positives and the
    // offsets would read a box that does not exist (the reference's bbox[argmax_ious] raises there)
    TSOD_REQUIRE(pos_iou_thresh > 0.f, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_pos <= n_sample, TSOD_ERR_INVALID_ARG);           // (as tsod_anchor_targets_f32)
    TSOD_REQUIRE(tsod_aligned16(anchor) && tsod_aligned16(loc) && (Gmax == 0 || tsod_aligned16(bbox)), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && workspace_bytes >= tsod_anchor_targets_batch_workspace_bytes(B, A, Gmax) && tsod_aligned16(workspace),
                 TSOD_ERR_WORKSPACE);
    return launch_anchor_targets(anchor, A, bbox, gt_counts, B, Gmax, pos_iou_thresh, neg_iou_thresh, n_pos, n_sample, loc, label,
                                 argmax, workspace, stream);
}

extern "C" size_t tsod_proposal_targets_batch_workspace_bytes(int32_t B, int32_t R, int32_t Gmax, int32_t n_sample) {
    if (B <= 0 || B > kMaxBatch) return 0;
    return (size_t)B * tsod_proposal_targets_workspace_bytes(R, Gmax, n_sample);
}

// sample_src may be NULL; the rows behind counts[b][0] are written (fill_rest = 1)
extern "C" int tsod_proposal_targets_batch_f32(const float *roi, int32_t R, const float *bbox, const int64_t *gt_label,
                                               const int32_t *gt_counts, int32_t B, int32_t Gmax, int32_t n_sample,
                                               int32_t pos_per_image, float pos_iou_thresh, float neg_iou_thresh_high,
                                               float neg_iou_thresh_low, float *sample_roi, float *gt_roi_loc,
                                               int64_t *gt_roi_label, int32_t *counts, int32_t *sample_src, void *workspace,
                                               size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(sample_roi && gt_roi_loc && gt_roi_label && counts, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && B <= kMaxBatch && R >= 0 && Gmax >= 0 && R + Gmax > 0 && n_sample > 0 && pos_per_image >= 0,
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(pos_per_image <= n_sample, TSOD_ERR_INVALID_ARG);   // (as tsod_proposal_targets_f32)
    TSOD_REQUIRE((roi || R == 0) && ((bbox && gt_label && gt_counts) || Gmax == 0), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((R == 0 || tsod_aligned16(roi)) && (Gmax == 0 || tsod_aligned16(bbox)) && tsod_aligned16(sample_roi) &&
                     tsod_aligned16(gt_roi_loc), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && workspace_bytes >= tsod_proposal_targets_batch_workspace_bytes(B, R, Gmax, n_sample) &&
                     tsod_aligned16(workspace), TSOD_ERR_WORKSPACE);
    return launch_proposal_targets(roi, R, bbox, gt_label, gt_counts, B, Gmax, n_sample, pos_per_image, pos_iou_thresh,
                                   neg_iou_thresh_high, neg_iou_thresh_low, sample_roi, gt_roi_loc, gt_roi_label, counts, sample_src,
                                   1, workspace, stream);
}

extern "C" int tsod_bbox2loc_f32(const float *src, const float *dst, int64_t n, float *out, tsod_stream_t stream) {
    TSOD_REQUIRE(src && dst && out && n > 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(tsod_aligned16(src) && tsod_aligned16(dst) && tsod_aligned16(out), TSOD_ERR_ALIGNMENT);
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(bbox2loc_kernel, dim3(blocks), dim3(256), 0, tsod_stream(stream), reinterpret_cast<const float4 *>(src),
                       reinterpret_cast<const float4 *>(dst), (long)n, reinterpret_cast<float4 *>(out));
    return tsod_launch_status();
}
