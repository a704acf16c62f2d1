// eval_metrics.hip -- detection mAP on the GPU: COCOeval's evaluateImg + accumulate with an exact integer recall rule, once for
// both metrics.  Every kernel that sees a record is a template on its type: tsod_eval_record is the plain metric (DESIGN.md
// section 4.14: area "all" without any area comparison, no crowd / ignore regions, one cap), tsod_eval_record_coco adds
// COCOeval's area ranges, crowd regions, ignore rules and detection caps (section 4.25) behind `if constexpr`.
//
//   eval_match_kernel      one workgroup per image: order each class's detections (bitonic sort of (class, score, row) keys in
//                          LDS), cap at max_dets per class, then the greedy one-to-one match, one wave per class chain: lanes
//                          over the class's ground truth for the IoUs, then lanes over thresholds, each walking the IoUs for its
//                          own arg-max (max IoU, then max index).  Records go to a per-image staging slot; per-class GT counts
//                          are added with integer atomics.  COCO: the chain is walked once per area range over a GT list of
//                          not-ignored, then ignored ground truth, and a record carries its rank and a mask pair per range.
//   eval_offsets_kernel    one workgroup: exclusive scan of the per-image record counts on top of the device running total
//   eval_compact_kernel    copies the staged records to their place in the caller's record buffer (update order, image order)
//   radix_*                stable LSD radix sort of u64 keys + i32 payload: histogram / per-digit row scan / scatter passes of 8
//                          bits, local ranks from wave ballots in index order (deterministic, no atomics on the output path)
//   eval_keys_kernel, eval_segments_kernel, eval_ap_kernel
//                          the accumulate: key = class << 32 | order-inverted score bits, sorted; per-class segments; one
//                          workgroup per (class, threshold) - COCO: per (class, range, cap, threshold) - scans TP over its
//                          segment in order, counting every record - COCO: those the range does not ignore and the cap admits -,
//                          bins each counted position's f64 precision by floor(100 tp / npig) (LDS integer max), and the suffix
//                          max over the 101 bins is the envelope sampled at the 101 recall points.
//   launch_match, launch_accumulate
//                          the two launch sequences behind the four entry points, which keep their own argument checks.
// Every count is an integer; every f64 value comes from one division or a fixed-order sum: two runs give identical bits.
#include <type_traits>

#include "tsod_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxR = 8192;           // rows per image (the NMS limit); a row index fits the key's 13 low bits
constexpr int kMaxG = 1024;           // ground-truth boxes per image (LDS: 56 bytes each)
constexpr int kMaxT = 32;             // thresholds: bits of the TP mask
constexpr int kMaxClasses = 1 << 18;  // the class field of the per-image key (19 bits, all-ones reserved for padding)
constexpr int kRadixItems = 16;       // keys per thread per radix tile
constexpr int kRadixTile = kThreads * kRadixItems;
constexpr int kApItems = 16;          // positions per thread per chunk of the AP scan
constexpr float kIouEps = 1e-8f;
constexpr int kMaxA = 4;              // area ranges: the words of a COCO record's masks
constexpr int kMaxM = 4;              // detection caps of one COCO accumulate
constexpr unsigned kCrowdFlag = 1u << kMaxA;   // gflag: bit a = ignored in area range a, bit kMaxA = crowd
static_assert(sizeof(tsod_eval_record_coco) == 44, "hip_ops.EVAL_COCO_RECORD_INTS rows of int32");
template <typename Rec> constexpr bool is_coco = std::is_same<Rec, tsod_eval_record_coco>::value;   // else tsod_eval_record

struct DetCaps { int v[kMaxM]; };

__device__ __forceinline__ unsigned desc_score_bits(float s) {
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;                               // -0 == +0
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;                                               // ascending bits = descending score
}

// exclusive prefix over a 256-thread workgroup (4 waves); `scr` >= 4 ints; returns the prefix, *total = the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int *scr, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int other = __shfl_up(incl, o);
        if (lane >= o) incl += other;
    }
    __syncthreads();
    if (lane == 63) scr[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += scr[w];
    *total = scr[0] + scr[1] + scr[2] + scr[3];
    return before + incl - v;
}

// LDS written by some lanes of a wave, then read by others of the same wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane `l`'s value of v (l wave-uniform)
__device__ __forceinline__ float lane_value(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__device__ __forceinline__ long det_row(const int *__restrict__ keep, int b, int R, int j) {
    if (keep == nullptr) return j;
    const int r = keep[(long)b * R + j];
    return (r >= 0 && r < R) ? r : -1;
}

// ------------------------------------------------------------------------------------------------------ matching
// keys[p] of image b's candidate p < n: class << 45 | order-inverted score bits << 13 | p; all ones for dropped rows and padding
__device__ __forceinline__ void fill_detection_keys(const float *__restrict__ det, int R, const int *__restrict__ keep, int b, int n,
                                                    int C, int ignore_class, int NP, unsigned long long *keys) {
    const long drow0 = (long)b * R;
    for (int p = threadIdx.x; p < NP; p += kThreads) {
        unsigned long long key = ~0ull;
        if (p < n) {
            const long r = det_row(keep, b, R, p);
            if (r >= 0) {
                const float *q = det + (drow0 + r) * 6;
                const float s = q[4], c = q[5];
                if (!__builtin_isnan(s) && c >= 0.f && c < (float)C) {
                    const int cls = (int)c;
                    if (cls != ignore_class)
                        key = ((unsigned long long)cls << 45) | ((unsigned long long)desc_score_bits(s) << 13) | (unsigned)p;
                }
            }
        }
        keys[p] = key;
    }
}

// Orders the filled keys (call after a barrier) and caps every class segment at max_dets: comp[p] = the survivor's place in the
// image's record list.  Returns the number of survivors; ends on a barrier.
__device__ __forceinline__ int sort_and_cap_detections(unsigned long long *keys, unsigned short *comp, int NP, int max_dets,
                                                       int *scr) {
    const int tid = threadIdx.x;
    // ascending bitonic sort of the NP keys: (class, descending score, row); padding (all ones) last
    for (int k = 2; k <= NP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < NP; i += kThreads) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = keys[i], c = keys[ixj];
                    if ((a > c) == ((i & k) == 0)) { keys[i] = c; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }

    // survivors: the first max_dets of each class segment; compact index by a block scan over contiguous chunks
    const int per = (NP + kThreads - 1) / kThreads;
    const int p0 = min(tid * per, NP), p1 = min(p0 + per, NP);
    int mine = 0;
    for (int p = p0; p < p1; ++p) {
        const unsigned long long key = keys[p];
        if (key == ~0ull) break;
        const unsigned long long lo = (key >> 45) << 45;                 // first key of this class
        int a = 0, z = p;                                                // lower bound of lo in keys[0, p]
        while (a < z) { const int m = (a + z) >> 1; if (keys[m] < lo) a = m + 1; else z = m; }
        if (p - a < max_dets) ++mine;
    }
    int total = 0;
    int at = block_exclusive_scan(mine, scr, &total);
    for (int p = p0; p < p1; ++p) {
        const unsigned long long key = keys[p];
        if (key == ~0ull) break;
        const unsigned long long lo = (key >> 45) << 45;
        int a = 0, z = p;
        while (a < z) { const int m = (a + z) >> 1; if (keys[m] < lo) a = m + 1; else z = m; }
        if (p - a < max_dets) comp[p] = (unsigned short)at++;
    }
    __syncthreads();
    return total;
}

// what only the COCO metric passes to the match (all unused by the plain instantiation)
struct AreaRanges {
    const unsigned char *gt_crowd;    // [B][G] or NULL
    const float *gt_area;             // [B][G] or NULL: the boxes' own areas
    const float *lo, *hi;             // [A], both inclusive
    int A;
};

// IoU of detection A against a crowd region: the intersection of tsod_bbox_iou over the detection's own area
__device__ __forceinline__ float crowd_iou(const float4 A, const float4 Bx, float area_a, float eps) {
    const float tlx = fmaxf(A.x, Bx.x), tly = fmaxf(A.y, Bx.y);
    const float brx = fminf(A.z, Bx.z), bry = fminf(A.w, Bx.w);
    const float w = fmaxf(brx - tlx, 0.f), h = fmaxf(bry - tly, 0.f);
    return (w * h) / (area_a + eps);
}

// One workgroup per image.  Rec = tsod_eval_record is the metric of DESIGN.md section 4.14: no area is ever compared, a class's
// ground truth is one ascending list, a record is 12 bytes.  Rec = tsod_eval_record_coco adds COCOeval's ignore rules (section
// 4.25), all of them behind `coco`: per class chain the area ranges one after the other; for range a the class's GT list is the
// not-ignored ones (ascending), then the ignored ones (ascending), and a lane that found nothing in the first part walks the
// second, where a crowd region may be taken again.
template <typename Rec>
__global__ void __launch_bounds__(kThreads)
eval_match_kernel(const float *__restrict__ det, int R, const int *__restrict__ counts, const int *__restrict__ keep,
                  const int *__restrict__ n_kept, const float *__restrict__ gt_boxes, const long long *__restrict__ gt_labels,
                  const int *__restrict__ gt_counts, int G, const float *__restrict__ thr_in, int T, AreaRanges ranges, int C,
                  int max_dets, int ignore_class, int NP, Rec *__restrict__ stage, int *__restrict__ stage_counts,
                  unsigned long long *__restrict__ npig) {
    constexpr bool coco = is_coco<Rec>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);          // [NP]
    float4 *gbox = reinterpret_cast<float4 *>(keys + NP);                              // [G]
    int *gcls = reinterpret_cast<int *>(gbox + G);                                     // [G]
    unsigned *gflag = reinterpret_cast<unsigned *>(gcls + G);                          // [G], coco only: ignore bits per range, crowd
    unsigned *matched = coco ? gflag + G : gflag;                                      // [G]: bit t, for the chain being walked
    int *gmatch_list = reinterpret_cast<int *>(matched + G);                           // [4][G]: a wave's class GT list
    float *gmatch_iou = reinterpret_cast<float *>(gmatch_list + 4 * G);                // [4][G]: and their IoUs
    unsigned short *comp = reinterpret_cast<unsigned short *>(gmatch_iou + 4 * G);     // [NP]
    __shared__ float thr[kMaxT];
    __shared__ float alo[kMaxA], ahi[kMaxA];                                           // coco only (not allocated otherwise)
    __shared__ int scr[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long drow0 = (long)b * R;
    const int A = coco ? ranges.A : 1;

    int n = keep != nullptr ? n_kept[b] : counts[b];
    n = min(max(n, 0), R);
    const int gn = G > 0 ? min(max(gt_counts[b], 0), G) : 0;
    if (tid < T) thr[tid] = thr_in[tid];
    fill_detection_keys(det, R, keep, b, n, C, ignore_class, NP, keys);
    if constexpr (coco) {
        if (tid < A) { alo[tid] = ranges.lo[tid]; ahi[tid] = ranges.hi[tid]; }
        __syncthreads();
    }
    for (int g = tid; g < G; g += kThreads) {
        int cls = -1;
        unsigned flag = 0u;
        if (g < gn) {
            const float4 box = reinterpret_cast<const float4 *>(gt_boxes)[(long)b * G + g];
            gbox[g] = box;
            const long long l = gt_labels[(long)b * G + g];
            if (l >= 0 && l < C && l != ignore_class) {
                cls = (int)l;
                if constexpr (coco) {
                    const bool crowd = ranges.gt_crowd != nullptr && ranges.gt_crowd[(long)b * G + g] != 0;
                    const float area = ranges.gt_area != nullptr ? ranges.gt_area[(long)b * G + g]
                                                                 : (box.z - box.x) * (box.w - box.y);
                    if (crowd) flag = kCrowdFlag;
                    for (int a = 0; a < A; ++a) {
                        if (crowd || area < alo[a] || area > ahi[a]) flag |= 1u << a;
                        else atomicAdd(npig + (long)cls * A + a, 1ull);
                    }
                } else {
                    atomicAdd(npig + cls, 1ull);
                }
            }
        }
        gcls[g] = cls;
        if constexpr (coco) gflag[g] = flag;
        else matched[g] = 0u;                                            // coco: cleared per chain and range below
    }
    __syncthreads();

    const int total = sort_and_cap_detections(keys, comp, NP, max_dets, scr);
    if (tid == 0) stage_counts[b] = total;

    // greedy matching: class segments dealt round-robin to the four waves; a wave walks its chain in order.  Per detection the
    // lanes first compute its IoU with the class's ground truth (the class's GT list, built once per chain and range), then
    // lane t < T walks that list for threshold t on its own: the largest IoU >= t among the GT not yet matched at t, ties to the
    // later (higher) index.  matched[g] bit t is written only by lane t of the wave that owns g's class.
    int *glist = gmatch_list + wave * G;
    float *giou = gmatch_iou + wave * G;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const float th = lane < T ? thr[lane] : 0.f;
    int seg = 0;
    for (int base = 0; base < NP; base += 64) {
        const int p = base + lane;
        const unsigned long long key = p < NP ? keys[p] : ~0ull;
        const bool valid = key != ~0ull;
        const bool start = valid && (p == 0 || (keys[p - 1] >> 45) != (key >> 45));
        unsigned long long starts = __ballot(start);
        if (__ballot(valid) == 0ull) break;
        while (starts) {
            const int sl = __builtin_ctzll(starts);
            starts &= starts - 1;
            const int s = base + sl;
            if ((seg++ & 3) != wave) continue;
            const unsigned long long cls_hi = keys[s] >> 45;
            const int cls = (int)cls_hi;
            for (int a = 0; a < A; ++a) {
                const float lo = coco ? alo[a] : 0.f, hi = coco ? ahi[a] : 0.f;
                int nn = 0, nc = 0;                                     // not-ignored GT of the class, all of them
                for (unsigned part = 0; part < (coco ? 2u : 1u); ++part) {
                    for (int g0 = 0; g0 < gn; g0 += 64) {
                        const int g = g0 + lane;
                        bool in = g < gn && gcls[g] == cls;
                        if constexpr (coco) in = in && ((gflag[g] >> a) & 1u) == part;
                        const unsigned long long bal = __ballot(in);
                        if (in) glist[nc + __popcll(bal & lt)] = g;
                        nc += __popcll(bal);
                    }
                    if (part == 0u) nn = nc;
                }
                wave_sync();
                if constexpr (coco) {                                    // the ranges share the words; the wave_sync after the
                    for (int i = lane; i < nc; i += 64) matched[glist[i]] = 0u;   // first IoUs orders the clear before the walk
                }
                for (int q0 = 0; q0 < max_dets; q0 += 64) {
                    const int qi = q0 + lane, pq = s + qi;
                    const unsigned long long kq = (qi < max_dets && pq < NP) ? keys[pq] : ~0ull;
                    const bool mine = kq != ~0ull && (kq >> 45) == cls_hi;  // a prefix of the lanes: the keys are sorted
                    const int nv = __popcll(__ballot(mine));
                    float bx = 0.f, by = 0.f, bz = 0.f, bw = 0.f, sc = 0.f;
                    if (mine) {
                        const float *dq = det + (drow0 + det_row(keep, b, R, (int)(kq & 0x1FFFu))) * 6;
                        bx = dq[0]; by = dq[1]; bz = dq[2]; bw = dq[3]; sc = dq[4];
                    }
                    for (int qq = 0; qq < nv; ++qq) {
                        const float4 dbox = make_float4(lane_value(bx, qq), lane_value(by, qq), lane_value(bz, qq), lane_value(bw, qq));
                        const float darea = (dbox.z - dbox.x) * (dbox.w - dbox.y);   // coco only
                        for (int i = lane; i < nc; i += 64) {
                            const int g = glist[i];
                            bool crowd = false;
                            if constexpr (coco) crowd = gflag[g] & kCrowdFlag;
                            giou[i] = crowd ? crowd_iou(dbox, gbox[g], darea, kIouEps) : tsod_bbox_iou(dbox, gbox[g], kIouEps);
                        }
                        wave_sync();
                        float best = -__builtin_inff();
                        int bg = -1;
                        bool ignored = false;
                        if (lane < T) {
                            for (int i = 0; i < nn; ++i) {
                                const float v = giou[i];
                                const int g = glist[i];
                                if (v >= th && v >= best && !((matched[g] >> lane) & 1u)) { best = v; bg = g; }
                            }
                            if constexpr (coco) {
                                if (bg < 0) {                            // nothing not-ignored: the ignored part, crowd re-matchable
                                    for (int i = nn; i < nc; ++i) {
                                        const float v = giou[i];
                                        const int g = glist[i];
                                        if (v >= th && v >= best && (!((matched[g] >> lane) & 1u) || (gflag[g] & kCrowdFlag))) {
                                            best = v;
                                            bg = g;
                                        }
                                    }
                                    ignored = bg >= 0 || darea < lo || darea > hi;
                                }
                            }
                            if (bg >= 0) atomicOr(&matched[bg], 1u << lane);
                        }
                        const unsigned tp = (unsigned)__ballot(bg >= 0 && !ignored);   // lanes >= T: neither
                        const unsigned ig = (unsigned)__ballot(ignored);
                        if (lane == qq) {
                            Rec *rec = stage + drow0 + comp[s + qi];
                            if (a == 0) {
                                rec->score = sc;
                                rec->cls = cls;
                            }
                            if constexpr (coco) {
                                if (a == 0) {
                                    rec->rank = qi;
                                    for (int k = 1; k < kMaxA; ++k) { rec->tp_mask[k] = 0u; rec->ig_mask[k] = 0u; }
                                }
                                rec->tp_mask[a] = tp;
                                rec->ig_mask[a] = ig;
                            } else {
                                rec->tp_mask = tp;
                            }
                        }
                        wave_sync();
                    }
                    if (nv < 64) break;
                }
            }
        }
    }
}

// running total += counts, offsets[b] = running total before image b (update order, then image order)
__global__ void __launch_bounds__(kThreads)
eval_offsets_kernel(const int *__restrict__ counts, int B, long long *__restrict__ offsets, long long *__restrict__ n_records) {
    __shared__ int scr[4];
    long long carry = *n_records;
    for (int b0 = 0; b0 < B; b0 += kThreads) {
        const int b = b0 + threadIdx.x;
        const int v = b < B ? counts[b] : 0;
        int total = 0;
        const int ex = block_exclusive_scan(v, scr, &total);
        if (b < B) offsets[b] = carry + ex;
        carry += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) *n_records = carry;
}

template <typename Rec>
__global__ void __launch_bounds__(kThreads)
eval_compact_kernel(const Rec *__restrict__ stage, const int *__restrict__ counts, const long long *__restrict__ offsets, int R,
                    Rec *__restrict__ records, long long capacity) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= counts[b]) return;
    const long long dst = offsets[b] + j;
    if (dst < capacity) records[dst] = stage[(long)b * R + j];
}

// ------------------------------------------------------------------------------------------------------ radix sort
__device__ __forceinline__ long long live_count(long long n_max, const long long *n_dev) {
    if (n_dev == nullptr) return n_max;
    const long long n = *n_dev;
    return n < 0 ? 0 : (n < n_max ? n : n_max);
}

__global__ void __launch_bounds__(kThreads)
radix_hist_kernel(const unsigned long long *__restrict__ keys, long long n_max, const long long *__restrict__ n_dev, int shift,
                  unsigned digit_mask, int nblk, unsigned *__restrict__ hist) {
    __shared__ unsigned h[256];
    const long long n = live_count(n_max, n_dev);
    h[threadIdx.x] = 0u;
    __syncthreads();
    const long long tile = (long long)blockIdx.x * kRadixTile;
#pragma unroll 4
    for (int it = 0; it < kRadixItems; ++it) {
        const long long i = tile + it * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(unsigned)(keys[i] >> shift) & digit_mask], 1u);
    }
    __syncthreads();
    hist[(long)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// workgroup d: exclusive scan of hist[d][0..nblk) in place, totals[d] = the row's sum
__global__ void __launch_bounds__(kThreads)
radix_rowscan_kernel(unsigned *__restrict__ hist, int nblk, unsigned *__restrict__ totals) {
    __shared__ int scr[4];
    unsigned *row = hist + (long)blockIdx.x * nblk;
    unsigned carry = 0;
    for (int i0 = 0; i0 < nblk; i0 += kThreads) {
        const int i = i0 + threadIdx.x;
        const int v = i < nblk ? (int)row[i] : 0;
        int total = 0;
        const int ex = block_exclusive_scan(v, scr, &total);
        if (i < nblk) row[i] = carry + (unsigned)ex;
        carry += (unsigned)total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kThreads)
radix_scatter_kernel(const unsigned long long *__restrict__ keys_in, const int *__restrict__ vals_in, long long n_max,
                     const long long *__restrict__ n_dev, int shift, unsigned digit_mask, int nblk,
                     const unsigned *__restrict__ hist, const unsigned *__restrict__ totals,
                     unsigned long long *__restrict__ keys_out, int *__restrict__ vals_out) {
    __shared__ unsigned base[256];
    __shared__ unsigned running[256];
    __shared__ unsigned wcnt[4][256];
    __shared__ int scr[4];
    const long long n = live_count(n_max, n_dev);
    const long long tile = (long long)blockIdx.x * kRadixTile;
    if (tile >= n) return;                                            // uniform per workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int total = 0;
    const int ex = block_exclusive_scan((int)totals[tid], scr, &total);
    base[tid] = (unsigned)ex + hist[(long)tid * nblk + blockIdx.x];
    running[tid] = 0u;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int it = 0; it < kRadixItems; ++it) {
        const long long i = tile + it * kThreads + tid;
        const bool valid = i < n;
        const unsigned long long key = valid ? keys_in[i] : 0ull;
        const int val = valid ? (vals_in != nullptr ? vals_in[i] : (int)i) : 0;
        const unsigned d = (unsigned)(key >> shift) & digit_mask;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long m = __ballot((d >> bit) & 1u);
            peers &= ((d >> bit) & 1u) ? m : ~m;
        }
        wcnt[0][tid] = 0u; wcnt[1][tid] = 0u; wcnt[2][tid] = 0u; wcnt[3][tid] = 0u;
        __syncthreads();
        if (valid && (peers & lt) == 0ull) wcnt[wave][d] = (unsigned)__popcll(peers);
        __syncthreads();
        if (valid) {
            unsigned pos = base[d] + running[d] + (unsigned)__popcll(peers & lt);
            for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
            keys_out[pos] = key;
            vals_out[pos] = val;
        }
        __syncthreads();
        running[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        __syncthreads();
    }
}

struct SortWs {
    unsigned long long *alt_keys;
    int *alt_vals;
    unsigned *hist;
    unsigned *totals;
    size_t bytes;
};


SortWs sort_ws_layout(void *ws, long long n) {
    const long long nblk = tsod_cdiv(n, kRadixTile);
    SortWs w;
    char *p = static_cast<char *>(ws);
    size_t off = 0;
    w.alt_keys = reinterpret_cast<unsigned long long *>(p + off); off += tsod_align_up((size_t)n * 8, 256);
    w.alt_vals = reinterpret_cast<int *>(p + off);                off += tsod_align_up((size_t)n * 4, 256);
    w.hist = reinterpret_cast<unsigned *>(p + off);               off += tsod_align_up((size_t)nblk * 256 * 4, 256);
    w.totals = reinterpret_cast<unsigned *>(p + off);             off += tsod_align_up(256 * 4, 256);
    w.bytes = off;
    return w;
}

int launch_sort(const unsigned long long *keys_in, const int *vals_in, long long n, const long long *n_dev, int begin_bit,
                int end_bit, unsigned long long *keys_out, int *vals_out, const SortWs &w, hipStream_t st) {
    const int nblk = (int)tsod_cdiv(n, kRadixTile);
    const int passes = (int)tsod_cdiv(end_bit - begin_bit, 8);
    const unsigned long long *src_k = keys_in;
    const int *src_v = vals_in;                                      // NULL: the identity payload (first pass only)
    for (int i = 0; i < passes; ++i) {
        const bool to_out = ((passes - 1 - i) & 1) == 0;             // the last pass lands in the caller's output
        unsigned long long *dk = to_out ? keys_out : w.alt_keys;
        int *dv = to_out ? vals_out : w.alt_vals;
        const int shift = begin_bit + 8 * i;
        const unsigned digit_mask = (1u << (end_bit - shift < 8 ? end_bit - shift : 8)) - 1u;   // the last pass stops at end_bit
        hipLaunchKernelGGL(radix_hist_kernel, dim3(nblk), dim3(kThreads), 0, st, src_k, n, n_dev, shift, digit_mask, nblk,
                           w.hist);
        hipLaunchKernelGGL(radix_rowscan_kernel, dim3(256), dim3(kThreads), 0, st, w.hist, nblk, w.totals);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(kThreads), 0, st, src_k, src_v, n, n_dev, shift, digit_mask,
                           nblk, w.hist, w.totals, dk, dv);
        src_k = dk;
        src_v = dv;
    }
    return tsod_launch_status();
}

// ------------------------------------------------------------------------------------------------------ accumulate
template <typename Rec>
__global__ void __launch_bounds__(kThreads)
eval_keys_kernel(const Rec *__restrict__ records, long long n_max, const long long *__restrict__ n_dev,
                 unsigned long long *__restrict__ keys) {
    const long long n = live_count(n_max, n_dev);
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const Rec r = records[i];
    keys[i] = ((unsigned long long)(unsigned)r.cls << 32) | desc_score_bits(r.score);
}

// what the AP scan reads of a record, at its sorted position i: the TP mask, or for a COCO record planes of `plane` words each,
// (rank, tp_mask[0..4), ig_mask[0..4))
template <typename Rec> constexpr int kSortedPlanes = is_coco<Rec> ? 1 + 2 * kMaxA : 1;
__device__ __forceinline__ void store_sorted(unsigned *masks, long long, long long i, const tsod_eval_record &r) {
    masks[i] = r.tp_mask;
}
__device__ __forceinline__ void store_sorted(unsigned *masks, long long plane, long long i, const tsod_eval_record_coco &r) {
    masks[i] = (unsigned)r.rank;
#pragma unroll
    for (int a = 0; a < kMaxA; ++a) {
        masks[(1 + a) * plane + i] = r.tp_mask[a];
        masks[(1 + kMaxA + a) * plane + i] = r.ig_mask[a];
    }
}

// per-class [begin, end) of the sorted keys, and the TP masks in sorted order
template <typename Rec>
__global__ void __launch_bounds__(kThreads)
eval_segments_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ perm, const Rec *__restrict__ records,
                     long long n_max, const long long *__restrict__ n_dev, int *__restrict__ seg_begin,
                     int *__restrict__ seg_end, unsigned *__restrict__ masks) {
    const long long n = live_count(n_max, n_dev);
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(keys[i] >> 32);
    if (i == 0 || (int)(keys[i - 1] >> 32) != c) seg_begin[c] = (int)i;
    if (i == n - 1 || (int)(keys[i + 1] >> 32) != c) seg_end[c] = (int)(i + 1);
    store_sorted(masks, n_max, i, records[perm[i]]);
}

// workgroup (c, a, m, t), the plain metric's A = M = 1: TP / FP along the class's sorted segment, the precision envelope and its
// 101-point sample.  `sorted` holds store_sorted's planes.  Every position of a plain record counts; a COCO record counts when
// its rank is below cap[m] and range a does not ignore it at threshold t.
template <typename Rec>
__global__ void __launch_bounds__(kThreads)
eval_ap_kernel(const unsigned *__restrict__ sorted, long long plane, const int *__restrict__ seg_begin,
               const int *__restrict__ seg_end, const long long *__restrict__ npig, int A, int M, int T, DetCaps caps,
               double *__restrict__ ap, long long *__restrict__ tp_out, long long *__restrict__ fp_out,
               long long *__restrict__ fn_out, double *__restrict__ recall) {
    constexpr bool coco = is_coco<Rec>;
    __shared__ unsigned long long bins[101];
    __shared__ int scr[4];
    const int tid = threadIdx.x;
    const int t = blockIdx.x % T, m = (blockIdx.x / T) % M, a = (blockIdx.x / (T * M)) % A, c = blockIdx.x / (T * M * A);
    const unsigned cap = (unsigned)(m == 0 ? caps.v[0] : m == 1 ? caps.v[1] : m == 2 ? caps.v[2] : caps.v[3]);
    const unsigned *rank = sorted, *tpw = sorted + (coco ? (1 + a) * plane : 0), *igw = sorted + (1 + kMaxA + a) * plane;
    const int s = seg_begin[c], e = seg_end[c];
    const long long np = npig[(long)c * A + a];
    if (tid < 101) bins[tid] = 0ull;
    long long carry_tp = 0, carry_n = 0;
    for (int c0 = s; c0 < e; c0 += kThreads * kApItems) {
        const int j0 = c0 + tid * kApItems, j1 = min(j0 + kApItems, e);
        unsigned live = 0u, hit = 0u;                                 // bit j - j0: counted at all, counted as a TP
        for (int j = j0; j < j1; ++j) {
            unsigned l = 1u;
            if constexpr (coco) l = (rank[j] < cap && !((igw[j] >> t) & 1u)) ? 1u : 0u;
            live |= l << (j - j0);
            hit |= (l & (tpw[j] >> t)) << (j - j0);
        }
        // TP in the low half, counted records in the high half (the scan's first barrier also orders the bins' zeroing)
        int total = 0;
        const int ex = block_exclusive_scan(__popc(hit) | (__popc(live) << 16), scr, &total);
        if (np > 0) {
            long long tp = carry_tp + (ex & 0xFFFF), n = carry_n + (ex >> 16);
            int cur = -1;
            unsigned long long best = 0ull;
            for (int j = j0; j < j1; ++j) {
                if (!((live >> (j - j0)) & 1u)) continue;
                tp += (hit >> (j - j0)) & 1u;
                ++n;
                const double prec = (double)tp / (double)n;
                const long long q = (100 * tp) / np;
                const int bin = q < 100 ? (int)q : 100;
                if (bin != cur) {
                    if (cur >= 0) atomicMax(&bins[cur], best);
                    cur = bin;
                    best = 0ull;
                }
                const unsigned long long pb = (unsigned long long)__double_as_longlong(prec);
                best = pb > best ? pb : best;
            }
            if (cur >= 0) atomicMax(&bins[cur], best);
        }
        carry_tp += total & 0xFFFF;
        carry_n += total >> 16;
    }
    __syncthreads();
    if (tid == 0) {
        const long k = blockIdx.x;
        tp_out[k] = carry_tp;
        fp_out[k] = carry_n - carry_tp;
        fn_out[k] = np - carry_tp;
        if (np > 0) {
            unsigned long long env = 0ull;                            // the envelope, right to left (bits of doubles >= 0)
            for (int i = 100; i >= 0; --i) {
                env = bins[i] > env ? bins[i] : env;
                bins[i] = env;
            }
            double sum = 0.0;
            for (int i = 0; i <= 100; ++i) sum += __longlong_as_double((long long)bins[i]);
            ap[k] = sum / 101.0;
            recall[k] = (double)carry_tp / (double)np;
        } else {
            ap[k] = -1.0;
            recall[k] = -1.0;
        }
    }
}

int class_bits(int C) {
    int bits = 1;
    while (bits < 31 && (1ll << bits) < (long long)C) ++bits;
    return bits;
}

struct AccWs {
    unsigned long long *keys, *sorted_keys;
    int *perm;
    unsigned *masks;
    int *seg_begin, *seg_end;
    void *sort_ws;
    size_t sort_bytes, bytes;
};

AccWs acc_ws_layout(void *ws, long long capacity, int C, int mask_planes = 1) {
    AccWs w;
    char *p = static_cast<char *>(ws);
    size_t off = 0;
    w.keys = reinterpret_cast<unsigned long long *>(p + off);        off += tsod_align_up((size_t)capacity * 8, 256);
    w.sorted_keys = reinterpret_cast<unsigned long long *>(p + off); off += tsod_align_up((size_t)capacity * 8, 256);
    w.perm = reinterpret_cast<int *>(p + off);                       off += tsod_align_up((size_t)capacity * 4, 256);
    w.masks = reinterpret_cast<unsigned *>(p + off);                 off += tsod_align_up((size_t)capacity * 4 * mask_planes, 256);
    w.seg_begin = reinterpret_cast<int *>(p + off);                  off += tsod_align_up((size_t)C * 4, 256);
    w.seg_end = reinterpret_cast<int *>(p + off);                    off += tsod_align_up((size_t)C * 4, 256);
    w.sort_ws = p + off;
    w.sort_bytes = sort_ws_layout(nullptr, capacity).bytes;
    off += w.sort_bytes;
    w.bytes = off;
    return w;
}

// dynamic LDS of the match: keys, per GT box / class / matched (+ gflag) / four waves' list and IoUs, comp
size_t match_lds_bytes(int NP, int G, bool coco = false) {
    return (size_t)NP * 8 + (size_t)G * (16 + 4 + 4 + 4 * 8 + (coco ? 4 : 0)) + (size_t)NP * 2;
}

// staging slots of B * R records, the per-image record counts, the per-image offsets
template <typename Rec>
size_t match_ws_bytes(int B, int R) {
    return tsod_align_up((size_t)B * R * sizeof(Rec), 256) + tsod_align_up((size_t)B * 4, 256) + tsod_align_up((size_t)B * 8, 256);
}

// match -> offsets -> compact, after the entry point's checks
template <typename Rec>
int launch_match(const float *det, int B, int R, const int *counts, const int *keep, const int *n_kept, const float *gt_boxes,
                 const int64_t *gt_labels, const int *gt_counts, int G, const float *iou_thr, int T, AreaRanges ranges,
                 int num_classes, int max_dets, int ignore_class, Rec *records, int64_t capacity, int64_t *n_records,
                 int64_t *npig, void *workspace, tsod_stream_t stream) {
    char *p = static_cast<char *>(workspace);
    const size_t stage_bytes = tsod_align_up((size_t)B * R * sizeof(Rec), 256);
    Rec *stage = reinterpret_cast<Rec *>(p);
    int *stage_counts = reinterpret_cast<int *>(p + stage_bytes);
    long long *offsets = reinterpret_cast<long long *>(p + stage_bytes + tsod_align_up((size_t)B * 4, 256));
    int NP = 64;
    while (NP < R) NP <<= 1;
    const size_t lds = match_lds_bytes(NP, G, is_coco<Rec>);
    hipStream_t st = tsod_stream(stream);
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(eval_match_kernel<Rec>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return TSOD_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(eval_match_kernel<Rec>, dim3(B), dim3(kThreads), lds, st, det, R, counts, keep, n_kept, gt_boxes,
                       reinterpret_cast<const long long *>(gt_labels), gt_counts, G, iou_thr, T, ranges, num_classes, max_dets,
                       ignore_class, NP, stage, stage_counts, reinterpret_cast<unsigned long long *>(npig));
    hipLaunchKernelGGL(eval_offsets_kernel, dim3(1), dim3(kThreads), 0, st, stage_counts, B, offsets,
                       reinterpret_cast<long long *>(n_records));
    hipLaunchKernelGGL(eval_compact_kernel<Rec>, dim3((unsigned)tsod_cdiv(R, kThreads), B), dim3(kThreads), 0, st, stage,
                       stage_counts, offsets, R, records, (long long)capacity);
    return tsod_launch_status();
}

// keys -> sort -> segments -> AP over [num_classes][A][M][T] cells (the plain metric: A = M = 1, caps unused)
template <typename Rec>
int launch_accumulate(const Rec *records, int64_t capacity, const int64_t *n_records, const int64_t *npig, int num_classes, int A,
                      int M, int T, DetCaps caps, double *ap, int64_t *tp, int64_t *fp, int64_t *fn, double *recall,
                      void *workspace, tsod_stream_t stream) {
    const AccWs w = acc_ws_layout(workspace, capacity, num_classes, kSortedPlanes<Rec>);
    hipStream_t st = tsod_stream(stream);
    const long long *nd = reinterpret_cast<const long long *>(n_records);
    const unsigned grid = (unsigned)tsod_cdiv(capacity, kThreads);
    if (hipMemsetAsync(w.seg_begin, 0, (size_t)num_classes * 4, st) != hipSuccess ||
        hipMemsetAsync(w.seg_end, 0, (size_t)num_classes * 4, st) != hipSuccess)
        return TSOD_ERR_LAUNCH;
    hipLaunchKernelGGL(eval_keys_kernel<Rec>, dim3(grid), dim3(kThreads), 0, st, records, (long long)capacity, nd, w.keys);
    const int rc = launch_sort(w.keys, nullptr, capacity, nd, 0, 32 + class_bits(num_classes), w.sorted_keys, w.perm,
                               sort_ws_layout(w.sort_ws, capacity), st);
    if (rc != TSOD_OK) return rc;
    hipLaunchKernelGGL(eval_segments_kernel<Rec>, dim3(grid), dim3(kThreads), 0, st, w.sorted_keys, w.perm, records,
                       (long long)capacity, nd, w.seg_begin, w.seg_end, w.masks);
    hipLaunchKernelGGL(eval_ap_kernel<Rec>, dim3((unsigned)num_classes * (unsigned)(A * M * T)), dim3(kThreads), 0, st, w.masks,
                       (long long)capacity, w.seg_begin, w.seg_end, reinterpret_cast<const long long *>(npig), A, M, T, caps, ap,
                       reinterpret_cast<long long *>(tp), reinterpret_cast<long long *>(fp), reinterpret_cast<long long *>(fn),
                       recall);
    return tsod_launch_status();
}

}  // namespace

extern "C" size_t tsod_eval_match_workspace_bytes(int32_t B, int32_t R) {
    if (B <= 0 || R <= 0) return 0;
    return match_ws_bytes<tsod_eval_record>(B, R);
}

extern "C" int tsod_eval_match_f32(const float *det, int32_t B, int32_t R, const int32_t *counts, const int32_t *keep,
                                   const int32_t *n_kept, const float *gt_boxes, const int64_t *gt_labels,
                                   const int32_t *gt_counts, int32_t G, const float *iou_thr, int32_t T, int32_t num_classes,
                                   int32_t max_dets, int32_t ignore_class, tsod_eval_record *records, int64_t capacity,
                                   int64_t *n_records, int64_t *npig, void *workspace, size_t workspace_bytes,
                                   tsod_stream_t stream) {
    TSOD_REQUIRE(det && iou_thr && records && n_records && npig, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((keep != nullptr) == (n_kept != nullptr) && (counts != nullptr) != (keep != nullptr), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && R > 0 && G >= 0 && T > 0 && num_classes > 0 && max_dets > 0 && capacity >= 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(G == 0 || (gt_boxes && gt_labels && gt_counts), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(R <= kMaxR && G <= kMaxG && T <= kMaxT && num_classes <= kMaxClasses && B <= 65535, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(G == 0 || tsod_aligned16(gt_boxes), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace != nullptr && workspace_bytes >= tsod_eval_match_workspace_bytes(B, R), TSOD_ERR_WORKSPACE);
    return launch_match<tsod_eval_record>(det, B, R, counts, keep, n_kept, gt_boxes, gt_labels, gt_counts, G, iou_thr, T,
                                          AreaRanges{}, num_classes, max_dets, ignore_class, records, capacity, n_records, npig,
                                          workspace, stream);
}

extern "C" size_t tsod_sort_pairs_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return sort_ws_layout(nullptr, n).bytes;
}

extern "C" int tsod_sort_pairs_u64(const uint64_t *keys_in, const int32_t *vals_in, int64_t n, const int64_t *n_dev,
                                   int32_t begin_bit, int32_t end_bit, uint64_t *keys_out, int32_t *vals_out, void *workspace,
                                   size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(keys_in && keys_out && vals_out, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n > 0 && (const void *)keys_in != (const void *)keys_out && (const void *)vals_in != (const void *)vals_out,
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(0 <= begin_bit && begin_bit < end_bit && end_bit <= 64, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n <= (int64_t)INT32_MAX - kRadixTile, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(workspace != nullptr && workspace_bytes >= tsod_sort_pairs_workspace_bytes(n), TSOD_ERR_WORKSPACE);
    const SortWs w = sort_ws_layout(workspace, n);
    return launch_sort(reinterpret_cast<const unsigned long long *>(keys_in), vals_in, n,
                       reinterpret_cast<const long long *>(n_dev), begin_bit, end_bit,
                       reinterpret_cast<unsigned long long *>(keys_out), vals_out, w, tsod_stream(stream));
}

extern "C" size_t tsod_eval_accumulate_workspace_bytes(int64_t capacity, int32_t num_classes) {
    if (capacity <= 0 || num_classes <= 0) return 0;
    return acc_ws_layout(nullptr, capacity, num_classes, kSortedPlanes<tsod_eval_record>).bytes;
}

extern "C" int tsod_eval_accumulate_f64(const tsod_eval_record *records, int64_t capacity, const int64_t *n_records,
                                        const int64_t *npig, int32_t num_classes, int32_t T, double *ap, int64_t *tp,
                                        int64_t *fp, int64_t *fn, double *recall, void *workspace, size_t workspace_bytes,
                                        tsod_stream_t stream) {
    TSOD_REQUIRE(records && n_records && npig && ap && tp && fp && fn && recall, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(capacity > 0 && num_classes > 0 && T > 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(T <= kMaxT && num_classes <= kMaxClasses && capacity <= (int64_t)INT32_MAX - kRadixTile, TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(workspace != nullptr && workspace_bytes >= tsod_eval_accumulate_workspace_bytes(capacity, num_classes),
                 TSOD_ERR_WORKSPACE);
    return launch_accumulate<tsod_eval_record>(records, capacity, n_records, npig, num_classes, 1, 1, T, DetCaps{}, ap, tp, fp, fn,
                                               recall, workspace, stream);
}

extern "C" size_t tsod_eval_match_coco_workspace_bytes(int32_t B, int32_t R) {
    if (B <= 0 || R <= 0 || R > kMaxR || B > 65535) return 0;
    return match_ws_bytes<tsod_eval_record_coco>(B, R);
}

extern "C" int tsod_eval_match_coco_f32(const float *det, int32_t B, int32_t R, const int32_t *counts, const int32_t *keep,
                                        const int32_t *n_kept, const float *gt_boxes, const int64_t *gt_labels,
                                        const int32_t *gt_counts, const uint8_t *gt_crowd, const float *gt_area, int32_t G,
                                        const float *iou_thr, int32_t T, const float *area_lo, const float *area_hi, int32_t A,
                                        int32_t num_classes, int32_t max_dets, int32_t ignore_class,
                                        tsod_eval_record_coco *records, int64_t capacity, int64_t *n_records, int64_t *npig,
                                        void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(det && iou_thr && area_lo && area_hi && records && n_records && npig, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((keep != nullptr) == (n_kept != nullptr) && (counts != nullptr) != (keep != nullptr), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && R > 0 && G >= 0 && T > 0 && A > 0 && num_classes > 0 && max_dets > 0 && capacity >= 0,
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(G == 0 || (gt_boxes && gt_labels && gt_counts), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(R <= kMaxR && G <= kMaxG && T <= kMaxT && A <= kMaxA && num_classes <= kMaxClasses && B <= 65535,
                 TSOD_ERR_UNSUPPORTED);
    TSOD_REQUIRE(G == 0 || tsod_aligned16(gt_boxes), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace != nullptr && workspace_bytes >= tsod_eval_match_coco_workspace_bytes(B, R), TSOD_ERR_WORKSPACE);
    return launch_match<tsod_eval_record_coco>(det, B, R, counts, keep, n_kept, gt_boxes, gt_labels, gt_counts, G, iou_thr, T,
                                               AreaRanges{gt_crowd, gt_area, area_lo, area_hi, A}, num_classes, max_dets,
                                               ignore_class, records, capacity, n_records, npig, workspace, stream);
}

extern "C" size_t tsod_eval_accumulate_coco_workspace_bytes(int64_t capacity, int32_t num_classes) {
    if (capacity <= 0 || num_classes <= 0 || num_classes > kMaxClasses || capacity > (int64_t)INT32_MAX - kRadixTile) return 0;
    return acc_ws_layout(nullptr, capacity, num_classes, kSortedPlanes<tsod_eval_record_coco>).bytes;
}

extern "C" int tsod_eval_accumulate_coco_f64(const tsod_eval_record_coco *records, int64_t capacity, const int64_t *n_records,
                                             const int64_t *npig, int32_t num_classes, int32_t A, int32_t T,
                                             const int32_t *max_dets_list, int32_t M, int32_t max_dets, double *ap, int64_t *tp,
                                             int64_t *fp, int64_t *fn, double *recall, void *workspace, size_t workspace_bytes,
                                             tsod_stream_t stream) {
    TSOD_REQUIRE(records && n_records && npig && max_dets_list && ap && tp && fp && fn && recall, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(capacity > 0 && num_classes > 0 && T > 0 && A > 0 && M > 0 && max_dets > 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(T <= kMaxT && A <= kMaxA && M <= kMaxM && num_classes <= kMaxClasses &&
                     capacity <= (int64_t)INT32_MAX - kRadixTile,
                 TSOD_ERR_UNSUPPORTED);
    DetCaps caps = {{0, 0, 0, 0}};
    for (int m = 0; m < M; ++m) {
        TSOD_REQUIRE(max_dets_list[m] > (m ? max_dets_list[m - 1] : 0), TSOD_ERR_INVALID_ARG);   // ascending, from 1
        caps.v[m] = max_dets_list[m];
    }
    TSOD_REQUIRE(caps.v[M - 1] <= max_dets, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(workspace != nullptr && workspace_bytes >= tsod_eval_accumulate_coco_workspace_bytes(capacity, num_classes),
                 TSOD_ERR_WORKSPACE);
    return launch_accumulate<tsod_eval_record_coco>(records, capacity, n_records, npig, num_classes, A, M, T, caps, ap, tp, fp, fn,
                                                    recall, workspace, stream);
}
