// feature_grads.hip -- the backward of the RoI head's pooling into the feature map: d loss / d base_feature's RoI term.
//
//   tsod_roi_pool_avg_grad_f32    backward of tsod_roi_pool_avg_f32 (RoI rescale + index + RoIPool + mean over PH x PW):
//                                 torchvision's published roi_pool backward - each bin's d_out / (PH PW) goes to the bin's
//                                 arg-max pixel, empty bins give nothing
//   tsod_roi_align_avg_grad_f32   backward of tsod_roi_align_avg_f32: torchvision's roi_align backward - sample (iy, ix) of a
//                                 bin gives w1..w4 x d_out / (PH PW count) to its four corners, skipped samples give nothing
//
// The geometry (tsod_roi_to_map, tsod_roi_pool_geom, tsod_bin_range, tsod_roi_align_geom, TSOD_ALIGN_SAMPLE and
// TSOD_ALIGN_BILINEAR_OR_CONTINUE) is tsod_internal.h's, the forward kernels' own, so forward and backward agree on every
// pixel a bin reads.
//
// Determinism: no atomics.  The output is a GATHER: one thread owns (pixel, channel quad) of d_feat, walks the RoI groups whose
// roi_indices name its image in group order, the RoIs of a group in ascending order, and within a RoI the bins (and for
// RoIAlign the samples and corners) in the forward's order; it adds what reaches its pixel and writes the element once
// (``accumulate``: added to what is there, e.g. the RPN's input gradient).  Bit-identical from run to run.
//
// RoIPool's arg-max is recomputed from the saved feature bits by a pre-pass with the forward's exact rule (torchvision
// roi_pool_kernel.cpp: start from -FLT_MAX, strict '>', h outer, w inner, so the first maximum wins; a bin whose values never
// exceed -FLT_MAX - NaN, -inf - has none).  It records the winner as the pixel's index h * Wf + w in the map: u16, since a bin
// never leaves the map, Hf * Wf <= 65535 bounds every bin; 0xFFFF = no arg-max.  Bins sharing rows or columns (floor / ceil
// edges, RoIs smaller than PH x PW pixels) each keep their own record, so a pixel collects every bin it wins.
#include "tsod_internal.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int kQuadsPerWave = 64;      // a wave: 64 channel quads (256 channels) of a pixel strip
constexpr int kStrip = 4;              // ... of kStrip neighbouring pixels of one row (the RoI checks are shared by the strip)
constexpr int kWaves = 4;
constexpr unsigned kNoArgmax = 0xFFFFu;

__device__ __forceinline__ void add4(float4 &a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

// ------------------------------------------------------------------------------------------------------------ RoIPool
// per RoI k: ext[k] = (y0, y1, x0, x1), every bin's rows in [y0, y1) and columns in [x0, x1) (bin edges are monotone in the bin
// index); rec [B*R][PH*PW][C] u16 = the arg-max pixel of (bin, channel).  grid (channel groups, B*R): lanes over channel quads,
// wave w runs bins w, w + 4, ...
__global__ void __launch_bounds__(256)
roi_pool_argmax_kernel(const float *__restrict__ feat, int B, int Hf, int Wf, int C, int pitch, const float *__restrict__ rois,
                       const int *__restrict__ roi_indices, int R, float img_h, float img_w, float scale, int PH, int PW,
                       int4 *__restrict__ ext, uint16_t *__restrict__ rec) {
    const int k = blockIdx.y;
    const float4 fm = tsod_roi_to_map(reinterpret_cast<const float4 *>(rois)[k], img_h, img_w, Hf, Wf);
    const tsod_pool_geom g = tsod_roi_pool_geom((float)roi_indices[k / R], fm.x, fm.y, fm.z, fm.w, scale);
    const bool valid = g.b >= 0 && g.b < B;
    const float bin_h = (float)g.rh / (float)PH;
    const float bin_w = (float)g.rw / (float)PW;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int4 e = make_int4(0, 0, 0, 0);                                        // (an invalid RoI covers nothing)
        if (valid) {
            int lo, hi;
            tsod_bin_range(0, bin_h, g.sh, Hf, e.x, hi);
            tsod_bin_range(PH - 1, bin_h, g.sh, Hf, lo, e.y);
            tsod_bin_range(0, bin_w, g.sw, Wf, e.z, hi);
            tsod_bin_range(PW - 1, bin_w, g.sw, Wf, lo, e.w);
        }
        ext[k] = e;
    }
    const int c4 = blockIdx.x * kQuadsPerWave + (threadIdx.x & 63);
    if (!valid || c4 >= (C >> 2)) return;
    const float *fmap = feat + (long)g.b * Hf * Wf * pitch + 4 * c4;
    const int bins = PH * PW;
    for (int bin = threadIdx.x >> 6; bin < bins; bin += kWaves) {
        const int ph = bin / PW, pw = bin - ph * PW;
        int hs, he, ws, we;
        tsod_bin_range(ph, bin_h, g.sh, Hf, hs, he);
        tsod_bin_range(pw, bin_w, g.sw, Wf, ws, we);
        float4 m = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX);
        unsigned ix = kNoArgmax, iy = kNoArgmax, iz = kNoArgmax, iw = kNoArgmax;
        for (int h = hs; h < he; ++h)
            for (int w = ws; w < we; ++w) {
                const float4 v = *reinterpret_cast<const float4 *>(fmap + ((long)h * Wf + w) * pitch);
                const unsigned idx = (unsigned)(h * Wf + w);
                if (v.x > m.x) { m.x = v.x; ix = idx; }
                if (v.y > m.y) { m.y = v.y; iy = idx; }
                if (v.z > m.z) { m.z = v.z; iz = idx; }
                if (v.w > m.w) { m.w = v.w; iw = idx; }
            }
        *reinterpret_cast<uint2 *>(rec + ((long)k * bins + bin) * C + 4 * c4) = make_uint2(ix | (iy << 16), iz | (iw << 16));
    }
}

// d_feat of a pixel strip: grid (ceil(strips / 4), channel groups), one wave per (strip, 64 channel quads)
__global__ void __launch_bounds__(256)
roi_pool_gather_kernel(int B, int Hf, int Wf, int C, const float *__restrict__ rois, const int *__restrict__ roi_indices, int R,
                       float img_h, float img_w, float scale, int PH, int PW, const float *__restrict__ d_out, int d_out_pitch,
                       const int4 *__restrict__ ext, const uint16_t *__restrict__ rec, float *__restrict__ d_feat, int d_pitch,
                       int accumulate) {
    const int per_row = (Wf + kStrip - 1) / kStrip;
    const long strip = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (strip >= (long)B * Hf * per_row) return;                              // (wave-uniform; no barrier below)
    const int b = (int)(strip / ((long)Hf * per_row));
    const int rem = (int)(strip - (long)b * Hf * per_row);
    const int py = rem / per_row, px0 = (rem - py * per_row) * kStrip;
    const int c4 = blockIdx.y * kQuadsPerWave + (threadIdx.x & 63);
    const bool live = c4 < (C >> 2);
    const int bins = PH * PW;
    const float nb = (float)bins;
    float4 acc[kStrip];
#pragma unroll
    for (int p = 0; p < kStrip; ++p) acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int grp = 0; grp < B; ++grp) {
        if (roi_indices[grp] != b) continue;
        for (int k = grp * R; k < (grp + 1) * R; ++k) {
            const int4 e = ext[k];
            if (py < e.x || py >= e.y || px0 + kStrip <= e.z || px0 >= e.w) continue;
            const float4 fm = tsod_roi_to_map(reinterpret_cast<const float4 *>(rois)[k], img_h, img_w, Hf, Wf);
            const tsod_pool_geom g = tsod_roi_pool_geom((float)b, fm.x, fm.y, fm.z, fm.w, scale);
            const float bin_h = (float)g.rh / (float)PH;
            const float bin_w = (float)g.rw / (float)PW;
            float4 gd = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                const float4 d = *reinterpret_cast<const float4 *>(d_out + (long)k * d_out_pitch + 4 * c4);
                gd = make_float4(d.x / nb, d.y / nb, d.z / nb, d.w / nb);      // the mean's backward
            }
            for (int ph = 0; ph < PH; ++ph) {
                int hs, he;
                tsod_bin_range(ph, bin_h, g.sh, Hf, hs, he);
                if (py < hs || py >= he) continue;
                for (int pw = 0; pw < PW; ++pw) {
                    int ws, we;
                    tsod_bin_range(pw, bin_w, g.sw, Wf, ws, we);
                    if (we <= px0 || ws >= px0 + kStrip || !live) continue;
                    const uint2 r = *reinterpret_cast<const uint2 *>(rec + ((long)k * bins + ph * PW + pw) * C + 4 * c4);
                    const unsigned rx = r.x & 0xFFFFu, ry = r.x >> 16, rz = r.y & 0xFFFFu, rw = r.y >> 16;
#pragma unroll
                    for (int p = 0; p < kStrip; ++p) {
                        const int px = px0 + p;
                        if (px < ws || px >= we) continue;
                        const unsigned idx = (unsigned)(py * Wf + px);
                        if (rx == idx) acc[p].x += gd.x;
                        if (ry == idx) acc[p].y += gd.y;
                        if (rz == idx) acc[p].z += gd.z;
                        if (rw == idx) acc[p].w += gd.w;
                    }
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int p = 0; p < kStrip; ++p) {
        const int px = px0 + p;
        if (px >= Wf) break;
        float4 *dst = reinterpret_cast<float4 *>(d_feat + (((long)b * Hf + py) * Wf + px) * d_pitch + 4 * c4);
        float4 v = acc[p];
        if (accumulate) {
            v = *dst;
            add4(v, acc[p]);
        }
        *dst = v;
    }
}

// ----------------------------------------------------------------------------------------------------------- RoIAlign
// per RoI k: ext[k] = a superset (y0, y1, x0, x1) of the pixels its samples touch: samples lie between start and
// start + P bin (bin < 0 is possible with aligned = 1) up to rounding, and touch floor(max(coordinate, 0)) and the pixel after
// it - one pixel of margin on both sides.
__device__ __forceinline__ void align_span(float start, float bin, int P, int n, int &lo, int &hi) {
    const float end = start + (float)P * bin;
    const float a = fminf(fmaxf(fminf(start, end), -4.f), (float)n + 4.f);
    const float z = fminf(fmaxf(fmaxf(start, end), -4.f), (float)n + 4.f);
    lo = max((int)floorf(a) - 1, 0);
    hi = min((int)floorf(z) + 3, n);
}

__global__ void __launch_bounds__(256)
roi_align_extent_kernel(int B, int Hf, int Wf, const float *__restrict__ rois, const int *__restrict__ roi_indices, int R, int K,
                        float img_h, float img_w, float scale, int PH, int PW, int sampling_ratio, int aligned,
                        int4 *__restrict__ ext) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const float4 fm = tsod_roi_to_map(reinterpret_cast<const float4 *>(rois)[k], img_h, img_w, Hf, Wf);
    const tsod_align_geom g = tsod_roi_align_geom((float)roi_indices[k / R], fm.x, fm.y, fm.z, fm.w, scale, PH, PW,
                                                  sampling_ratio, aligned);
    int4 e = make_int4(0, 0, 0, 0);
    if (g.b >= 0 && g.b < B) {
        align_span(g.start_h, g.bin_h, PH, Hf, e.x, e.y);
        align_span(g.start_w, g.bin_w, PW, Wf, e.z, e.w);
    }
    ext[k] = e;
}

__global__ void __launch_bounds__(256)
roi_align_gather_kernel(int B, int Hf, int Wf, int C, const float *__restrict__ rois, const int *__restrict__ roi_indices, int R,
                        float img_h, float img_w, float scale, int PH, int PW, int sampling_ratio, int aligned,
                        const float *__restrict__ d_out, int d_out_pitch, const int4 *__restrict__ ext,
                        float *__restrict__ d_feat, int d_pitch, int accumulate) {
    const int per_row = (Wf + kStrip - 1) / kStrip;
    const long strip = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (strip >= (long)B * Hf * per_row) return;
    const int b = (int)(strip / ((long)Hf * per_row));
    const int rem = (int)(strip - (long)b * Hf * per_row);
    const int py = rem / per_row, px0 = (rem - py * per_row) * kStrip;
    const int c4 = blockIdx.y * kQuadsPerWave + (threadIdx.x & 63);
    const bool live = c4 < (C >> 2);
    const float nb = (float)(PH * PW);
    float4 acc[kStrip];
#pragma unroll
    for (int p = 0; p < kStrip; ++p) acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int grp = 0; grp < B; ++grp) {
        if (roi_indices[grp] != b) continue;
        for (int k = grp * R; k < (grp + 1) * R; ++k) {
            const int4 e = ext[k];
            if (py < e.x || py >= e.y || px0 + kStrip <= e.z || px0 >= e.w || !live) continue;
            const float4 fm = tsod_roi_to_map(reinterpret_cast<const float4 *>(rois)[k], img_h, img_w, Hf, Wf);
            const tsod_align_geom g = tsod_roi_align_geom((float)b, fm.x, fm.y, fm.z, fm.w, scale, PH, PW, sampling_ratio, aligned);
            const float4 d = *reinterpret_cast<const float4 *>(d_out + (long)k * d_out_pitch + 4 * c4);
            const float4 gb = make_float4(d.x / nb, d.y / nb, d.z / nb, d.w / nb);       // the mean's backward
            for (int ph = 0; ph < PH; ++ph) {
                int r0, r1;                                                       // (the extent rule for one bin row)
                align_span(g.start_h + (float)ph * g.bin_h, g.bin_h, 1, Hf, r0, r1);
                if (py < r0 || py >= r1) continue;
                for (int pw = 0; pw < PW; ++pw) {
                    int q0, q1;
                    align_span(g.start_w + (float)pw * g.bin_w, g.bin_w, 1, Wf, q0, q1);
                    if (px0 + kStrip <= q0 || px0 >= q1) continue;
                    for (int iy = 0; iy < g.grid_h; ++iy) {
                        const float yy = TSOD_ALIGN_SAMPLE(g.start_h, g.bin_h, g.grid_h, ph, iy);
                        for (int ix = 0; ix < g.grid_w; ++ix) {
                            const float xx = TSOD_ALIGN_SAMPLE(g.start_w, g.bin_w, g.grid_w, pw, ix);
                            TSOD_ALIGN_BILINEAR_OR_CONTINUE(yy, xx, Hf, Wf);
                            if (y_low != py && y_high != py) continue;
                            const float hy = 1.f - ly, hx = 1.f - lx;
                            const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
#pragma unroll
                            for (int p = 0; p < kStrip; ++p) {
                                const int px = px0 + p;
                                // corners in torchvision's order: (low, low), (low, high), (high, low), (high, high)
                                const float cw[4] = {w1, w2, w3, w4};
                                const bool hit[4] = {y_low == py && x_low == px, y_low == py && x_high == px,
                                                     y_high == py && x_low == px, y_high == py && x_high == px};
#pragma unroll
                                for (int c = 0; c < 4; ++c)
                                    if (hit[c]) {
                                        acc[p].x += gb.x * cw[c] / g.count;
                                        acc[p].y += gb.y * cw[c] / g.count;
                                        acc[p].z += gb.z * cw[c] / g.count;
                                        acc[p].w += gb.w * cw[c] / g.count;
                                    }
                            }
                        }
                    }
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int p = 0; p < kStrip; ++p) {
        const int px = px0 + p;
        if (px >= Wf) break;
        float4 *dst = reinterpret_cast<float4 *>(d_feat + (((long)b * Hf + py) * Wf + px) * d_pitch + 4 * c4);
        float4 v = acc[p];
        if (accumulate) {
            v = *dst;
            add4(v, acc[p]);
        }
        *dst = v;
    }
}


dim3 gather_grid(int B, int Hf, int Wf, int C) {
    const long strips = (long)B * Hf * ((Wf + kStrip - 1) / kStrip);
    return dim3((unsigned)tsod_cdiv(strips, kWaves), (unsigned)tsod_cdiv(C / 4, kQuadsPerWave));
}

}  // namespace

extern "C" size_t tsod_roi_pool_avg_grad_workspace_bytes(int32_t B, int32_t R, int32_t C, int32_t PH, int32_t PW) {
    if (B <= 0 || R <= 0 || C <= 0 || PH <= 0 || PW <= 0) return 0;
    const size_t K = (size_t)B * R;
    return tsod_align_up(K * sizeof(int4), 16) + K * (size_t)PH * PW * C * sizeof(uint16_t);
}

extern "C" int tsod_roi_pool_avg_grad_f32(const float *feat, int32_t B, int32_t Hf, int32_t Wf, int32_t C, int32_t feat_pitch,
                                          const float *rois, const int32_t *roi_indices, int32_t R, float img_h, float img_w,
                                          float spatial_scale, int32_t PH, int32_t PW, const float *d_out, int32_t d_out_pitch,
                                          float *d_feat, int32_t d_feat_pitch, int32_t accumulate, void *workspace,
                                          size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(feat && rois && roi_indices && d_out && d_feat, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && Hf > 0 && Wf > 0 && C > 0 && R > 0 && PH > 0 && PW > 0 && (long)B * R <= 65535, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((long)Hf * Wf <= 65535, TSOD_ERR_UNSUPPORTED);                 // the u16 arg-max record (0xFFFF: none)
    TSOD_REQUIRE(img_h > 0.f && img_w > 0.f, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((C & 3) == 0 && (feat_pitch & 3) == 0 && feat_pitch >= C && (d_out_pitch & 3) == 0 && d_out_pitch >= C &&
                 (d_feat_pitch & 3) == 0 && d_feat_pitch >= C, TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(feat) && tsod_aligned16(rois) && tsod_aligned16(d_out) && tsod_aligned16(d_feat), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) &&
                 workspace_bytes >= tsod_roi_pool_avg_grad_workspace_bytes(B, R, C, PH, PW), TSOD_ERR_WORKSPACE);
    hipStream_t s = tsod_stream(stream);
    int4 *ext = static_cast<int4 *>(workspace);
    uint16_t *rec = reinterpret_cast<uint16_t *>(static_cast<char *>(workspace) + tsod_align_up((size_t)B * R * sizeof(int4), 16));
    hipLaunchKernelGGL(roi_pool_argmax_kernel, dim3((unsigned)tsod_cdiv(C / 4, kQuadsPerWave), B * R), dim3(256), 0, s, feat, B,
                       Hf, Wf, C, feat_pitch, rois, roi_indices, R, img_h, img_w, spatial_scale, PH, PW, ext, rec);
    hipLaunchKernelGGL(roi_pool_gather_kernel, gather_grid(B, Hf, Wf, C), dim3(256), 0, s, B, Hf, Wf, C, rois, roi_indices, R,
                       img_h, img_w, spatial_scale, PH, PW, d_out, d_out_pitch, (const int4 *)ext, (const uint16_t *)rec, d_feat,
                       d_feat_pitch, accumulate ? 1 : 0);
    return tsod_launch_status();
}

extern "C" size_t tsod_roi_align_avg_grad_workspace_bytes(int32_t B, int32_t R) {
    if (B <= 0 || R <= 0) return 0;
    return (size_t)B * R * sizeof(int4);
}

extern "C" int tsod_roi_align_avg_grad_f32(int32_t B, int32_t Hf, int32_t Wf, int32_t C, const float *rois,
                                           const int32_t *roi_indices, int32_t R, float img_h, float img_w, float spatial_scale,
                                           int32_t PH, int32_t PW, int32_t sampling_ratio, int32_t aligned, const float *d_out,
                                           int32_t d_out_pitch, float *d_feat, int32_t d_feat_pitch, int32_t accumulate,
                                           void *workspace, size_t workspace_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(rois && roi_indices && d_out && d_feat, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(B > 0 && Hf > 0 && Wf > 0 && C > 0 && R > 0 && PH > 0 && PW > 0 && sampling_ratio >= 0, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(img_h > 0.f && img_w > 0.f, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE((C & 3) == 0 && (d_out_pitch & 3) == 0 && d_out_pitch >= C && (d_feat_pitch & 3) == 0 && d_feat_pitch >= C,
                 TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(tsod_aligned16(rois) && tsod_aligned16(d_out) && tsod_aligned16(d_feat), TSOD_ERR_ALIGNMENT);
    TSOD_REQUIRE(workspace && tsod_aligned16(workspace) && workspace_bytes >= tsod_roi_align_avg_grad_workspace_bytes(B, R),
                 TSOD_ERR_WORKSPACE);
    hipStream_t s = tsod_stream(stream);
    int4 *ext = static_cast<int4 *>(workspace);
    const int K = B * R;
    hipLaunchKernelGGL(roi_align_extent_kernel, dim3((unsigned)tsod_cdiv(K, 256)), dim3(256), 0, s, B, Hf, Wf, rois, roi_indices, R,
                       K, img_h, img_w, spatial_scale, PH, PW, sampling_ratio, aligned ? 1 : 0, ext);
    hipLaunchKernelGGL(roi_align_gather_kernel, gather_grid(B, Hf, Wf, C), dim3(256), 0, s, B, Hf, Wf, C, rois, roi_indices, R,
                       img_h, img_w, spatial_scale, PH, PW, sampling_ratio, aligned ? 1 : 0, d_out, d_out_pitch,
                       (const int4 *)ext, d_feat, d_feat_pitch, accumulate ? 1 : 0);
    return tsod_launch_status();
}
