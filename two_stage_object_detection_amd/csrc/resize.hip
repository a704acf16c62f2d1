// resize.hip -- the input step in front of the path: antialiased bilinear resize of a decoded u8 HWC image to the
// detector's fixed input size, fused with the u8 -> f32 conversion and the NHWC(4-channel) / NCHW layout the
// backbone reads, and the same resize of an f32 image (the training transform's second one).  HBM / LDS-bound gather
// + a handful of multiply-adds per output value; no MFMA.
//
//   dataset/dataloader.py:35-44   PIL RGB -> tv_tensors.Image(img, dtype=float32)  (f32 CHW, values 0..255, quirk: never /255)
//   dataset/transform.py:14-17    eval_transform = Resize((600, 600)) + ToTensor (a pass-through for tensors)
//   torchvision v2 Resize on a float tensor = torch.nn.functional.interpolate(mode="bilinear", antialias=True,
//   align_corners=False): separable triangle filter whose support grows with the down-scale factor
//   (ATen UpSampleKernel.cpp, HelperInterpLinear::aa_filter + _compute_indices_min_size_weights_aa); restated here:
//   the tap tables on the host in f32 with ATen's own expression order, the two passes (horizontal, then vertical) in
//   one kernel with the horizontal sums kept in f32 like ATen's intermediate image.  Compiled with -ffp-contract=off.
//
// The tap loop, the store, the tile and the two kernel templates are resize_aa.h's; this file holds the tap tables and
// the two plain source policies (augment.hip holds the third).
#include "resize_aa.h"

namespace {

// u8 [H, W, C] with a row pitch.  The region is staged as raw bytes with coalesced aligned dword loads: row r of the
// region starts at global byte address a_r = src + (ry0 + r) * pitch + rx0 * C; LDS holds the aligned dwords from
// a_r - (a_r & 3) on, so a consumer adds that misalignment back.
struct U8Bytes {
    const unsigned char *src;
    int C;
    long pitch;
    static constexpr size_t kLdsCap = 48 * 1024;
    static constexpr int kPrologueDoubles = 0;
    __host__ __device__ static int row_bytes(int C, int cap_cols) { return ((cap_cols * C + 3 + 3) / 4) * 4; }
    __host__ __device__ static size_t region_bytes(int C, int cap_rows, int cap_cols) {
        return (size_t)cap_rows * row_bytes(C, cap_cols);
    }
    __device__ void prologue(double *) {}
    __device__ unsigned long long row_addr(int y, int rx0) const {
        return reinterpret_cast<unsigned long long>(src) + (unsigned long long)rx0 * C + (unsigned long long)y * pitch;
    }
    __device__ void stage(unsigned char *lds, const TileGeom &g, int cap_rows, int cap_cols) const {
        const int cap_row_bytes = row_bytes(C, cap_cols), words_cap = cap_row_bytes >> 2;
        for (int r = threadIdx.x / kTX; r < g.rows; r += kTY) {      // a row of the region per 32 threads
            const unsigned long long a = row_addr(g.ry0 + r, g.rx0);
            const int mis = (int)(a & 3ull);
            const int words = min((g.cols * C + mis + 3) >> 2, words_cap);
            const unsigned *gw = reinterpret_cast<const unsigned *>(a - mis);
            unsigned *lw = reinterpret_cast<unsigned *>(lds + (long)r * cap_row_bytes);
            for (int w = threadIdx.x % kTX; w < words; w += kTX) lw[w] = gw[w];
        }
    }
    __device__ auto tile_px(const unsigned char *lds, const TileGeom &g, int cap_rows, int cap_cols, int y, int x) const {
        const int mis = (int)(row_addr(y, g.rx0) & 3ull);
        const unsigned char *q = lds + (long)min(y - g.ry0, cap_rows - 1) * row_bytes(C, cap_cols) + mis + (x - g.rx0) * C;
        return [q](int c) { return (float)q[c]; };
    }
    __device__ auto src_px(int y, int x) const {
        const unsigned char *q = src + (long)y * pitch + (long)x * C;
        return [q](int c) { return (float)q[c]; };
    }
};

// f32 [H, W, C] through three strides; the region is staged as C planes.
struct StridedF32 : F32Planes {
    const float *src;
    int H, W, C;
    long sy, sx, sc;
    static constexpr int kPrologueDoubles = 0;
    __device__ void prologue(double *) {}
    __device__ void stage(unsigned char *lds, const TileGeom &g, int cap_rows, int cap_cols) const {
        float *planes = reinterpret_cast<float *>(lds);
        const long plane = (long)cap_rows * cap_cols;
        for (int c = 0; c < C; ++c)
            for (int r = threadIdx.x / kTX; r < g.rows; r += kTY)
                for (int col = threadIdx.x % kTX; col < g.cols; col += kTX) {
                    const int y = g.ry0 + r, x = g.rx0 + col;
                    if (y >= H || x >= W) continue;
                    planes[c * plane + (long)r * cap_cols + col] = src[(long)y * sy + (long)x * sx + (long)c * sc];
                }
    }
    __device__ auto src_px(int y, int x) const {
        const float *q = src + (long)y * sy + (long)x * sx;
        return [q, sc = sc](int c) { return q[(long)c * sc]; };
    }
};

}  // namespace

extern "C" int32_t tsod_resize_aa_taps(int32_t in_size, int32_t out_size) {
    if (in_size <= 0 || out_size <= 0) return 0;
    const float scale = (float)in_size / (float)out_size;
    const float support = scale >= 1.0f ? scale : 1.0f;
    return (int32_t)ceilf(support) * 2 + 1;
}

extern "C" int tsod_resize_aa_tables_f32(int32_t in_size, int32_t out_size, int32_t *first, int32_t *count,
                                         float *weights) {
    TSOD_REQUIRE(first && count && weights && in_size > 0 && out_size > 0, TSOD_ERR_INVALID_ARG);
    const int taps = tsod_resize_aa_taps(in_size, out_size);
    // f32 throughout, in ATen's expression order (area_pixel_compute_scale + _compute_indices_min_size_weights_aa)
    const float scale = (float)in_size / (float)out_size;
    const float support = scale >= 1.0f ? scale : 1.0f;
    const float invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
    for (int i = 0; i < out_size; ++i) {
        const float center = scale * ((float)i + 0.5f);
        // ATen adds the 0.5 as a double to the f32 difference / sum before truncating
        long lo = (long)((double)(center - support) + 0.5);
        if (lo < 0) lo = 0;
        long hi = (long)((double)(center + support) + 0.5);
        if (hi > in_size) hi = in_size;
        long n = hi - lo;
        if (n < 0) n = 0;
        if (n > taps) n = taps;
        float *w = weights + (long)i * taps;
        float total = 0.f;
        for (long j = 0; j < n; ++j) {
            float x = (float)(((double)((float)(j + lo) - center) + 0.5) * (double)invscale);
            if (x < 0.f) x = -x;
            w[j] = x < 1.0f ? 1.0f - x : 0.f;
            total += w[j];
        }
        if (total != 0.f)
            for (long j = 0; j < n; ++j) w[j] /= total;
        for (long j = n; j < taps; ++j) w[j] = 0.f;
        first[i] = (int32_t)lo;
        count[i] = (int32_t)n;
    }
    return TSOD_OK;
}

extern "C" int tsod_resize_bilinear_aa_u8_f32(const uint8_t *src, int32_t H, int32_t W, int32_t C, int64_t src_row_bytes,
                                              const int32_t *yfirst, const int32_t *ycount, const float *ywt,
                                              const int32_t *xfirst, const int32_t *xcount, const float *xwt,
                                              int32_t OH, int32_t OW, float mul, float *out, int64_t stride_y,
                                              int64_t stride_x, int64_t stride_c, int32_t C_out, tsod_stream_t stream) {
    TSOD_REQUIRE(src && yfirst && ycount && ywt && xfirst && xcount && xwt && out, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(H > 0 && W > 0 && OH > 0 && OW > 0 && C >= 1 && C <= 4 && C_out >= C && C_out <= 4, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(src_row_bytes >= (int64_t)W * C, TSOD_ERR_INVALID_ARG);
    const U8Bytes p = {src, C, (long)src_row_bytes};
    return launch_resize(p, H, W, yfirst, ycount, ywt, xfirst, xcount, xwt, OH, OW, mul, out, stride_y, stride_x, stride_c,
                         C_out, stream);
}

extern "C" int tsod_resize_bilinear_aa_f32(const float *src, int32_t H, int32_t W, int32_t C, int64_t src_stride_y,
                                           int64_t src_stride_x, int64_t src_stride_c, const int32_t *yfirst,
                                           const int32_t *ycount, const float *ywt, const int32_t *xfirst,
                                           const int32_t *xcount, const float *xwt, int32_t OH, int32_t OW, float *out,
                                           int64_t stride_y, int64_t stride_x, int64_t stride_c, int32_t C_out,
                                           tsod_stream_t stream) {
    TSOD_REQUIRE(src && yfirst && ycount && ywt && xfirst && xcount && xwt && out, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(H > 0 && W > 0 && OH > 0 && OW > 0 && C >= 1 && C <= 4 && C_out >= C && C_out <= 4, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(src_stride_y >= 0 && src_stride_x >= 0 && src_stride_c >= 0, TSOD_ERR_INVALID_ARG);
    StridedF32 p;
    p.src = src, p.H = H, p.W = W, p.C = C;
    p.sy = (long)src_stride_y, p.sx = (long)src_stride_x, p.sc = (long)src_stride_c;
    return launch_resize(p, H, W, yfirst, ycount, ywt, xfirst, xcount, xwt, OH, OW, 1.0f, out, stride_y, stride_x, stride_c,
                         C_out, stream);
}
