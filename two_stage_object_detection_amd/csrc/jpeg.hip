// jpeg.hip -- JPEG decoding (include/tsod.h "JPEG decoding"): the host Huffman pass of jpeg_entropy.h
// behind two C entry points, and the two kernels that turn a batch's coefficients into packed RGB - dequantisation with the
// 8x8 inverse DCT, then chroma upsampling, colour conversion and the crop.  Every address either kernel forms comes from the
// table and work list that the entry points checked on the host; file-derived data only ever appear as values.
#include "jpeg_checks.h"
#include "jpeg_entropy.h"
#include "tsod_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlockWords = 72;          // LDS words per 8x8 block: 64 + 8, so the 4 blocks of a 32-lane group fill 32 banks
constexpr int kRun = 4;                  // pixels per thread of to_rgb
static_assert(TSOD_JPEG_IDCT_BLOCKS * 8 == kThreads, "8 lanes per block");
static_assert(TSOD_JPEG_RGB_TILE_W * TSOD_JPEG_RGB_TILE_H == kThreads * kRun, "four pixels per thread");
static_assert(TSOD_JPEG_RGB_TILE_W % kRun == 0 && TSOD_JPEG_RGB_TILE_W / kRun == TSOD_WAVE, "one wave per tile row");

__device__ __forceinline__ uint32_t descale(uint32_t x, int n) { return (uint32_t)((int32_t)(x + (1u << (n - 1))) >> n); }

// One 8-point pass of jidctint.c's jpeg_idct_islow in wrapping 32-bit arithmetic; the output is descaled by N bits.
template <int N>
__device__ __forceinline__ void idct_pass(uint32_t (&d)[8]) {
    uint32_t z1 = (d[2] + d[6]) * 4433u;
    uint32_t tmp2 = z1 + d[6] * (uint32_t)-15137;
    uint32_t tmp3 = z1 + d[2] * 6270u;
    uint32_t tmp0 = (d[0] + d[4]) << 13;
    uint32_t tmp1 = (d[0] - d[4]) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7], tmp1 = d[5], tmp2 = d[3], tmp3 = d[1];
    z1 = tmp0 + tmp3;
    uint32_t z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
    z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995, z3 *= (uint32_t)-16069, z4 *= (uint32_t)-3196;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    d[0] = descale(tmp10 + tmp3, N), d[7] = descale(tmp10 - tmp3, N);
    d[1] = descale(tmp11 + tmp2, N), d[6] = descale(tmp11 - tmp2, N);
    d[2] = descale(tmp12 + tmp1, N), d[5] = descale(tmp12 - tmp1, N);
    d[3] = descale(tmp13 + tmp0, N), d[4] = descale(tmp13 - tmp0, N);
}

__device__ __forceinline__ uint32_t range_limit(uint32_t v) {
    const uint32_t j = v & 1023u;
    return j < 128u ? j + 128u : (j < 512u ? 255u : (j < 896u ? 0u : j - 896u));
}

__global__ void __launch_bounds__(kThreads)
jpeg_idct_kernel(const tsod_jpeg_image *__restrict__ table, const int4 *__restrict__ work, const int16_t *__restrict__ coef,
                 const uint16_t *__restrict__ quant, uint8_t *__restrict__ planes) {
    __shared__ uint32_t lds[TSOD_JPEG_IDCT_BLOCKS * kBlockWords];
    const int4 item = work[blockIdx.x];
    const tsod_jpeg_image &im = table[item.x];
    const int comp = item.y;
    const int bw = im.blocks_w[comp], n_blocks = bw * im.blocks_h[comp];
    const int sub = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const int blk = item.z + sub;
    const bool live = blk < n_blocks;
    uint32_t *tile = lds + sub * kBlockWords;
    uint32_t d[8];
    if (live) {                                                  // row `lane` of the block: dequantise, store as a row
        const uint4 c = *reinterpret_cast<const uint4 *>(coef + im.coef_offset[comp] + (long long)blk * 64 + lane * 8);
        const uint4 q = *reinterpret_cast<const uint4 *>(quant + im.quant_offset + comp * 64 + lane * 8);
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[2 * k] = (uint32_t)(int32_t)(int16_t)(cw[k] & 0xffffu) * (qw[k] & 0xffffu);
            d[2 * k + 1] = (uint32_t)((int32_t)cw[k] >> 16) * (qw[k] >> 16);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[lane * 8 + k] = d[k];
    }
    __syncthreads();
    if (live) {                                                  // column `lane`, in place: no other lane touches these words
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = tile[k * 8 + lane];
        idct_pass<11>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[k * 8 + lane] = d[k];
    }
    __syncthreads();
    if (live) {                                                  // row `lane` again
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = tile[lane * 8 + k];
        idct_pass<18>(d);
        uint2 o;
        o.x = range_limit(d[0]) | range_limit(d[1]) << 8 | range_limit(d[2]) << 16 | range_limit(d[3]) << 24;
        o.y = range_limit(d[4]) | range_limit(d[5]) << 8 | range_limit(d[6]) << 16 | range_limit(d[7]) << 24;
        const int by = blk / bw, bx = blk - by * bw;
        *reinterpret_cast<uint2 *>(planes + im.plane_offset[comp] + ((long long)by * 8 + lane) * (bw * 8) + bx * 8) = o;
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The four upsampled chroma samples of columns x0 .. x0 + 3 (x0 a multiple of 4) of output row y, for one plane `a` of pitch
// `pw` whose true size is dw x dh.  hs == 2 here.
__device__ __forceinline__ void chroma_run(const uint8_t *__restrict__ a, int pw, int dw, int dh, int vs, int x0, int y, int (&out)[kRun]) {
    const int i0 = x0 >> 1;
    if (dw <= 2) {                                               // libjpeg's rule: no smoothing in either direction
        const uint8_t *row = a + (long long)(vs == 2 ? y >> 1 : y) * pw;
        out[0] = out[1] = row[min(i0, dw - 1)];
        out[2] = out[3] = row[min(i0 + 1, dw - 1)];
        return;
    }
    int t[4];                                                    // columns i0 - 1 .. i0 + 2, clamped into the plane
    if (vs == 1) {
        const uint8_t *row = a + (long long)y * pw;
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = row[clampi(i0 - 1 + k, 0, dw - 1)];
        out[0] = (3 * t[1] + t[0] + 1) >> 2, out[1] = (3 * t[1] + t[2] + 2) >> 2;
        out[2] = (3 * t[2] + t[1] + 1) >> 2, out[3] = (3 * t[2] + t[3] + 2) >> 2;
    } else {
        const int r = y >> 1;
        const uint8_t *near = a + (long long)r * pw;
        const uint8_t *far = a + (long long)clampi((y & 1) ? r + 1 : r - 1, 0, dh - 1) * pw;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = clampi(i0 - 1 + k, 0, dw - 1);
            t[k] = 3 * near[i] + far[i];
        }
        out[0] = (3 * t[1] + t[0] + 8) >> 4, out[1] = (3 * t[1] + t[2] + 7) >> 4;
        out[2] = (3 * t[2] + t[1] + 8) >> 4, out[3] = (3 * t[2] + t[3] + 7) >> 4;
    }
}

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ void __launch_bounds__(kThreads)
jpeg_to_rgb_kernel(const tsod_jpeg_image *__restrict__ table, const int4 *__restrict__ work, const uint8_t *__restrict__ planes,
                   uint8_t *__restrict__ out) {
    const int4 item = work[blockIdx.x];
    const tsod_jpeg_image &im = table[item.x];
    const int H = im.H, W = im.W;
    const int y = item.y * TSOD_JPEG_RGB_TILE_H + (threadIdx.x >> 6);
    const int x0 = item.z * TSOD_JPEG_RGB_TILE_W + (threadIdx.x & 63) * kRun;
    if (y >= H || x0 >= W) return;
    // the luma plane is 8 blocks_w wide, a multiple of 8 that covers W: the aligned word at x0 lies inside it
    const uint32_t yw = *reinterpret_cast<const uint32_t *>(planes + im.plane_offset[0] + (long long)y * (im.blocks_w[0] * 8) + x0);
    uint32_t r[kRun], g[kRun], b[kRun];
    if (im.n_comp == 1) {
#pragma unroll
        for (int k = 0; k < kRun; ++k) r[k] = g[k] = b[k] = (yw >> (8 * k)) & 0xffu;
    } else {
        int cb[kRun], cr[kRun];
        const uint8_t *pb = planes + im.plane_offset[1], *pr = planes + im.plane_offset[2];
        const int pw = im.blocks_w[1] * 8;                       // (both chroma planes have one grid)
        if (im.hs == 1) {
            const uint32_t bw4 = *reinterpret_cast<const uint32_t *>(pb + (long long)y * pw + x0);
            const uint32_t rw4 = *reinterpret_cast<const uint32_t *>(pr + (long long)y * pw + x0);
#pragma unroll
            for (int k = 0; k < kRun; ++k) cb[k] = (int)((bw4 >> (8 * k)) & 0xffu), cr[k] = (int)((rw4 >> (8 * k)) & 0xffu);
        } else {
            const int dw = (W + 1) >> 1, dh = im.vs == 2 ? (H + 1) >> 1 : H;
            chroma_run(pb, pw, dw, dh, im.vs, x0, y, cb);
            chroma_run(pr, pw, dw, dh, im.vs, x0, y, cr);
        }
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            const int Y = (int)((yw >> (8 * k)) & 0xffu), u = cb[k] - 128, v = cr[k] - 128;
            r[k] = clamp255(Y + ((91881 * v + 32768) >> 16));
            g[k] = clamp255(Y + ((-22554 * u - 46802 * v + 32768) >> 16));
            b[k] = clamp255(Y + ((116130 * u + 32768) >> 16));
        }
    }
    uint8_t *p = out + im.out_offset + ((long long)y * W + x0) * 3;
    if (x0 + kRun <= W && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
        uint32_t *p4 = reinterpret_cast<uint32_t *>(p);
        p4[0] = r[0] | g[0] << 8 | b[0] << 16 | r[1] << 24;
        p4[1] = g[1] | b[1] << 8 | r[2] << 16 | g[2] << 24;
        p4[2] = b[2] | r[3] << 8 | g[3] << 16 | b[3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < kRun; ++k)
            if (x0 + k < W) p[3 * k] = (uint8_t)r[k], p[3 * k + 1] = (uint8_t)g[k], p[3 * k + 2] = (uint8_t)b[k];
    }
}

using tsod_jpeg::aligned;
using tsod_jpeg::fits;
using tsod_jpeg::grid_fits;

// What both entries need of a record: its shape (jpeg_checks.h), the H / W range, grids that cover the image, planes inside
// `plane_bytes`
int check_image(const tsod_jpeg_image &im, int64_t plane_bytes) {
    TSOD_REQUIRE(tsod_jpeg::shape_ok(im), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(im.H > 0 && im.W > 0 && im.H <= 65535 && im.W <= 65535, TSOD_ERR_INVALID_ARG);
    for (int c = 0; c < im.n_comp; ++c) {
        const int64_t w = c ? tsod_cdiv(im.W, im.hs) : im.W, h = c ? tsod_cdiv(im.H, im.vs) : im.H;
        TSOD_REQUIRE((int64_t)im.blocks_w[c] * 8 >= w && (int64_t)im.blocks_h[c] * 8 >= h, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(grid_fits(im, c, im.plane_offset[c], plane_bytes, 8), TSOD_ERR_INVALID_ARG);
    }
    if (im.n_comp == 3) TSOD_REQUIRE(im.blocks_w[1] == im.blocks_w[2] && im.blocks_h[1] == im.blocks_h[2], TSOD_ERR_INVALID_ARG);
    return TSOD_OK;
}

}  // namespace

extern "C" int tsod_jpeg_parse(const uint8_t *data, size_t n, tsod_jpeg_info *info) {
    TSOD_REQUIRE(data && info, TSOD_ERR_INVALID_ARG);
    tsod_jpeg::State st;
    const int rc = tsod_jpeg::parse(data, n, st);
    if (rc == TSOD_OK) *info = st.info;
    return rc;
}

extern "C" int tsod_jpeg_entropy_decode(const uint8_t *data, size_t n, int16_t *coef, size_t capacity) {
    TSOD_REQUIRE(data && coef, TSOD_ERR_INVALID_ARG);
    tsod_jpeg::State st;
    return tsod_jpeg::decode(data, n, coef, capacity, st);
}

extern "C" int tsod_jpeg_idct_u8(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images,
                                 const int32_t *work_host, const int32_t *work, int32_t n_work, const int16_t *coef, int64_t coef_count,
                                 const uint16_t *quant, int64_t quant_count, uint8_t *planes, int64_t plane_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(n_images >= 0 && n_work >= 0 && coef_count >= 0 && quant_count >= 0 && plane_bytes >= 0, TSOD_ERR_INVALID_ARG);
    if (n_work == 0) return TSOD_OK;
    TSOD_REQUIRE(table_host && table && work_host && work && coef && quant && planes && n_images > 0, TSOD_ERR_INVALID_ARG);
    for (int i = 0; i < n_images; ++i) {
        const tsod_jpeg_image &im = table_host[i];
        const int rc = check_image(im, plane_bytes);
        if (rc != TSOD_OK) return rc;
        for (int c = 0; c < im.n_comp; ++c)
            TSOD_REQUIRE(grid_fits(im, c, im.coef_offset[c], coef_count, 64), TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(fits(im.quant_offset, (int64_t)64 * im.n_comp, quant_count, 64), TSOD_ERR_INVALID_ARG);
    }
    for (int64_t k = 0; k < n_work; ++k) {
        const int32_t *w = work_host + 4 * k;
        TSOD_REQUIRE(w[0] >= 0 && w[0] < n_images, TSOD_ERR_INVALID_ARG);
        const tsod_jpeg_image &im = table_host[w[0]];
        TSOD_REQUIRE(w[1] >= 0 && w[1] < im.n_comp, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(w[2] >= 0 && w[2] % TSOD_JPEG_IDCT_BLOCKS == 0 && w[2] < im.blocks_w[w[1]] * im.blocks_h[w[1]], TSOD_ERR_INVALID_ARG);
    }
    TSOD_REQUIRE(aligned(coef, 16) && aligned(quant, 16) && aligned(table, 16) && aligned(work, 16) && aligned(planes, 8), TSOD_ERR_ALIGNMENT);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)n_work), dim3(kThreads), 0, tsod_stream(stream), table,
                       reinterpret_cast<const int4 *>(work), coef, quant, planes);
    return tsod_launch_status();
}

extern "C" int tsod_jpeg_to_rgb_u8(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images,
                                   const int32_t *work_host, const int32_t *work, int32_t n_work, const uint8_t *planes,
                                   int64_t plane_bytes, uint8_t *out, int64_t out_bytes, tsod_stream_t stream) {
    TSOD_REQUIRE(n_images >= 0 && n_work >= 0 && plane_bytes >= 0 && out_bytes >= 0, TSOD_ERR_INVALID_ARG);
    if (n_work == 0) return TSOD_OK;
    TSOD_REQUIRE(table_host && table && work_host && work && planes && out && n_images > 0, TSOD_ERR_INVALID_ARG);
    for (int i = 0; i < n_images; ++i) {
        const tsod_jpeg_image &im = table_host[i];
        const int rc = check_image(im, plane_bytes);
        if (rc != TSOD_OK) return rc;
        TSOD_REQUIRE(fits(im.out_offset, (int64_t)3 * im.H * im.W, out_bytes, 1), TSOD_ERR_INVALID_ARG);
    }
    for (int64_t k = 0; k < n_work; ++k) {
        const int32_t *w = work_host + 4 * k;
        TSOD_REQUIRE(w[0] >= 0 && w[0] < n_images, TSOD_ERR_INVALID_ARG);
        const tsod_jpeg_image &im = table_host[w[0]];
        TSOD_REQUIRE(w[1] >= 0 && (int64_t)w[1] * TSOD_JPEG_RGB_TILE_H < im.H, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(w[2] >= 0 && (int64_t)w[2] * TSOD_JPEG_RGB_TILE_W < im.W, TSOD_ERR_INVALID_ARG);
    }
    TSOD_REQUIRE(aligned(table, 16) && aligned(work, 16) && aligned(planes, 8), TSOD_ERR_ALIGNMENT);
    hipLaunchKernelGGL(jpeg_to_rgb_kernel, dim3((unsigned)n_work), dim3(kThreads), 0, tsod_stream(stream), table,
                       reinterpret_cast<const int4 *>(work), planes, out);
    return tsod_launch_status();
}
