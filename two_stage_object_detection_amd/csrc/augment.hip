// augment.hip -- the reference's training transform (dataset/transform.py:4-12) on the GPU:
// RandomPhotometricDistort -> RandomHorizontalFlip -> ScaleJitter -> Resize((600, 600)) -> SanitizeBoundingBoxes.
// The random draws are made on the host (dataset/transform.py TrainTransform.make_params); these kernels apply them.
//
//   gray_mean_kernel      contrast's grayscale mean: the ops in front of contrast are recomputed from the u8 source
//                         (never materialised); fixed-order two-level sum (per-workgroup f64 tree, then a second tree
//                         over TSOD_AUGMENT_MEAN_PARTS partials in every consumer workgroup), no atomics
//   AugU8                 resize_aa.h's source policy of the first antialiased resize: colour ops + permutation +
//                         mirrored column index applied while the source region is staged into LDS as three f32
//                         planes (the clamps make the ops nonlinear, so they run on source pixels before any tap);
//                         its prologue reduces the mean's partials.  The second resize, f32 -> f32, is resize.hip's.
//   boxes_kernel          flip, two scalings, sanitize and a stable compaction of boxes + labels, one workgroup per image
// Compiled with -ffp-contract=off: every expression rounds like the f32 restatement of DESIGN 4.15.
#include "resize_aa.h"

namespace {

constexpr int kParts = TSOD_AUGMENT_MEAN_PARTS;
constexpr int kColorOps = TSOD_AUG_BRIGHTNESS | TSOD_AUG_CONTRAST | TSOD_AUG_SATURATION | TSOD_AUG_HUE;
constexpr int kAllFlags = kColorOps | TSOD_AUG_CONTRAST_FIRST | TSOD_AUG_PERMUTE;

__host__ __device__ inline float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// torchvision _rgb_to_grayscale_image: r*0.2989 + g*0.587 + b*0.114, in that order
__host__ __device__ inline float gray_of(const float c[3]) { return c[0] * 0.2989f + c[1] * 0.587f + c[2] * 0.114f; }

// torchvision _blend: clamp(f*x + (1-f)*m, 0, 1)
__host__ __device__ inline float blend(float x, float m, float f) { return clamp01(f * x + (1.f - f) * m); }

// adjust_hue: _rgb_to_hsv, H = (H + hue) mod 1 (torch.remainder), _hsv_to_rgb; v itself is not clamped
__host__ __device__ inline void hue_shift(float c[3], float hue) {
    const float r = c[0], g = c[1], b = c[2];
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float range = maxc - minc;
    const float s = range / (eqc ? 1.f : maxc);
    const float div = eqc ? 1.f : range;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = (rc + 2.f) - bc;
    else h = (gc + 4.f) - rc;
    h = fmodf(h * (float)(1.0 / 6.0) + 1.f, 1.f);
    h = fmodf(h + hue, 1.f);
    if (h != 0.f && h < 0.f) h += 1.f;
    const float v = maxc;
    const float h6 = h * 6.f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    int i = (int)fl % 6;
    if (i < 0) i += 6;
    const float sxf = s * f;
    const float oms = 1.f - s;
    const float q = clamp01((1.f - sxf) * v);
    const float t = clamp01((sxf + oms) * v);
    const float p = clamp01(oms * v);
    switch (i) {
        case 0: c[0] = v; c[1] = t; c[2] = p; break;
        case 1: c[0] = q; c[1] = v; c[2] = p; break;
        case 2: c[0] = p; c[1] = v; c[2] = t; break;
        case 3: c[0] = p; c[1] = q; c[2] = v; break;
        case 4: c[0] = t; c[1] = p; c[2] = v; break;
        default: c[0] = v; c[1] = p; c[2] = q; break;
    }
}

__host__ __device__ inline void contrast_op(float c[3], float mean, float f) {
    for (int k = 0; k < 3; ++k) c[k] = blend(c[k], mean, f);
}

__host__ __device__ inline void saturation_op(float c[3], float f) {
    const float g = gray_of(c);
    for (int k = 0; k < 3; ++k) c[k] = blend(c[k], g, f);
}

// RandomPhotometricDistort._transform on one pixel.  at_contrast: return the pixel as contrast sees it (in the
// 1/white domain), for the mean pass; the caller only asks when CONTRAST is set.
__host__ __device__ inline void aug_color(float c[3], const tsod_photometric &p, float mean, bool at_contrast) {
    const int fl = p.flags;
    if (fl & kColorOps) {
        for (int k = 0; k < 3; ++k) c[k] = c[k] / p.white;
        if (fl & TSOD_AUG_BRIGHTNESS)
            for (int k = 0; k < 3; ++k) c[k] = clamp01(c[k] * p.brightness);
        const bool con = (fl & TSOD_AUG_CONTRAST) != 0, first = (fl & TSOD_AUG_CONTRAST_FIRST) != 0;
        if (con && first) {
            if (at_contrast) return;
            contrast_op(c, mean, p.contrast);
        }
        if (fl & TSOD_AUG_SATURATION) saturation_op(c, p.saturation);
        if (fl & TSOD_AUG_HUE) hue_shift(c, p.hue);
        if (con && !first) {
            if (at_contrast) return;
            contrast_op(c, mean, p.contrast);
        }
        for (int k = 0; k < 3; ++k) c[k] = c[k] * p.white;
    }
    if (fl & TSOD_AUG_PERMUTE) {
        const float t[3] = {c[0], c[1], c[2]};
        for (int k = 0; k < 3; ++k) c[k] = t[p.perm[k]];
    }
}

bool valid_params(const tsod_photometric *p) {
    if (!p || (p->flags & ~kAllFlags) || !(p->white > 0.f) || !isfinite(p->white)) return false;
    if ((p->flags & TSOD_AUG_HUE) && !(p->hue >= -0.5f && p->hue <= 0.5f)) return false;
    if (p->flags & TSOD_AUG_PERMUTE) {
        int seen = 0;
        for (int k = 0; k < 3; ++k) {
            if (p->perm[k] < 0 || p->perm[k] > 2) return false;
            seen |= 1 << p->perm[k];
        }
        if (seen != 7) return false;
    }
    return true;
}

__device__ inline void load_rgb(const unsigned char *src, long pitch, int y, int x, float c[3]) {
    const unsigned char *px = src + (long)y * pitch + (long)x * 3;
    c[0] = (float)px[0];
    c[1] = (float)px[1];
    c[2] = (float)px[2];
}

constexpr int kMeanThreads = 1024;

// Workgroup b sums pixels [b*chunk, (b+1)*chunk) in row-major order, thread t every kMeanThreads-th from the t-th on
// (its row and column advanced incrementally: no integer division in the loop).
__global__ void __launch_bounds__(kMeanThreads)
gray_mean_kernel(const unsigned char *__restrict__ src, int H, int W, long pitch, tsod_photometric p,
                 double *__restrict__ partials) {
    __shared__ double red[kMeanThreads];
    const long n = (long)H * W;
    const long chunk = (n + kParts - 1) / kParts;
    const long q0 = (long)blockIdx.x * chunk, q1 = min(q0 + chunk, n);
    const int step_y = kMeanThreads / W, step_x = kMeanThreads % W;
    double acc = 0.0;
    long q = q0 + threadIdx.x;
    int y = (int)(q / W), x = (int)(q % W);
    for (; q < q1; q += kMeanThreads) {
        float c[3];
        load_rgb(src, pitch, y, x, c);
        aug_color(c, p, 0.f, true);
        acc += (double)gray_of(c);
        y += step_y;
        x += step_x;
        if (x >= W) {
            x -= W;
            ++y;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kMeanThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// The second level of the mean: every thread of the workgroup calls it; same tree everywhere.
static_assert(kThreads == kParts, "one partial per thread");
__device__ float reduce_mean(const double *__restrict__ partials, long n, double *red) {
    red[threadIdx.x] = partials ? partials[threadIdx.x] : 0.0;
    __syncthreads();
    for (int s = kParts / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float m = (float)(red[0] / (double)n);
    __syncthreads();
    return m;
}

// The first resize's source: u8 RGB rows through the colour ops, read at the mirrored column when flipped.
struct AugU8 : F32Planes {
    const unsigned char *src;
    int H, W;
    long pitch;
    tsod_photometric p;
    const double *mean_partials;
    int flip;
    float mean;                                          // set by prologue()
    static constexpr int C = 3;
    static constexpr int kPrologueDoubles = kParts;
    __device__ void prologue(double *red) {
        mean = (p.flags & TSOD_AUG_CONTRAST) ? reduce_mean(mean_partials, (long)H * W, red) : 0.f;
    }
    __device__ auto src_px(int y, int xf) const {                    // xf: column of the flipped image
        float c[3];
        load_rgb(src, pitch, y, flip ? W - 1 - xf : xf, c);
        aug_color(c, p, mean, false);
        return [c](int k) { return c[k]; };
    }
    __device__ void stage(unsigned char *lds, const TileGeom &g, int cap_rows, int cap_cols) const {
        const long plane = (long)cap_rows * cap_cols;
        for (int r = threadIdx.x / kTX; r < g.rows; r += kTY)        // a row of the region per 32 threads
            for (int col = threadIdx.x % kTX; col < g.cols; col += kTX) {
                const int y = g.ry0 + r, xf = g.rx0 + col;
                if (y >= H || xf >= W) continue;
                const auto px = src_px(y, xf);
                float *d = reinterpret_cast<float *>(lds) + (long)r * cap_cols + col;
                d[0] = px(0);
                d[plane] = px(1);
                d[2 * plane] = px(2);
            }
    }
};

__global__ void __launch_bounds__(kThreads)
boxes_kernel(const float *__restrict__ boxes, const long long *__restrict__ labels, const int *__restrict__ iparams,
             const float *__restrict__ fparams, float *__restrict__ boxes_out, long long *__restrict__ labels_out,
             int *__restrict__ kept) {
    __shared__ int scan[kThreads];
    const int b = blockIdx.x;
    const int first = iparams[4 * b], count = iparams[4 * b + 1], flip = iparams[4 * b + 2];
    const float *fp = fparams + 8 * b;
    const float W = fp[0], sx1 = fp[1], sy1 = fp[2], sx2 = fp[3], sy2 = fp[4], OW = fp[5], OH = fp[6], ms = fp[7];
    int base = 0;
    for (int c0 = 0; c0 < count; c0 += kThreads) {
        const int i = c0 + (int)threadIdx.x;
        bool keep = false;
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
        if (i < count) {
            const float *bx = boxes + (long)(first + i) * 4;
            x1 = bx[0];
            y1 = bx[1];
            x2 = bx[2];
            y2 = bx[3];
            if (flip) {
                const float a = W - x2, c = W - x1;
                x1 = a;
                x2 = c;
            }
            x1 = x1 * sx1; x2 = x2 * sx1; y1 = y1 * sy1; y2 = y2 * sy1;   // ScaleJitter's resize
            x1 = x1 * sx2; x2 = x2 * sx2; y1 = y1 * sy2; y2 = y2 * sy2;   // Resize((600, 600))
            keep = (x2 - x1 >= ms) && (y2 - y1 >= ms) && x1 >= 0.f && y1 >= 0.f && x2 >= 0.f && y2 >= 0.f &&
                   x1 <= OW && x2 <= OW && y1 <= OH && y2 <= OH;
        }
        scan[threadIdx.x] = keep ? 1 : 0;                       // inclusive scan of the keep flags
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const int v = (int)threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        if (keep) {
            const long o = (long)first + base + scan[threadIdx.x] - 1;
            float *d = boxes_out + o * 4;
            d[0] = x1;
            d[1] = y1;
            d[2] = x2;
            d[3] = y2;
            labels_out[o] = labels[first + i];
        }
        base += scan[kThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) kept[b] = base;
}

}  // namespace

extern "C" int tsod_augment_gray_mean_partials(const uint8_t *src, int32_t H, int32_t W, int64_t src_row_bytes,
                                               const tsod_photometric *params, double *partials, tsod_stream_t stream) {
    TSOD_REQUIRE(src && partials && valid_params(params), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(H > 0 && W > 0 && src_row_bytes >= (int64_t)W * 3, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(params->flags & TSOD_AUG_CONTRAST, TSOD_ERR_INVALID_ARG);
    hipLaunchKernelGGL(gray_mean_kernel, dim3(kParts), dim3(kMeanThreads), 0, tsod_stream(stream), src, H, W,
                       (long)src_row_bytes, *params, partials);
    return tsod_launch_status();
}

extern "C" int tsod_augment_resize_u8_f32(const uint8_t *src, int32_t H, int32_t W, int64_t src_row_bytes,
                                          const tsod_photometric *params, const double *mean_partials, int32_t flip,
                                          const int32_t *yfirst, const int32_t *ycount, const float *ywt,
                                          const int32_t *xfirst, const int32_t *xcount, const float *xwt, int32_t OH,
                                          int32_t OW, float *out, int64_t stride_y, int64_t stride_x, int64_t stride_c,
                                          int32_t C_out, tsod_stream_t stream) {
    TSOD_REQUIRE(src && yfirst && ycount && ywt && xfirst && xcount && xwt && out && valid_params(params),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(H > 0 && W > 0 && OH > 0 && OW > 0 && C_out >= 3 && C_out <= 4 && (flip == 0 || flip == 1),
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(src_row_bytes >= (int64_t)W * 3, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(mean_partials || !(params->flags & TSOD_AUG_CONTRAST), TSOD_ERR_INVALID_ARG);
    AugU8 a;
    a.src = src, a.H = H, a.W = W, a.pitch = (long)src_row_bytes;
    a.p = *params, a.mean_partials = mean_partials, a.flip = flip, a.mean = 0.f;
    return launch_resize(a, H, W, yfirst, ycount, ywt, xfirst, xcount, xwt, OH, OW, 1.0f, out, stride_y, stride_x, stride_c,
                         C_out, stream);
}

extern "C" int tsod_augment_boxes_f32(const float *boxes, const int64_t *labels, int32_t B, const int32_t *iparams,
                                      const float *fparams, float *boxes_out, int64_t *labels_out, int32_t *kept,
                                      tsod_stream_t stream) {
    TSOD_REQUIRE(iparams && fparams && kept && B > 0 && B <= 65535, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(boxes && labels && boxes_out && labels_out, TSOD_ERR_INVALID_ARG);
    hipLaunchKernelGGL(boxes_kernel, dim3(B), dim3(kThreads), 0, tsod_stream(stream), boxes,
                       reinterpret_cast<const long long *>(labels), iparams, fparams, boxes_out,
                       reinterpret_cast<long long *>(labels_out), kept);
    return tsod_launch_status();
}

extern "C" int tsod_augment_color_host(const float *rgb, int64_t n, const tsod_photometric *params, float mean,
                                       float *rgb_out) {
    TSOD_REQUIRE(rgb && rgb_out && n >= 0 && valid_params(params), TSOD_ERR_INVALID_ARG);
    for (int64_t i = 0; i < n; ++i) {
        float c[3] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
        aug_color(c, *params, mean, false);
        rgb_out[3 * i] = c[0];
        rgb_out[3 * i + 1] = c[1];
        rgb_out[3 * i + 2] = c[2];
    }
    return TSOD_OK;
}
