// jpeg_checks.h -- the host checks that the launch entries of csrc/jpeg.hip and csrc/jpeg_huffman.hip share (DESIGN.md section
// 4.29): pointer alignment, a range inside a buffer, and the shape of an image record - component count, sampling, block grids.
// What differs between the entries (planes inside plane_bytes or coefficients inside coef_count, the H / W range, whole-MCU
// grids) stays with them.  Plain C++17 in the style of jpeg_scan.h: host only, no HIP, no statics, no allocation.
#pragma once
#include <stdint.h>
#include "../../include/tsod.h"

namespace tsod_jpeg {

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// [offset, offset + extent) inside [0, size), offset a multiple of unit
inline bool fits(int64_t offset, int64_t extent, int64_t size, int64_t unit) {
    return offset >= 0 && offset % unit == 0 && extent >= 0 && offset <= size && extent <= size - offset;
}

// One or three components, a sampling the kernels know (hs and vs are then nonzero), every grid within [1, 8192] blocks a side
inline bool shape_ok(const tsod_jpeg_image &im) {
    if (im.n_comp != 1 && im.n_comp != 3) return false;
    const bool full = im.hs == 1 && im.vs == 1;
    if (!(im.n_comp == 1 ? full : (full || (im.hs == 2 && (im.vs == 1 || im.vs == 2))))) return false;
    for (int c = 0; c < im.n_comp; ++c)
        if (!(im.blocks_w[c] > 0 && im.blocks_h[c] > 0 && im.blocks_w[c] <= 8192 && im.blocks_h[c] <= 8192)) return false;
    return true;
}

// The 64 elements per block of component c - coefficients or samples alike - inside a buffer of `size` elements
inline bool grid_fits(const tsod_jpeg_image &im, int c, int64_t offset, int64_t size, int64_t unit) {
    return fits(offset, (int64_t)64 * im.blocks_w[c] * im.blocks_h[c], size, unit);
}

}  // namespace tsod_jpeg
