// jpeg_scan.h -- what the host still does when the Huffman pass runs on the device: one byte-speed
// sweep over the entropy-coded segment that unstuffs FF 00, checks and removes the restart markers, and lays every restart
// interval out on a 4-byte boundary; and the scan's code tables in the fixed-size layout of include/tsod.h.  Plain C++17 in the
// style of jpeg_entropy.h: no HIP, no statics, no allocation; nothing is read outside [data, data + n) and nothing is written
// outside the stated capacities.
#pragma once
#include "jpeg_entropy.h"

namespace tsod_jpeg {

// The capacities scan_prepare needs at most.  A file of n bytes cannot hold more than n / 2 restart markers.
inline int scan_sizes(const tsod_jpeg_info &info, size_t n, int64_t *stream_bytes, int32_t *n_segments) {
    const int64_t n_mcu = (int64_t)info.mcus_x * info.mcus_y;
    if (!stream_bytes || !n_segments || info.mcus_x <= 0 || info.mcus_y <= 0 || info.restart_interval < 0) return TSOD_ERR_INVALID_ARG;
    int64_t segs = info.restart_interval ? (n_mcu + info.restart_interval - 1) / info.restart_interval : 1;
    if (segs > (int64_t)(n / 2) + 1) segs = (int64_t)(n / 2) + 1;
    *n_segments = (int32_t)segs;
    *stream_bytes = ((int64_t)n + 4 * segs + 3) / 4 * 4;
    return TSOD_OK;
}

inline void copy_table(tsod_jpeg_huff &out, const Huffman &h) {
    memcpy(out.look, h.look, sizeof(out.look));
    memcpy(out.maxcode, h.maxcode, sizeof(out.maxcode));
    memcpy(out.valoff, h.valoff, sizeof(out.valoff));
    memcpy(out.vals, h.vals, sizeof(out.vals));
}
static_assert(sizeof(((tsod_jpeg_huff *)0)->look) == sizeof(((Huffman *)0)->look) && sizeof(((tsod_jpeg_huff *)0)->vals) == 256, "one layout");

inline int scan_prepare(const uint8_t *data, size_t n, uint8_t *stream, int64_t stream_capacity, int64_t *stream_bytes,
                        tsod_jpeg_segment *segments, int32_t segment_capacity, int32_t *n_segments, tsod_jpeg_huff *tables, State &st) {
    const int rc = parse(data, n, st);
    if (rc != TSOD_OK) return rc;
    if (!stream || !stream_bytes || !segments || !n_segments || !tables || stream_capacity < 0 || segment_capacity < 0)
        return TSOD_ERR_INVALID_ARG;
    const tsod_jpeg_info &info = st.info;
    memset(tables, 0, sizeof(tsod_jpeg_huff) * TSOD_JPEG_HUFF_TABLES);
    for (int c = 0; c < info.n_comp; ++c) {
        copy_table(tables[2 * c], st.dc[st.td[c]]);
        copy_table(tables[2 * c + 1], st.ac[st.ta[c]]);
    }
    const int64_t n_mcu = (int64_t)info.mcus_x * info.mcus_y;
    const int64_t interval = info.restart_interval ? info.restart_interval : n_mcu;
    size_t pos = st.scan;
    int64_t out = 0;
    int32_t seg = 0;
    int next_rst = 0;
    for (int64_t first = 0; first < n_mcu; first += interval, ++seg) {
        if (seg >= segment_capacity) return TSOD_ERR_INVALID_ARG;
        const int64_t start = out;
        while (pos < n) {                                        // Bits::fill's rule: a marker or the end of the data stops the supply
            const uint8_t b = data[pos];
            if (b == 0xFF) {
                if (pos + 1 >= n || data[pos + 1] != 0x00) break;
                pos += 2;
            } else {
                pos += 1;
            }
            if (out >= stream_capacity) return TSOD_ERR_INVALID_ARG;
            stream[out++] = b;
        }
        const bool last = first + interval >= n_mcu;
        tsod_jpeg_segment &rec = segments[seg];
        rec.stream_offset = start;
        rec.bit_length = 8 * (out - start);
        rec.image = 0;
        rec.first_mcu = (int32_t)first;
        rec.n_mcu = (int32_t)(last ? n_mcu - first : interval);
        rec.flags = last ? 0 : 1;
        while (out % 4) {
            if (out >= stream_capacity) return TSOD_ERR_INVALID_ARG;
            stream[out++] = 0;
        }
        if (!last) {                                             // decode()'s restart rule: fill bytes, then the expected RSTn
            size_t p = pos;
            while (p < n && data[p] == 0xFF) ++p;
            if (p >= n || p == pos || data[p] != 0xD0 + next_rst) return TSOD_ERR_INVALID_ARG;
            next_rst = (next_rst + 1) & 7;
            pos = p + 1;
        }
    }
    *stream_bytes = out;
    *n_segments = seg;
    return TSOD_OK;
}

}  // namespace tsod_jpeg
