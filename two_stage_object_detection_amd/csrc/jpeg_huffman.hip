// jpeg_huffman.hip -- the JPEG Huffman pass on the device (include/tsod.h "The Huffman pass on the
// DEVICE"): the host sweep of jpeg_scan.h behind two C entry points, and one kernel that decodes every restart interval of a
// batch, one workgroup per interval, as a workgroup-local self-synchronising decoder.  The per-lane work is
// jpeg_huffman_core.h, shared with the stand-alone CPU program tests/jpeg_huffman_main.cpp; this file is the orchestration:
// rounds, the fixpoint vote, the scan and the status word.  Every address comes from records checked on the host.
#include "jpeg_huffman_core.h"
#include "jpeg_scan.h"
#include "tsod_internal.h"

namespace {

using namespace tsod_jpeg;

constexpr int kThreads = kHuffLanes;
constexpr int kTableWords = (int)(sizeof(tsod_jpeg_huff) * TSOD_JPEG_HUFF_TABLES / 4);
static_assert(sizeof(tsod_jpeg_huff) % 4 == 0 && sizeof(tsod_jpeg_segment) == 32 && kThreads % 64 == 0, "layouts the kernel relies on");

__global__ void __launch_bounds__(kThreads)
jpeg_clear_kernel(uint4 *__restrict__ coef16, long long n16, int16_t *__restrict__ tail, int n_tail, int32_t *__restrict__ status,
                  int n_images) {
    const long long stride = (long long)gridDim.x * kThreads;
    const long long first = (long long)blockIdx.x * kThreads + threadIdx.x;
    for (long long i = first; i < n16; i += stride) coef16[i] = make_uint4(0u, 0u, 0u, 0u);
    for (long long i = first; i < n_tail; i += stride) tail[i] = 0;
    for (long long i = first; i < n_images; i += stride) status[i] = 0;
}

__global__ void __launch_bounds__(kThreads)
jpeg_huffman_kernel(const tsod_jpeg_image *__restrict__ table, const tsod_jpeg_segment *__restrict__ segments,
                    const int4 *__restrict__ work, const uint32_t *__restrict__ stream, const tsod_jpeg_huff *__restrict__ huff,
                    int16_t *__restrict__ coef, int32_t *__restrict__ status, int subseq_words) {
    __shared__ uint32_t lds_tables[kTableWords];                 // the image's six code tables
    __shared__ HuffState lds_end[kThreads];                      // every lane's end state
    __shared__ uint4 lds_scan[2][kThreads];                      // (blocks, dc[0], dc[1], dc[2]) ping-pong
    const int lane = threadIdx.x;
    const tsod_jpeg_segment seg = segments[work[blockIdx.x].x];
    const tsod_jpeg_image &im = table[seg.image];
    const HuffGeometry g = huff_geometry(im, seg);
    const uint32_t bits = (uint32_t)seg.bit_length;
    const SegmentBits s = {stream + seg.stream_offset / 4, (bits + 31u) / 32u, bits};
    const bool restart_follows = (seg.flags & 1) != 0;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(huff + (long long)seg.image * TSOD_JPEG_HUFF_TABLES);
    for (int i = lane; i < kTableWords; i += kThreads) lds_tables[i] = src[i];
    __syncthreads();
    const tsod_jpeg_huff *tables = reinterpret_cast<const tsod_jpeg_huff *>(lds_tables);

    const uint32_t sub_bits = 32u * (uint32_t)subseq_words, round_bits = sub_bits * kThreads;
    const uint32_t n_rounds = bits / round_bits + (bits % round_bits ? 1u : 0u);
    HuffState carry_state = {0u, 0u};                            // the same in every lane
    HuffTally carry = {0u, {0u, 0u, 0u}};
    int32_t flags = 0;
    for (uint32_t r = 0; r < n_rounds; ++r) {
        const uint32_t first_bit = r * round_bits + (uint32_t)lane * sub_bits;     // < bits + round_bits: no wrap
        const uint32_t limit = min(first_bit + sub_bits, bits);
        const bool active = first_bit < bits;                    // a lane past the segment's end takes no part in the vote
        const int last_active = (int)min((bits - 1u - r * round_bits) / sub_bits, (uint32_t)(kThreads - 1));
        HuffState start = lane == 0 ? carry_state : assumed_state(first_bit);
        HuffTally mine = {0u, {0u, 0u, 0u}};
        int32_t unused = 0;
        bool changed = true;                                     // the first pass: every lane from its assumed start
        for (int k = 0; k <= kThreads; ++k) {                    // after pass k lanes 0 .. k are final: at most 256 passes do work
            if (changed) {
                mine = HuffTally{0u, {0u, 0u, 0u}};
                lds_end[lane] = huff_run<false>(s, tables, g, start, limit, sub_bits, restart_follows, mine, nullptr, unused);
            }
            __syncthreads();
            const HuffState before = lane == 0 ? start : lds_end[lane - 1];
            // An ERROR end state is never taken over: the lane that made it reports it in the last pass if it is the true
            // parse's, and a guess that failed must not undo the lanes after it that are already in step.
            changed = active && before.p != kErrorP && !same(before, start);
            if (!__syncthreads_or(changed)) break;               // (also: every read above precedes every write of the next pass)
            if (changed) start = before;
        }
        // inclusive scan of the tallies over the lanes
        lds_scan[0][lane] = make_uint4(mine.blocks, mine.dc[0], mine.dc[1], mine.dc[2]);
        __syncthreads();
        int from = 0;
        for (int d = 1; d < kThreads; d <<= 1, from ^= 1) {
            uint4 v = lds_scan[from][lane];
            if (lane >= d) {
                const uint4 o = lds_scan[from][lane - d];
                v.x += o.x, v.y += o.y, v.z += o.z, v.w += o.w;
            }
            lds_scan[from ^ 1][lane] = v;
            __syncthreads();
        }
        const uint4 incl = lds_scan[from][lane], total = lds_scan[from][kThreads - 1];
        HuffTally at = {carry.blocks + incl.x - mine.blocks, {carry.dc[0] + incl.y - mine.dc[0], carry.dc[1] + incl.z - mine.dc[1],
                                                              carry.dc[2] + incl.w - mine.dc[2]}};
        huff_run<true>(s, tables, g, start, limit, sub_bits, restart_follows, at, coef, flags);
        carry_state = lds_end[last_active];
        carry.blocks += total.x, carry.dc[0] += total.y, carry.dc[1] += total.z, carry.dc[2] += total.w;
        __syncthreads();                                         // lds_end and lds_scan are free for the next round
    }
    if (lane == 0 && carry.blocks < g.n_blocks) flags |= kStatusBlocks;
    if (flags) atomicOr(status + seg.image, flags);
}

bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// [offset, offset + extent) inside [0, size), offset a multiple of unit
bool fits(int64_t offset, int64_t extent, int64_t size, int64_t unit) {
    return offset >= 0 && offset % unit == 0 && extent >= 0 && offset <= size && extent <= size - offset;
}

// What the Huffman kernel reads of a record: the component count, the sampling, whole-MCU grids, coefficients inside coef_count
int check_image(const tsod_jpeg_image &im, int64_t coef_count) {
    TSOD_REQUIRE(im.n_comp == 1 || im.n_comp == 3, TSOD_ERR_INVALID_ARG);
    const bool sampling = im.n_comp == 1 ? (im.hs == 1 && im.vs == 1) : ((im.hs == 1 && im.vs == 1) || (im.hs == 2 && (im.vs == 1 || im.vs == 2)));
    TSOD_REQUIRE(sampling, TSOD_ERR_INVALID_ARG);
    for (int c = 0; c < im.n_comp; ++c) {
        TSOD_REQUIRE(im.blocks_w[c] > 0 && im.blocks_h[c] > 0 && im.blocks_w[c] <= 8192 && im.blocks_h[c] <= 8192, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(fits(im.coef_offset[c], (int64_t)64 * im.blocks_w[c] * im.blocks_h[c], coef_count, 64), TSOD_ERR_INVALID_ARG);
    }
    TSOD_REQUIRE(im.blocks_w[0] % im.hs == 0 && im.blocks_h[0] % im.vs == 0, TSOD_ERR_INVALID_ARG);
    for (int c = 1; c < im.n_comp; ++c)
        TSOD_REQUIRE(im.blocks_w[c] == im.blocks_w[0] / im.hs && im.blocks_h[c] == im.blocks_h[0] / im.vs, TSOD_ERR_INVALID_ARG);
    return TSOD_OK;
}

}  // namespace

extern "C" int tsod_jpeg_scan_sizes(const tsod_jpeg_info *info, size_t n, int64_t *stream_bytes, int32_t *n_segments) {
    TSOD_REQUIRE(info, TSOD_ERR_INVALID_ARG);
    return tsod_jpeg::scan_sizes(*info, n, stream_bytes, n_segments);
}

extern "C" int tsod_jpeg_scan_prepare(const uint8_t *data, size_t n, uint8_t *stream, int64_t stream_capacity, int64_t *stream_bytes,
                                      tsod_jpeg_segment *segments, int32_t segment_capacity, int32_t *n_segments,
                                      tsod_jpeg_huff *tables) {
    TSOD_REQUIRE(data, TSOD_ERR_INVALID_ARG);
    tsod_jpeg::State st;
    return tsod_jpeg::scan_prepare(data, n, stream, stream_capacity, stream_bytes, segments, segment_capacity, n_segments, tables, st);
}

extern "C" int tsod_jpeg_huffman_i16(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images,
                                     const tsod_jpeg_segment *segments_host, const tsod_jpeg_segment *segments, int32_t n_segments,
                                     const int32_t *work_host, const int32_t *work, int32_t n_work, const uint8_t *stream,
                                     int64_t stream_bytes, const tsod_jpeg_huff *huff, int64_t n_huff, int16_t *coef,
                                     int64_t coef_count, int32_t *status, int32_t subseq_words, tsod_stream_t stream_handle) {
    TSOD_REQUIRE(subseq_words >= 1 && subseq_words <= 64, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_images >= 0 && n_segments >= 0 && n_work >= 0 && stream_bytes >= 0 && n_huff >= 0 && coef_count >= 0, TSOD_ERR_INVALID_ARG);
    if (n_work == 0) return TSOD_OK;
    TSOD_REQUIRE(table_host && table && segments_host && segments && work_host && work && stream && huff && coef && status,
                 TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_images > 0 && n_segments > 0 && n_huff >= (int64_t)TSOD_JPEG_HUFF_TABLES * n_images, TSOD_ERR_INVALID_ARG);
    for (int i = 0; i < n_images; ++i) {
        const int rc = check_image(table_host[i], coef_count);
        if (rc != TSOD_OK) return rc;
    }
    int32_t image = -1;                                          // segments: sorted by image, tiling each image's MCUs in order
    int64_t next_mcu = 0, n_mcu = 0;
    for (int k = 0; k < n_segments; ++k) {
        const tsod_jpeg_segment &sg = segments_host[k];
        if (sg.image != image) {
            TSOD_REQUIRE(next_mcu == n_mcu && sg.image == image + 1 && sg.image < n_images, TSOD_ERR_INVALID_ARG);
            image = sg.image;
            const tsod_jpeg_image &im = table_host[image];
            next_mcu = 0, n_mcu = (int64_t)(im.blocks_w[0] / im.hs) * (im.blocks_h[0] / im.vs);
        }
        TSOD_REQUIRE(sg.n_mcu > 0 && sg.first_mcu == next_mcu && sg.n_mcu <= n_mcu - next_mcu, TSOD_ERR_INVALID_ARG);
        next_mcu += sg.n_mcu;
        TSOD_REQUIRE(sg.flags == 0 || sg.flags == 1, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(sg.bit_length >= 0 && sg.bit_length % 8 == 0 && sg.bit_length <= TSOD_JPEG_MAX_SEGMENT_BITS, TSOD_ERR_INVALID_ARG);
        TSOD_REQUIRE(fits(sg.stream_offset, (sg.bit_length + 31) / 32 * 4, stream_bytes, 4), TSOD_ERR_INVALID_ARG);
    }
    TSOD_REQUIRE(next_mcu == n_mcu && image == n_images - 1, TSOD_ERR_INVALID_ARG);
    for (int64_t k = 0; k < n_work; ++k) TSOD_REQUIRE(work_host[4 * k] >= 0 && work_host[4 * k] < n_segments, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(aligned(table, 16) && aligned(segments, 16) && aligned(work, 16) && aligned(coef, 16) && aligned(stream, 4) &&
                     aligned(huff, 4) && aligned(status, 4),
                 TSOD_ERR_ALIGNMENT);
    const long long n16 = coef_count / 8;
    const int n_tail = (int)(coef_count % 8);
    const unsigned clear_blocks = (unsigned)std::min<long long>(std::max<long long>(tsod_cdiv(n16, kThreads), 1), 2048);
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3(clear_blocks), dim3(kThreads), 0, tsod_stream(stream_handle),
                       reinterpret_cast<uint4 *>(coef), n16, coef + n16 * 8, n_tail, status, n_images);
    hipLaunchKernelGGL(jpeg_huffman_kernel, dim3((unsigned)n_work), dim3(kThreads), 0, tsod_stream(stream_handle), table, segments,
                       reinterpret_cast<const int4 *>(work), reinterpret_cast<const uint32_t *>(stream), huff, coef, status,
                       (int)subseq_words);
    return tsod_launch_status();
}
