// jpeg_huffman.hip -- the JPEG Huffman pass on the device (include/tsod.h "The Huffman pass on the
// DEVICE"): the host sweep of jpeg_scan.h behind two C entry points, and one kernel that decodes every restart interval of a
// batch, one workgroup per interval, as a workgroup-local self-synchronising decoder.  The per-lane work is
// jpeg_huffman_core.h, shared with the stand-alone CPU program tests/jpeg_huffman_main.cpp; this file is the orchestration:
// rounds, the fixpoint vote, the scan and the status word.  Every address comes from records checked on the host
// (jpeg_checks.h, check_batch; check_entry is the opening both launch entries share).  The split
// mode (tsod_jpeg_huffman_split_i16, jpeg_huffman_split.h) gives a segment's subsequences to several workgroups in chunks: three
// launches - sync, stitch, write - ordered by the stream alone; the CPU program for it is tests/jpeg_huffman_split_main.cpp.
#include "jpeg_checks.h"
#include "jpeg_huffman_core.h"
#include "jpeg_huffman_split.h"
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

// What the Huffman kernels read of a record: its shape (jpeg_checks.h), whole-MCU grids, coefficients inside coef_count
int check_image(const tsod_jpeg_image &im, int64_t coef_count) {
    TSOD_REQUIRE(shape_ok(im), TSOD_ERR_INVALID_ARG);
    for (int c = 0; c < im.n_comp; ++c) TSOD_REQUIRE(grid_fits(im, c, im.coef_offset[c], coef_count, 64), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(im.blocks_w[0] % im.hs == 0 && im.blocks_h[0] % im.vs == 0, TSOD_ERR_INVALID_ARG);
    for (int c = 1; c < im.n_comp; ++c)
        TSOD_REQUIRE(im.blocks_w[c] == im.blocks_w[0] / im.hs && im.blocks_h[c] == im.blocks_h[0] / im.vs, TSOD_ERR_INVALID_ARG);
    return TSOD_OK;
}

// The records both launch entries read: every image, and segments sorted by image that tile each image's MCUs in order
int check_batch(const tsod_jpeg_image *table_host, int32_t n_images, const tsod_jpeg_segment *segments_host, int32_t n_segments,
                int64_t stream_bytes, int64_t n_huff, int64_t coef_count) {
    TSOD_REQUIRE(n_images > 0 && n_segments > 0 && n_huff >= (int64_t)TSOD_JPEG_HUFF_TABLES * n_images, TSOD_ERR_INVALID_ARG);
    for (int i = 0; i < n_images; ++i) {
        const int rc = check_image(table_host[i], coef_count);
        if (rc != TSOD_OK) return rc;
    }
    int32_t image = -1;
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
    return TSOD_OK;
}

// The opening of both launch entries, `list` being the work list of the one and the chunk list of the other: the lengths,
// then - unless the list is empty, which is TSOD_OK and for the caller to return on - the pointers (`others`: the entry's
// further ones are there) and the records.  The entry checks its own list next and the alignment last.
int check_entry(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images, const tsod_jpeg_segment *segments_host,
                const tsod_jpeg_segment *segments, int32_t n_segments, const int32_t *list_host, const int32_t *list, int32_t n_list,
                const uint8_t *stream, int64_t stream_bytes, const tsod_jpeg_huff *huff, int64_t n_huff, int16_t *coef, int64_t coef_count,
                int32_t *status, int32_t subseq_words, bool others) {
    TSOD_REQUIRE(subseq_words >= 1 && subseq_words <= 64, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(n_images >= 0 && n_segments >= 0 && n_list >= 0 && stream_bytes >= 0 && n_huff >= 0 && coef_count >= 0, TSOD_ERR_INVALID_ARG);
    if (n_list == 0) return TSOD_OK;
    TSOD_REQUIRE(table_host && table && segments_host && segments && list_host && list && stream && huff && coef && status && others,
                 TSOD_ERR_INVALID_ARG);
    return check_batch(table_host, n_images, segments_host, n_segments, stream_bytes, n_huff, coef_count);
}

// The pointers both entries hand to the kernels
bool entry_aligned(const void *table, const void *segments, const void *list, const void *coef, const void *stream, const void *huff,
                   const void *status) {
    return aligned(table, 16) && aligned(segments, 16) && aligned(list, 16) && aligned(coef, 16) && aligned(stream, 4) && aligned(huff, 4) &&
           aligned(status, 4);
}

void launch_clear(int16_t *coef, int64_t coef_count, int32_t *status, int32_t n_images, tsod_stream_t stream_handle) {
    const long long n16 = coef_count / 8;
    const int n_tail = (int)(coef_count % 8);
    const unsigned clear_blocks = (unsigned)std::min<long long>(std::max<long long>(tsod_cdiv(n16, kThreads), 1), 2048);
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3(clear_blocks), dim3(kThreads), 0, tsod_stream(stream_handle),
                       reinterpret_cast<uint4 *>(coef), n16, coef + n16 * 8, n_tail, status, n_images);
}

// ---- the split mode: a segment's subsequences in chunks, one workgroup per chunk (jpeg_huffman_split.h) ----

struct SplitArgs {
    const tsod_jpeg_image *table;
    const tsod_jpeg_segment *segments;
    const int4 *work;                        // (segment, chunk, list index of the segment's chunk 0, the segment's chunks)
    const uint32_t *stream;
    const tsod_jpeg_huff *huff;
    SplitChunk *chunks;                      // the workspace: one record per list item ..
    SplitLane *lanes;                        // .. and chunk_subseqs records per list item
    int subseq_words, chunk_subseqs, overlap;
};

// What a workgroup knows of its segment once the code tables are in LDS
struct SplitSegment {
    HuffGeometry g;
    SegmentBits s;
    uint32_t sub_bits, n_sub;
    int32_t image;
    bool restart_follows;
};

__device__ SplitSegment split_open(const SplitArgs &a, int segment, uint32_t *lds_tables, int lane) {
    const tsod_jpeg_segment seg = a.segments[segment];
    const uint32_t bits = (uint32_t)seg.bit_length;
    SplitSegment sg;
    sg.g = huff_geometry(a.table[seg.image], seg);
    sg.s = SegmentBits{a.stream + seg.stream_offset / 4, (bits + 31u) / 32u, bits};
    sg.sub_bits = 32u * (uint32_t)a.subseq_words;
    sg.n_sub = split_subseqs(bits, sg.sub_bits);
    sg.image = seg.image;
    sg.restart_follows = (seg.flags & 1) != 0;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.huff + (long long)seg.image * TSOD_JPEG_HUFF_TABLES);
    for (int i = lane; i < kTableWords; i += kThreads) lds_tables[i] = src[i];
    __syncthreads();
    return sg;
}

// The bits of subsequence `sub` (< n_sub: no wrap), or nothing
__device__ void split_bits(const SplitSegment &sg, bool active, uint32_t sub, uint32_t &first_bit, uint32_t &limit) {
    first_bit = active ? sub * sg.sub_bits : 0u;
    limit = active ? min(first_bit + sg.sub_bits, sg.s.bits) : 0u;
}

// jpeg_huffman_kernel's fixpoint over the first n lanes of the workgroup: lane 0 keeps its start, every other lane takes its
// predecessor's end state when it differs from the start it used and is not ERROR, and decodes again; after pass k lanes
// 0 .. k are final, so at most n passes do work.  `changed` says which lanes decode in the first pass.
__device__ void split_fixpoint(const SplitSegment &sg, const tsod_jpeg_huff *tables, HuffState *lds_end, int lane, int n, uint32_t limit,
                               HuffState &start, HuffState &end, HuffTally &mine, bool changed) {
    const bool active = lane < n;
    int32_t unused = 0;
    for (int k = 0; k <= n; ++k) {
        if (changed) {
            mine = HuffTally{0u, {0u, 0u, 0u}};
            end = huff_run<false>(sg.s, tables, sg.g, start, limit, sg.sub_bits, sg.restart_follows, mine, nullptr, unused);
        }
        lds_end[lane] = end;
        __syncthreads();
        const HuffState before = lane == 0 ? start : lds_end[lane - 1];
        changed = active && before.p != kErrorP && !same(before, start);
        if (!__syncthreads_or(changed)) break;                   // (also: every read above precedes every write of the next pass)
        if (changed) start = before;
    }
}

// Inclusive Hillis-Steele scan of one uint4 per lane; the workgroup's sum in `total`.  lds_scan is free again on return.
__device__ uint4 split_scan(uint4 (*lds_scan)[kThreads], int lane, uint4 v, uint4 &total) {
    lds_scan[0][lane] = v;
    __syncthreads();
    int from = 0;
    for (int d = 1; d < kThreads; d <<= 1, from ^= 1) {
        uint4 x = lds_scan[from][lane];
        if (lane >= d) {
            const uint4 o = lds_scan[from][lane - d];
            x.x += o.x, x.y += o.y, x.z += o.z, x.w += o.w;
        }
        lds_scan[from ^ 1][lane] = x;
        __syncthreads();
    }
    const uint4 incl = lds_scan[from][lane];
    total = lds_scan[from][kThreads - 1];
    __syncthreads();
    return incl;
}

// The sum of the tallies of the lanes that call it, into lds_total (zeroed, and a barrier since)
__device__ void split_add(uint32_t *lds_total, const HuffTally &t) {
    atomicAdd(lds_total + 0, t.blocks), atomicAdd(lds_total + 1, t.dc[0]), atomicAdd(lds_total + 2, t.dc[1]), atomicAdd(lds_total + 3, t.dc[2]);
}

// sync, one workgroup per chunk: the chunk's lanes and up to `overlap` warm-up lanes before them from assumed states, the
// fixpoint among them, and the owned lanes' records.  Whether the chunk's entry is the true one is the stitch launch's to find.
__global__ void __launch_bounds__(kThreads) jpeg_split_sync_kernel(SplitArgs a) {
    __shared__ uint32_t lds_tables[kTableWords];
    __shared__ HuffState lds_end[kThreads];
    __shared__ uint32_t lds_total[4];
    const int lane = threadIdx.x;
    const int4 item = a.work[blockIdx.x];
    if (lane < 4) lds_total[lane] = 0u;
    const SplitSegment sg = split_open(a, item.x, lds_tables, lane);
    const tsod_jpeg_huff *tables = reinterpret_cast<const tsod_jpeg_huff *>(lds_tables);
    const SplitSpan sp = split_span(sg.n_sub, (uint32_t)item.y, (uint32_t)a.chunk_subseqs, (uint32_t)a.overlap);
    const bool active = (uint32_t)lane < sp.n_lanes;
    const uint32_t sub = sp.first + (uint32_t)lane;
    uint32_t first_bit, limit;
    split_bits(sg, active, sub, first_bit, limit);
    HuffState start = sub == 0u ? HuffState{0u, 0u} : assumed_state(first_bit), end = error_state();
    HuffTally mine = {0u, {0u, 0u, 0u}};
    split_fixpoint(sg, tables, lds_end, lane, (int)sp.n_lanes, limit, start, end, mine, active);
    const long long at = (long long)(item.z + item.y);
    SplitChunk &chunk = a.chunks[at];
    if (active && (uint32_t)lane >= sp.warm) {
        a.lanes[at * a.chunk_subseqs + (lane - (int)sp.warm)] = SplitLane{start, end, mine};
        split_add(lds_total, mine);
        if ((uint32_t)lane == sp.warm) chunk.entry = start;
        if ((uint32_t)lane == sp.n_lanes - 1u) chunk.exit = end;
    }
    __syncthreads();
    if (lane == 0) {
        chunk.total = HuffTally{lds_total[0], {lds_total[1], lds_total[2], lds_total[3]}};
        if (sp.n_lanes == 0u) chunk.entry = chunk.exit = HuffState{0u, 0u};
    }
}

// stitch, one workgroup per segment (the workgroups of the list's other items leave at once): chunk 0 is true; chunk c
// stands when the final exit of chunk c - 1 is the entry it used, and is repaired from that exit otherwise - the fixpoint
// over its own lanes from their stored states.  The boundaries are compared 256 at a time across the lanes, and only the
// first mismatch of a window is walked to.  Then the chunk totals are scanned into every chunk's base.
__global__ void __launch_bounds__(kThreads) jpeg_split_stitch_kernel(SplitArgs a, int32_t *__restrict__ status, int32_t *__restrict__ repaired) {
    __shared__ uint32_t lds_tables[kTableWords];
    __shared__ HuffState lds_end[kThreads];
    __shared__ uint4 lds_scan[2][kThreads];
    __shared__ uint32_t lds_total[4];
    __shared__ int lds_first;
    const int lane = threadIdx.x;
    const int4 item = a.work[blockIdx.x];
    if (item.y != 0) return;                                     // (the same in every lane)
    const SplitSegment sg = split_open(a, item.x, lds_tables, lane);
    const tsod_jpeg_huff *tables = reinterpret_cast<const tsod_jpeg_huff *>(lds_tables);
    SplitChunk *chunks = a.chunks + item.z;                      // the segment's own
    SplitLane *lanes = a.lanes + (long long)item.z * a.chunk_subseqs;
    const int n_chunks = item.w;
    int n_repaired = 0;
    for (int it = 0, cur = 1; it < n_chunks && cur < n_chunks; ++it) {      // every pass moves cur on by at least one
        const int c = cur + lane;
        const bool differs = c < n_chunks && !same(chunks[c - 1].exit, chunks[c].entry);
        if (lane == 0) lds_first = n_chunks;
        __syncthreads();
        if (differs) atomicMin(&lds_first, c);
        __syncthreads();
        const int first = lds_first;
        __syncthreads();
        if (first == n_chunks) {                                 // this window's chunks stand
            cur += kThreads;
            continue;
        }
        const HuffState t = chunks[first - 1].exit;              // final: every chunk before `first` stands or is repaired
        if (t.p == kErrorP) break;                               // a true error: nothing after it is looked at
        const SplitSpan sp = split_span(sg.n_sub, (uint32_t)first, (uint32_t)a.chunk_subseqs, 0u);
        const bool active = (uint32_t)lane < sp.n_lanes;
        SplitLane &rec = lanes[(long long)first * a.chunk_subseqs + (active ? lane : 0)];
        uint32_t first_bit, limit;
        split_bits(sg, active, sp.first + (uint32_t)lane, first_bit, limit);
        HuffState start = lane == 0 ? t : rec.start, end = rec.end;
        HuffTally mine = rec.tally;
        if (lane < 4) lds_total[lane] = 0u;
        split_fixpoint(sg, tables, lds_end, lane, (int)sp.n_lanes, limit, start, end, mine, lane == 0);
        if (active) {
            rec = SplitLane{start, end, mine};
            split_add(lds_total, mine);
            if ((uint32_t)lane == sp.n_lanes - 1u) chunks[first].exit = end;
        }
        __syncthreads();
        if (lane == 0) {
            chunks[first].entry = t;
            chunks[first].total = HuffTally{lds_total[0], {lds_total[1], lds_total[2], lds_total[3]}};
        }
        __syncthreads();                                         // the next window reads this chunk's exit
        ++n_repaired;
        cur = first + 1;
    }
    HuffTally carry = {0u, {0u, 0u, 0u}};
    for (int first = 0; first < n_chunks; first += kThreads) {
        const int c = first + lane;
        const HuffTally mine = c < n_chunks ? chunks[c].total : HuffTally{0u, {0u, 0u, 0u}};
        uint4 total;
        const uint4 incl = split_scan(lds_scan, lane, make_uint4(mine.blocks, mine.dc[0], mine.dc[1], mine.dc[2]), total);
        if (c < n_chunks)
            chunks[c].base = HuffTally{carry.blocks + incl.x - mine.blocks, {carry.dc[0] + incl.y - mine.dc[0],
                                                                             carry.dc[1] + incl.z - mine.dc[1], carry.dc[2] + incl.w - mine.dc[2]}};
        carry.blocks += total.x, carry.dc[0] += total.y, carry.dc[1] += total.z, carry.dc[2] += total.w;
    }
    if (lane == 0) {
        if (carry.blocks < sg.g.n_blocks) atomicOr(status + sg.image, kStatusBlocks);
        if (repaired) repaired[item.x] = n_repaired;
    }
}

// write, one workgroup per chunk: every owned lane's standing from the chunk's base and the lanes before it, then the
// coefficients from its final start
__global__ void __launch_bounds__(kThreads) jpeg_split_write_kernel(SplitArgs a, int16_t *__restrict__ coef, int32_t *__restrict__ status) {
    __shared__ uint32_t lds_tables[kTableWords];
    __shared__ uint4 lds_scan[2][kThreads];
    const int lane = threadIdx.x;
    const int4 item = a.work[blockIdx.x];
    const SplitSegment sg = split_open(a, item.x, lds_tables, lane);
    const tsod_jpeg_huff *tables = reinterpret_cast<const tsod_jpeg_huff *>(lds_tables);
    const SplitSpan sp = split_span(sg.n_sub, (uint32_t)item.y, (uint32_t)a.chunk_subseqs, 0u);
    const bool active = (uint32_t)lane < sp.n_lanes;
    const long long at = (long long)(item.z + item.y);
    const SplitLane rec = active ? a.lanes[at * a.chunk_subseqs + lane] : SplitLane{error_state(), error_state(), {0u, {0u, 0u, 0u}}};
    const HuffTally base = a.chunks[at].base, mine = rec.tally;
    uint32_t first_bit, limit;
    split_bits(sg, active, sp.first + (uint32_t)lane, first_bit, limit);
    uint4 total;
    const uint4 incl = split_scan(lds_scan, lane, make_uint4(mine.blocks, mine.dc[0], mine.dc[1], mine.dc[2]), total);
    if (!active) return;
    HuffTally standing = {base.blocks + incl.x - mine.blocks, {base.dc[0] + incl.y - mine.dc[0], base.dc[1] + incl.z - mine.dc[1],
                                                               base.dc[2] + incl.w - mine.dc[2]}};
    int32_t flags = 0;
    huff_run<true>(sg.s, tables, sg.g, rec.start, limit, sg.sub_bits, sg.restart_follows, standing, coef, flags);
    if (flags) atomicOr(status + sg.image, flags);
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
    const int rc = check_entry(table_host, table, n_images, segments_host, segments, n_segments, work_host, work, n_work, stream, stream_bytes,
                               huff, n_huff, coef, coef_count, status, subseq_words, true);
    if (rc != TSOD_OK || n_work == 0) return rc;
    for (int64_t k = 0; k < n_work; ++k) TSOD_REQUIRE(work_host[4 * k] >= 0 && work_host[4 * k] < n_segments, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(entry_aligned(table, segments, work, coef, stream, huff, status), TSOD_ERR_ALIGNMENT);
    launch_clear(coef, coef_count, status, n_images, stream_handle);
    hipLaunchKernelGGL(jpeg_huffman_kernel, dim3((unsigned)n_work), dim3(kThreads), 0, tsod_stream(stream_handle), table, segments,
                       reinterpret_cast<const int4 *>(work), reinterpret_cast<const uint32_t *>(stream), huff, coef, status,
                       (int)subseq_words);
    return tsod_launch_status();
}

extern "C" size_t tsod_jpeg_huffman_split_workspace_bytes(int64_t n_subseqs, int32_t n_chunks, int32_t n_segments) {
    if (n_subseqs < 0 || n_chunks < 0 || n_segments < 0) return 0;
    return (size_t)tsod_jpeg::split_workspace_bytes(n_subseqs, n_chunks, n_segments);
}

extern "C" int tsod_jpeg_huffman_split_i16(const tsod_jpeg_image *table_host, const tsod_jpeg_image *table, int32_t n_images,
                                           const tsod_jpeg_segment *segments_host, const tsod_jpeg_segment *segments, int32_t n_segments,
                                           const int32_t *chunks_host, const int32_t *chunks, int32_t n_chunks, const uint8_t *stream,
                                           int64_t stream_bytes, const tsod_jpeg_huff *huff, int64_t n_huff, int16_t *coef,
                                           int64_t coef_count, int32_t *status, int32_t subseq_words, int32_t chunk_subseqs,
                                           int32_t overlap, void *workspace, size_t workspace_bytes, int32_t *repaired,
                                           tsod_stream_t stream_handle) {
    // (the two lengths of its own first: they are refused with an empty list too, and with the same status as subseq_words)
    TSOD_REQUIRE(chunk_subseqs >= 1 && chunk_subseqs <= kSplitMaxChunk && overlap >= 0 && overlap <= kSplitMaxChunk - chunk_subseqs,
                 TSOD_ERR_INVALID_ARG);
    const int rc = check_entry(table_host, table, n_images, segments_host, segments, n_segments, chunks_host, chunks, n_chunks, stream,
                               stream_bytes, huff, n_huff, coef, coef_count, status, subseq_words, workspace != nullptr);
    if (rc != TSOD_OK || n_chunks == 0) return rc;
    // the chunk list: sorted by segment, every segment's chunks 0 .. count - 1 with the count its bit length implies
    int64_t at = 0, n_subseqs = 0;
    for (int k = 0; k < n_segments; ++k) {
        const uint32_t n_sub = split_subseqs((uint32_t)segments_host[k].bit_length, 32u * (uint32_t)subseq_words);
        const int64_t count = split_chunks(n_sub, (uint32_t)chunk_subseqs);
        TSOD_REQUIRE(count <= n_chunks - at, TSOD_ERR_INVALID_ARG);
        for (int64_t c = 0; c < count; ++c) {
            const int32_t *item = chunks_host + 4 * (at + c);
            TSOD_REQUIRE(item[0] == k && item[1] == c && item[2] == at && item[3] == count, TSOD_ERR_INVALID_ARG);
        }
        at += count, n_subseqs += n_sub;
    }
    TSOD_REQUIRE(at == n_chunks, TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(workspace_bytes >= (size_t)split_workspace_bytes(n_subseqs, n_chunks, n_segments), TSOD_ERR_INVALID_ARG);
    TSOD_REQUIRE(entry_aligned(table, segments, chunks, coef, stream, huff, status) && aligned(workspace, 16) && aligned(repaired, 4),
                 TSOD_ERR_ALIGNMENT);
    SplitChunk *records = static_cast<SplitChunk *>(workspace);
    const SplitArgs args = {table, segments, reinterpret_cast<const int4 *>(chunks), reinterpret_cast<const uint32_t *>(stream), huff,
                            records, reinterpret_cast<SplitLane *>(records + n_chunks), (int)subseq_words, (int)chunk_subseqs, (int)overlap};
    launch_clear(coef, coef_count, status, n_images, stream_handle);
    hipLaunchKernelGGL(jpeg_split_sync_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, tsod_stream(stream_handle), args);
    hipLaunchKernelGGL(jpeg_split_stitch_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, tsod_stream(stream_handle), args, status,
                       repaired);
    hipLaunchKernelGGL(jpeg_split_write_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, tsod_stream(stream_handle), args, coef, status);
    return tsod_launch_status();
}
