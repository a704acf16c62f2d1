// jpeg_huffman_split.h -- the arithmetic of the split mode of the device Huffman pass ("split over
// workgroups"): how a segment's subsequences fall into chunks, which lanes a chunk's workgroup runs, and the records of the
// workspace.  Shared by csrc/jpeg_huffman.hip (the three kernels and the host checks of tsod_jpeg_huffman_split_i16) and the
// stand-alone CPU program tests/jpeg_huffman_split_main.cpp.  Plain C++ on top of jpeg_huffman_core.h, which does the per-lane
// work unchanged.
#pragma once
#include "jpeg_huffman_core.h"

namespace tsod_jpeg {

constexpr int kSplitMaxChunk = kHuffLanes;   // chunk_subseqs + overlap <= 256: a chunk with its warm-up is one workgroup

// What the sync launch leaves of every owned subsequence and the stitch launch may replace: the start the lane ended up
// with, the end state from there and the tally of kWrite == false
struct alignas(16) SplitLane {
    HuffState start, end;
    HuffTally tally;
};

// One chunk: the start of its first owned lane, the end of its last one, the sum of its lanes' tallies, and - from the stitch
// launch - the sum of the chunks before it in the segment
struct alignas(16) SplitChunk {
    HuffState entry, exit;
    HuffTally total, base;
};

TSOD_HD uint32_t split_subseqs(uint32_t bits, uint32_t sub_bits) { return bits / sub_bits + (bits % sub_bits ? 1u : 0u); }

TSOD_HD uint32_t split_chunks(uint32_t n_sub, uint32_t chunk_subseqs) {
    const uint32_t n = n_sub / chunk_subseqs + (n_sub % chunk_subseqs ? 1u : 0u);
    return n ? n : 1u;                       // a segment without bits is one chunk without lanes
}

// The lanes of chunk c's workgroup: subsequences [first, first + n_lanes) of the segment, of which the first `warm` belong
// to chunk c - 1 and only bring the parse into step.  overlap == 0 gives the owned lanes alone.  c < split_chunks(n_sub, ..).
struct SplitSpan {
    uint32_t first, warm, n_lanes;
};
TSOD_HD SplitSpan split_span(uint32_t n_sub, uint32_t c, uint32_t chunk_subseqs, uint32_t overlap) {
    const uint32_t owned_first = c * chunk_subseqs;
    const uint32_t owned_end = n_sub - owned_first < chunk_subseqs ? n_sub : owned_first + chunk_subseqs;
    SplitSpan sp;
    sp.warm = overlap < owned_first ? overlap : owned_first;
    sp.first = owned_first - sp.warm;
    sp.n_lanes = n_sub ? owned_end - sp.first : 0u;
    return sp;
}

// The workspace: n_chunks SplitChunk records in list order, then chunk_subseqs SplitLane records for every chunk of the list.
// A segment of n subsequences has at most n + chunk_subseqs lane records, so the size is stated without chunk_subseqs.
TSOD_HD int64_t split_workspace_bytes(int64_t n_subseqs, int64_t n_chunks, int64_t n_segments) {
    return (int64_t)sizeof(SplitChunk) * n_chunks + (int64_t)sizeof(SplitLane) * (n_subseqs + (int64_t)kSplitMaxChunk * n_segments);
}

}  // namespace tsod_jpeg
