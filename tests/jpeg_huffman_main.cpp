// A stand-alone CPU run of the device Huffman pass for sanitizer builds and for gdb (tests/test_jpeg_scan_abi.py):
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/jpeg_huffman_main.cpp -o jpeg_huffman_main
//   ./jpeg_huffman_main 1,2,3,32 file ...
// It uses only csrc/jpeg_scan.h and csrc/jpeg_huffman_core.h (and, as the oracle, csrc/jpeg_entropy.h's decode).  For every
// file and every subseq_words of the first argument it runs the kernel's algorithm lane by lane - the same huff_run, the same
// Jacobi fixpoint over 256 lanes with its bound of 256 iterations, the same scan and write pass - on malloc'd buffers of
// exactly the sizes the records state, so a read or write one byte outside is caught.  One line per file:
//   <host status> <prepare status> then per subseq_words: <device status word> <1: coefficients equal the host's, 0: not, -: n/a>
//   <most fixpoint iterations of a round> <median over the rounds>
// Exits 1 when a device status is 0 where the host pass refuses (or the reverse), or coefficients differ where both accept;
// 2 for a file it cannot read or arguments it cannot use; 0 otherwise, whatever the statuses are.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../two_stage_object_detection_amd/csrc/jpeg_huffman_core.h"
#include "../two_stage_object_detection_amd/csrc/jpeg_scan.h"

using namespace tsod_jpeg;

// jpeg_huffman_kernel for one segment, the lanes one after the other
static int32_t run_segment(const tsod_jpeg_image &im, const tsod_jpeg_segment &seg, const uint8_t *stream, const tsod_jpeg_huff *tables,
                           int16_t *coef, int subseq_words, std::vector<int> &iterations) {
    const HuffGeometry g = huff_geometry(im, seg);
    const uint32_t bits = (uint32_t)seg.bit_length;
    const SegmentBits s = {reinterpret_cast<const uint32_t *>(stream + seg.stream_offset), (bits + 31u) / 32u, bits};
    const bool restart_follows = (seg.flags & 1) != 0;
    const uint32_t sub_bits = 32u * (uint32_t)subseq_words, round_bits = sub_bits * kHuffLanes;
    const uint32_t n_rounds = bits / round_bits + (bits % round_bits ? 1u : 0u);
    HuffState carry_state = {0u, 0u};
    HuffTally carry = {0u, {0u, 0u, 0u}};
    int32_t flags = 0, unused = 0;
    HuffState start[kHuffLanes], end[kHuffLanes], before[kHuffLanes];
    HuffTally mine[kHuffLanes];
    uint32_t limit[kHuffLanes];
    for (uint32_t r = 0; r < n_rounds; ++r) {
        for (int lane = 0; lane < kHuffLanes; ++lane) {
            const uint32_t first_bit = r * round_bits + (uint32_t)lane * sub_bits;
            limit[lane] = std::min(first_bit + sub_bits, bits);
            start[lane] = lane == 0 ? carry_state : assumed_state(first_bit);
            mine[lane] = HuffTally{0u, {0u, 0u, 0u}};
            end[lane] = huff_run<false>(s, tables, g, start[lane], limit[lane], sub_bits, restart_follows, mine[lane], nullptr, unused);
        }
        const int last_active = (int)std::min((bits - 1u - r * round_bits) / sub_bits, (uint32_t)(kHuffLanes - 1));
        int k = 0;
        for (; k < kHuffLanes; ++k) {
            bool any = false;
            for (int lane = 0; lane < kHuffLanes; ++lane) {       // every lane reads before any lane writes
                before[lane] = lane == 0 || lane > last_active || end[lane - 1].p == kErrorP ? start[lane] : end[lane - 1];
                any = any || !same(before[lane], start[lane]);
            }
            if (!any) break;
            for (int lane = 0; lane < kHuffLanes; ++lane)
                if (!same(before[lane], start[lane])) {
                    start[lane] = before[lane];
                    mine[lane] = HuffTally{0u, {0u, 0u, 0u}};
                    end[lane] = huff_run<false>(s, tables, g, start[lane], limit[lane], sub_bits, restart_follows, mine[lane], nullptr, unused);
                }
        }
        iterations.push_back(k);
        HuffTally at = carry;
        for (int lane = 0; lane < kHuffLanes; ++lane) {
            HuffTally t = at;
            huff_run<true>(s, tables, g, start[lane], limit[lane], sub_bits, restart_follows, t, coef, flags);
            at.blocks += mine[lane].blocks;
            for (int c = 0; c < 3; ++c) at.dc[c] += mine[lane].dc[c];
        }
        carry = at;
        carry_state = end[last_active];
    }
    if (carry.blocks < g.n_blocks) flags |= kStatusBlocks;
    return flags;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<int> words;
    for (const char *p = argv[1]; *p;) {
        char *e;
        const long v = strtol(p, &e, 10);
        if (e == p || v < 1 || v > 64) return 2;
        words.push_back((int)v);
        p = *e == ',' ? e + 1 : e;
    }
    int bad = 0;
    for (int a = 2; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *data = (uint8_t *)malloc(size > 0 ? (size_t)size : 1);
        if (!data || (size > 0 && fread(data, 1, (size_t)size, f) != (size_t)size)) return 2;
        fclose(f);
        State st;
        int host = parse(data, (size_t)size, st), prepare = host;
        if (host != TSOD_OK) {
            printf("%d %d\n", host, prepare);
            free(data);
            continue;
        }
        const tsod_jpeg_info info = st.info;
        const size_t count = (size_t)info.coef_total;
        int16_t *want = (int16_t *)malloc(count * sizeof(int16_t));
        if (!want) return 2;
        host = decode(data, (size_t)size, want, count, st);
        int64_t cap_bytes = 0, stream_bytes = 0;
        int32_t cap_segs = 0, n_segs = 0;
        if (scan_sizes(info, (size_t)size, &cap_bytes, &cap_segs) != TSOD_OK) return 2;
        uint8_t *wide = (uint8_t *)malloc((size_t)cap_bytes);
        tsod_jpeg_segment *wide_segs = (tsod_jpeg_segment *)malloc(sizeof(tsod_jpeg_segment) * (size_t)cap_segs);
        tsod_jpeg_huff *tables = (tsod_jpeg_huff *)malloc(sizeof(tsod_jpeg_huff) * TSOD_JPEG_HUFF_TABLES);
        if (!wide || !wide_segs || !tables) return 2;
        prepare = scan_prepare(data, (size_t)size, wide, cap_bytes, &stream_bytes, wide_segs, cap_segs, &n_segs, tables, st);
        printf("%d %d", host, prepare);
        if (prepare != TSOD_OK) {
            if (host == TSOD_OK) bad = 1;                        // the sweep refuses only what the host pass refuses
        } else {
            uint8_t *stream = (uint8_t *)malloc(stream_bytes > 0 ? (size_t)stream_bytes : 1);   // exact sizes from here on
            tsod_jpeg_segment *segs = (tsod_jpeg_segment *)malloc(sizeof(tsod_jpeg_segment) * (size_t)n_segs);
            int16_t *coef = (int16_t *)malloc(count * sizeof(int16_t));
            if (!stream || !segs || !coef) return 2;
            memcpy(stream, wide, (size_t)stream_bytes);
            memcpy(segs, wide_segs, sizeof(tsod_jpeg_segment) * (size_t)n_segs);
            tsod_jpeg_image im;
            memset(&im, 0, sizeof(im));
            im.H = info.H, im.W = info.W, im.n_comp = info.n_comp, im.hs = info.hmax, im.vs = info.vmax;
            int64_t at = 0;
            for (int c = 0; c < info.n_comp; ++c) {
                im.blocks_w[c] = info.blocks_w[c], im.blocks_h[c] = info.blocks_h[c];
                im.coef_offset[c] = at;
                at += info.coef_count[c];
            }
            for (int w : words) {
                memset(coef, 0, count * sizeof(int16_t));
                std::vector<int> iterations;
                int32_t status = 0;
                for (int k = 0; k < n_segs; ++k) status |= run_segment(im, segs[k], stream, tables, coef, w, iterations);
                const bool equal = memcmp(coef, want, count * sizeof(int16_t)) == 0;
                std::sort(iterations.begin(), iterations.end());
                const int most = iterations.empty() ? 0 : iterations.back();
                const int median = iterations.empty() ? 0 : iterations[iterations.size() / 2];
                if (status == 0 && host == TSOD_OK)
                    printf(" %d %d %d %d", status, (int)equal, most, median);
                else
                    printf(" %d - %d %d", status, most, median);
                if ((status == 0) != (host == TSOD_OK) || (status == 0 && !equal)) bad = 1;
            }
            free(stream), free(segs), free(coef);
        }
        printf("\n");
        free(wide), free(wide_segs), free(tables), free(want), free(data);
    }
    return bad;
}
