// philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the library's
// counter-based random word source.  Plain C++: the same function on the host and in a kernel, so
// tests/dropout_restated.py's NumPy restatement, tsod_philox4x32_host and the dropout kernel give the same bits.
//   (c0, c1, c2, c3), (k0, k1) -> four 32-bit words; ten rounds of
//       hi0:lo0 = 0xD2511F53 * c0     hi1:lo1 = 0xCD9E8D57 * c2     c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
//   with the key bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TSOD_PHILOX_FN __host__ __device__ inline
#else
#define TSOD_PHILOX_FN inline
#endif

struct tsod_philox_words {
    uint32_t v[4];
};

TSOD_PHILOX_FN tsod_philox_words tsod_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        if (round > 0) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;       // (one v_mul_hi_u32 + one v_mul_lo_u32 each)
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    tsod_philox_words out;
    out.v[0] = c0;
    out.v[1] = c1;
    out.v[2] = c2;
    out.v[3] = c3;
    return out;
}
