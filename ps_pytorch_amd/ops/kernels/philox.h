// Philox4x32-10 (Salmon et al., SC'11), shared by the counter-based RNG
// kernels (dropout.hip, augment.hip). The CPU oracle is philox4x32_10 in
// ops/functional.py; both are pure integer arithmetic and agree bit for bit.
#pragma once
#include "common.h"

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

__host__ __device__ __forceinline__ void philox4x32_10(
    unsigned c0, unsigned c1, unsigned c2, unsigned c3,
    unsigned k0, unsigned k1, unsigned out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        unsigned long long p0 = (unsigned long long)PHILOX_M0 * c0;
        unsigned long long p1 = (unsigned long long)PHILOX_M1 * c2;
        unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
