// Counter-based Philox4x32-10 (Salmon et al. 2011), key = seed, counter = (location, sweep): the one
// generator of every per-location draw (the w sweep's normals, gibbs.hip; the Polya-Gamma draws,
// polya_gamma.h).  __host__ __device__, and plain C++ on a host compiler, so a CPU check program draws the
// same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NNGP_PHILOX_HD __host__ __device__ __forceinline__
#else
#define NNGP_PHILOX_HD static inline
#endif

namespace nngp {

NNGP_PHILOX_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c[0];
        const uint64_t p1 = (uint64_t)M1 * c[2];
        const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0;
        const uint32_t h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
        const uint32_t n0 = h1 ^ c[1] ^ k0, n2 = h0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = l1;
        c[2] = n2;
        c[3] = l0;
        k0 += W0;
        k1 += W1;
    }
}

// the two 53-bit uniforms in (0, 1) of the block (seed, location, sweep)
NNGP_PHILOX_HD void philox_uniform2(uint64_t seed, uint64_t loc, uint64_t sweep, double* u1, double* u2) {
    uint32_t c[4] = {(uint32_t)loc, (uint32_t)(loc >> 32), (uint32_t)sweep, (uint32_t)(sweep >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t a = ((uint64_t)c[0] << 21) ^ (c[1] >> 11);
    const uint64_t b = ((uint64_t)c[2] << 21) ^ (c[3] >> 11);
    *u1 = ((double)(a & ((1ull << 53) - 1)) + 0.5) * 0x1p-53;
    *u2 = ((double)(b & ((1ull << 53) - 1)) + 0.5) * 0x1p-53;
}

// standard normal for (seed, location, sweep): Box-Muller on two 53-bit uniforms in (0, 1)
NNGP_PHILOX_HD double philox_normal(uint64_t seed, uint64_t loc, uint64_t sweep) {
    uint32_t c[4] = {(uint32_t)loc, (uint32_t)(loc >> 32), (uint32_t)sweep, (uint32_t)(sweep >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t a = ((uint64_t)c[0] << 21) ^ (c[1] >> 11);
    const uint64_t b = ((uint64_t)c[2] << 21) ^ (c[3] >> 11);
    const double u1 = ((double)(a & ((1ull << 53) - 1)) + 0.5) * 0x1p-53;
    const double u2 = ((double)(b & ((1ull << 53) - 1)) + 0.5) * 0x1p-53;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

}  // namespace nngp
