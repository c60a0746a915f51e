// sbe_philox.hip.h -- the counter-based random numbers every unit draws from: Philox4x32-10 and the 53-bit uniform read from
// it.  Nothing else: the engine's sampling kernels (sbe_kernels_sampling.hip.h) and the model comparison's bootstrap
// (sbe_compare.hip) both include this file, so neither drags in the other's kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sbe {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter-based,
// so uniform i of draw d under seed k is a pure function philox((i, d), k) -- no RNG state in HBM, any
// grid shape gives the same numbers.  oracle/sbayes_oracle.py restates it (and its known-answer vectors).
__device__ __host__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t* out) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 53-bit uniform in [0, 1) from two words, like MT19937's genrand_res53 that np.random.random uses.
__device__ inline double philox_uniform(uint64_t seed, uint64_t draw, uint64_t i) {
    uint32_t r[4];
    philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    return ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6)) * (1.0 / 9007199254740992.0);
}

}  // namespace sbe
