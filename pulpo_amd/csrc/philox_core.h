// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the noise of the augmentation operators
// (augment.hip): a pure function of (seed, element index), independent of the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pulpo {

struct Philox4 {
    uint32_t r[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Philox4 out;
    out.r[0] = c0; out.r[1] = c1; out.r[2] = c2; out.r[3] = c3;
    return out;
}

// the four words of group g = i >> 2 of element index i under a 64-bit seed
__device__ __forceinline__ Philox4 philox_group(uint64_t g, uint32_t seed_lo, uint32_t seed_hi) {
    return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, seed_lo, seed_hi);
}

// standard normal of lane (i & 3) of a group: Box-Muller on the word pair (r0, r1) for lanes 0 and 1, (r2, r3) for lanes 2 and 3;
// u1 = ((ra >> 8) + 1) 2^-24 in (0, 1], u2 = (rb >> 8) 2^-24 in [0, 1); even lanes take the cosine, odd lanes the sine
__device__ __forceinline__ float philox_normal(const Philox4& w, int lane) {
    const uint32_t ra = (lane & 2) ? w.r[2] : w.r[0], rb = (lane & 2) ? w.r[3] : w.r[1];      // (selects: no indexed register array)
    const float u1 = (float)((ra >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)(rb >> 8) * 5.9604644775390625e-8f;
    const float R = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincospif(2.f * u2, &sn, &cs);                                // cos / sin (2 pi u2), the argument 2 u2 exact
    return R * ((lane & 1) ? sn : cs);
}

}  // namespace pulpo
