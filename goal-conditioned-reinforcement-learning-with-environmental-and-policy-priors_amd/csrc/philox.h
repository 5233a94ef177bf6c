// philox.h -- Philox4x32-10, written once: the engine's draws (twoarmy_engine.hip), the action sampler and hindsight
// relabelling (ppo_kernels.hip) are bit-exact against oracle/philox.py only while they share this one routine.
#ifndef TWOARMY_PHILOX_H
#define TWOARMY_PHILOX_H
#include <hip/hip_runtime.h>
#include <stdint.h>

static __device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t &c0, uint32_t &c1,
                                                     uint32_t &c2, uint32_t &c3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
#endif  // TWOARMY_PHILOX_H
