// Philox4x32-10 and the Box-Muller draw of the library's random streams. One definition for every kernel that draws
// from them, so that two kernels drawing the same (seed, counter) get the same bits; the host twin serves the host-only reference
// functions (the integer part is exact on both sides, the Box-Muller transcendentals agree to rounding).
// Stream ids (second counter word): 0 payload bytes, 1 baseband noise, 2 static echo phase, 3 passband noise, 4 HF channel draws,
// 5 streaming HF channel noise, 6 link simulator schedule, 7 link simulator payloads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace {

__host__ __device__ __forceinline__ uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umulhi(a, b);
#else
    return uint32_t((uint64_t(a) * uint64_t(b)) >> 32);
#endif
}

__host__ __device__ inline void philox4x32(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2_, uint32_t c3, uint32_t out[4]) {
    uint32_t k0 = uint32_t(seed), k1 = uint32_t(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = philox_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = philox_mulhi(0xCD9E8D57u, c2_), l1 = 0xCD9E8D57u * c2_;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2_ = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2_; out[3] = c3;
}

__host__ __device__ __forceinline__ double gauss_bm(uint32_t a, uint32_t b) {
    const double u1 = (double(a) + 1.0) * (1.0 / 4294967296.0);
    const double u2 = double(b) * (1.0 / 4294967296.0);
    return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}

}  // namespace
