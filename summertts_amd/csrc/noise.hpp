// noise.hpp -- the sampling noise of VITS inference: a counter-based Philox4x64-10 generator (Salmon, Moraes, Dror, Shaw, "Parallel
// random numbers: as easy as 1, 2, 3", SC'11) and the Box-Muller conversion of one 64-bit word to a standard normal.
//
// Element j of a noise stream of utterance u is a pure function of (seed_u, stream, j): Philox block j / 4 under key (seed_u, 0) and
// counter (j / 4, stream, 0, 0), output word j % 4.  No state is carried between launches, utterances or calls, so the numbers do not
// depend on launch geometry, batching, sharding or a repeated run.  j follows the column-major fill order of the reference's
// rand_gen(rows, cols): the SDP latent rand_gen(2, T) has j = t * 2 + ch, the prior rand_gen(F, C) has j = c * F + f.
// numpy.random.Philox(key=[seed, 0], counter=[j / 4 - 1, stream, 0, 0]).random_raw(4) yields the same block (numpy increments the
// counter before each block).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sts {

constexpr int kNoiseStreamSdp = 0;     // the stochastic duration predictor's latent
constexpr int kNoiseStreamPrior = 1;   // the prior sample z_p

struct Philox4 { uint64_t w[4]; };

__host__ __device__ inline void philox_mulhilo(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
    lo = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    hi = __umul64hi(a, b);
#else
    hi = (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// Philox4x64-10 of counter (c0, c1, 0, 0) under key (k0, 0)
__host__ __device__ inline Philox4 philox4x64_10(uint64_t c0, uint64_t c1, uint64_t k0) {
    uint64_t x0 = c0, x1 = c1, x2 = 0, x3 = 0, key0 = k0, key1 = 0;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint64_t hi0, lo0, hi1, lo1;
        philox_mulhilo(0xD2E7470EE14C6C93ull, x0, hi0, lo0);
        philox_mulhilo(0xCA5A826395121157ull, x2, hi1, lo1);
        x0 = hi1 ^ x1 ^ key0; x1 = lo1; x2 = hi0 ^ x3 ^ key1; x3 = lo0;
        key0 += 0x9E3779B97F4A7C15ull; key1 += 0xBB67AE8584CAA73Bull;
    }
    return Philox4{{x0, x1, x2, x3}};
}

// Box-Muller, cosine branch: u1 in (0, 1] from the top 24 bits, u2 in [0, 1) from the next 24; full-precision fp32 math
__device__ inline float philox_normal(uint64_t w) {
    const float u1 = (float)((w >> 40) + 1ull) * 5.9604644775390625e-8f;          // 2^-24
    const float u2 = (float)((w >> 16) & 0xFFFFFFull) * 5.9604644775390625e-8f;
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// element j of stream `stream` under seed `seed`
__device__ inline float noise_normal(uint64_t seed, int stream, uint64_t j) {
    const Philox4 p = philox4x64_10(j >> 2, (uint64_t)stream, seed);
    const int q = (int)(j & 3);
    return philox_normal(q == 0 ? p.w[0] : q == 1 ? p.w[1] : q == 2 ? p.w[2] : p.w[3]);
}

}  // namespace sts
