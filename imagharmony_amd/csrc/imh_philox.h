// The seeded step noise (include/imh.h, "seeded noise"): Philox4x32-10 as published (Salmon et al., Random123) and the four normals of one
// counter.  __host__ __device__ so that the same integer path runs in the kernels (elementwise.hip) and in imh_randn_seeded_host, which
// the CPU suite holds against the numpy restatement (imagharmony_amd/noise.py).  Plain C++ integer arithmetic, no inline assembly.
//   words   w0..w3 = philox4x32_10(counter = (e >> 2, row, stream, lane), key = (k0, k1))
//   uniform u_j = ((w_j >> 9) + 0.5) * 2^-23        exact in fp32, in [2^-24, 1 - 2^-24]: log(u) is finite and != 0 only where it should be
//   normals (z0, z1) = sqrt(-2 ln u0) * (cos, sin)(2 pi u1), (z2, z3) likewise from (u2, u3)                       |z| <= 5.77
// The device path uses the accurate logf / sqrtf / sincospif (not the __sinf family): a few fp32 ulps against the float64 restatement.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IMH_HD __host__ __device__ __forceinline__
#else
#define IMH_HD inline
#endif

namespace imh {

struct PhiloxWords { uint32_t w[4]; };
struct PhiloxNormals { float z[4]; };

IMH_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

IMH_HD PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = philox_mulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = philox_mulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    PhiloxWords o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// the words of quad `quad` (= element index >> 2 inside the sample) of the sample whose seed row is (k0, k1, lane, .)
IMH_HD PhiloxWords seeded_words(const uint32_t* seed_row, uint32_t quad, uint32_t row, uint32_t stream) {
    return philox4x32_10(quad, row, stream, seed_row[2], seed_row[0], seed_row[1]);
}

IMH_HD float philox_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }      // 2^-23; every step exact

IMH_HD void box_muller(float u0, float u1, float* z0, float* z1) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float rho = sqrtf(-2.0f * logf(u0));
    float s, c;
    sincospif(2.0f * u1, &s, &c);
    *z0 = rho * c;
    *z1 = rho * s;
#else
    // the host has no sincospi: float64 throughout, rounded once (within an fp32 ulp of the specification)
    const double rho = sqrt(-2.0 * log((double)u0)), a = 6.283185307179586476925286766559 * (double)u1;
    *z0 = (float)(rho * cos(a));
    *z1 = (float)(rho * sin(a));
#endif
}

IMH_HD PhiloxNormals seeded_normals(const uint32_t* seed_row, uint32_t quad, uint32_t row, uint32_t stream) {
    const PhiloxWords w = seeded_words(seed_row, quad, row, stream);
    PhiloxNormals n;
    box_muller(philox_uniform(w.w[0]), philox_uniform(w.w[1]), &n.z[0], &n.z[1]);
    box_muller(philox_uniform(w.w[2]), philox_uniform(w.w[3]), &n.z[2], &n.z[3]);
    return n;
}

}  // namespace imh
