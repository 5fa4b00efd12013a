// The counter-based generator of include/rmbx.h (rmbx_philox_normal), shared by every translation unit
// that draws from it, so that an element of (seed, episode, draw, plane, i) is the same bits wherever
// it is computed: the sampler noise (rmbx_philox.hip) and the observation perturbation
// (rmbx_perturb.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rmbx {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// Philox4x32-10 (Random123): ten rounds, the key bumped by the Weyl constants between rounds.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, c.x), lo0 = kPhiloxM0 * c.x;
    const uint32_t hi1 = __umulhi(kPhiloxM1, c.z), lo1 = kPhiloxM1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return c;
}

// One word -> one uniform: u = ((w >> 9) + 0.5) * 2^-23 is exact in f32 and inside (0, 1).
__device__ __forceinline__ float philox_uniform(uint32_t w) {
#pragma clang fp contract(off)
  return ((float)(w >> 9) + 0.5f) * 0x1p-23f;
}

// Two words -> two standard normals.  u = ((w >> 9) + 0.5) * 2^-23 is exact in f32 and inside
// (0, 1); 2 * u2 is exact too, so sincospif sees the exact angle in half turns.
__device__ __forceinline__ float2 box_muller(uint32_t wa, uint32_t wb) {
#pragma clang fp contract(off)
  const float u1 = ((float)(wa >> 9) + 0.5f) * 0x1p-23f;
  const float u2x2 = ((float)(wb >> 9) + 0.5f) * 0x1p-22f;
  const float r = sqrtf(-2.f * logf(u1));
  float s, c;
  sincospif(u2x2, &s, &c);
  return make_float2(r * c, r * s);
}

}  // namespace rmbx
