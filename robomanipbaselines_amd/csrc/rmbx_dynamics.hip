// Per-episode scale factors of the world's physical constants (the rule: include/rmbx.h,
// rmbx_dynamics_draw): contact friction, object joint damping, object mass and servo gain, each
// 1 + S * (2 u - 1) from one Philox block of rmbx_philox.h keyed by (seed, episode) on a plane of
// its own.  The engine reads the rows through rmbx_engine_bind_dynamics (rmbx_engine.hip).
//
// One thread per row: it computes the row's single Philox block and writes the row's four f64 (n is
// the number of env slots: the launch, not the arithmetic, is the cost).  No LDS, no atomics, no
// barriers (the range guard returns).

#include "rmbx_common.h"
#include "rmbx_philox.h"

#include <cmath>
#include <cstdint>

namespace rmbx {
namespace {

struct DynamicsArgs {
  double* scale;
  const int32_t* episode;
  const uint8_t* active;
  float S[4];
  uint32_t k0, k1;
  uint32_t n;
};

__device__ __forceinline__ double dynamics_scale(float S, uint32_t w) {
#pragma clang fp contract(off)
  if (S == 0.f) return 1.0;
  const float s = 2.f * philox_uniform(w) - 1.f;
  return 1.0 + (double)S * (double)s;
}

__global__ void __launch_bounds__(256) dynamics_draw_kernel(DynamicsArgs a) {
  const uint32_t row = blockIdx.x * 256u + threadIdx.x;
  if (row >= a.n) return;
  if (a.active && !a.active[row]) return;
  const uint32_t ep = (uint32_t)a.episode[row];
  const uint4 w = philox4x32_10(make_uint4(0u, (uint32_t)RMBX_DYNAMICS_PLANE, 0u, ep), a.k0, a.k1);
  double* const out = a.scale + 4 * (size_t)row;
  out[0] = dynamics_scale(a.S[0], w.x);
  out[1] = dynamics_scale(a.S[1], w.y);
  out[2] = dynamics_scale(a.S[2], w.z);
  out[3] = dynamics_scale(a.S[3], w.w);
}

}  // namespace
}  // namespace rmbx

extern "C" int rmbx_dynamics_draw(uint64_t seed, const int32_t* episode, const rmbx_dynamics_params* p, double* scale,
                                  const uint8_t* active, int n, void* stream) {
  RMBX_CHECK_ARG(episode && p && scale, "rmbx_dynamics_draw: NULL pointer");
  RMBX_CHECK_ARG(n >= 1, "rmbx_dynamics_draw: n=%d must be at least 1", n);
  const float S[4] = {p->friction, p->damping, p->mass, p->gain};
  for (int k = 0; k < 4; k++)
    RMBX_CHECK_ARG(S[k] >= 0.f && S[k] < 1.f, "rmbx_dynamics_draw: strength %d outside [0, 1)", k);
  RMBX_CHECK_ARG(((uintptr_t)scale & 7u) == 0, "rmbx_dynamics_draw: scale is not 8-byte aligned");
  RMBX_CHECK_ARG(((uintptr_t)episode & 3u) == 0, "rmbx_dynamics_draw: episode is not 4-byte aligned");

  rmbx::DynamicsArgs a;
  a.scale = scale, a.episode = episode, a.active = active;
  for (int k = 0; k < 4; k++) a.S[k] = S[k];
  a.k0 = (uint32_t)(seed & 0xffffffffull), a.k1 = (uint32_t)(seed >> 32);
  a.n = (uint32_t)n;
  hipLaunchKernelGGL(rmbx::dynamics_draw_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}
