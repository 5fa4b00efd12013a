// Per-episode perturbation of the command the robot executes (the rule: include/rmbx.h,
// rmbx_action_perturb): episode-constant bias and per-inference noise on the policy's denormalised
// action, a delay line of D env-steps and a lossy link, all from the Philox rule of rmbx_philox.h
// keyed by (seed, episode, draw, plane).  It sits between the policy and rmbx_motion_command: it
// writes the action that arrives at this step and the mask of the rows it arrives for.
//
// One thread per (row, k) of the n * A action elements (n * A <= 8192 at the benchmark's shapes: the
// launch, not the arithmetic, is the cost).  Each thread computes the Philox blocks its element needs
// (bias and noise: block k / 4; hold: block 0 of its row), so nothing is exchanged between lanes and
// a row may straddle waves; the hold decision and the validity r >= D are a row's, every thread of
// the row computes the same value and the thread of k = 0 stores the mask.  A thread of row x writes
// ring entry r % (D + 1) and reads (r + 1) % (D + 1), which only launches before this one wrote:
// no ordering inside a launch is needed.  No LDS, no atomics, no barriers (the range guard returns).

#include "rmbx_common.h"
#include "rmbx_philox.h"

#include <cmath>
#include <cstdint>

namespace rmbx {
namespace {

struct ActuationArgs {
  const double* action;
  double* out;
  uint8_t* mask_out;
  double* ring;
  const double* bias_scale;
  const double* noise_scale;
  float S, B, P;
  uint32_t D, skip;
  uint32_t k0, k1;
  const int32_t* episode;
  const int32_t* r;
  const uint8_t* mask_in;
  uint32_t n, A;
};

// word t (0..3) of a block
__device__ __forceinline__ uint32_t word_of(const uint4& w, uint32_t t) {
  return t == 0u ? w.x : t == 1u ? w.y : t == 2u ? w.z : w.w;
}

__global__ void __launch_bounds__(256) action_perturb_kernel(ActuationArgs a) {
#pragma clang fp contract(off)
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= a.n * a.A) return;
  const uint32_t row = idx / a.A, k = idx - row * a.A;
  const int32_t rs = a.r[row];
  // a row is active with its mask set and a rollout step to speak of (r >= 0 keeps the ring index
  // inside the ring whatever the caller's r holds)
  const bool active = (!a.mask_in || a.mask_in[row]) && rs >= 0;
  if (!active) {
    if (k == 0u) a.mask_out[row] = 0;
    return;
  }
  const uint32_t r = (uint32_t)rs, ep = (uint32_t)a.episode[row];
  const uint32_t j = k >> 2, t = k & 3u;
  double v = a.action[idx];
  if (a.B != 0.f) {
    const uint4 w = philox4x32_10(make_uint4(j, (uint32_t)RMBX_ACTUATION_PLANE_BIAS, 0u, ep), a.k0, a.k1);
    const float s = 2.f * philox_uniform(word_of(w, t)) - 1.f;
    v = v + a.bias_scale[k] * (double)s;
  }
  if (a.S != 0.f) {
    const uint32_t draw = r - r % a.skip;
    const uint4 w = philox4x32_10(make_uint4(j, (uint32_t)RMBX_ACTUATION_PLANE_NOISE, draw, ep), a.k0, a.k1);
    const float2 z = t < 2u ? box_muller(w.x, w.y) : box_muller(w.z, w.w);
    v = v + a.noise_scale[k] * (double)((t & 1u) ? z.y : z.x);
  }
  double arrived = v;
  if (a.D != 0u) {
    const uint32_t len = a.D + 1u;
    double* const ring = a.ring + ((size_t)row * len) * a.A + k;
    ring[(size_t)(r % len) * a.A] = v;
    arrived = ring[(size_t)((r + 1u) % len) * a.A];  // written at r - D; garbage while r < D: masked below
  } else {
    a.ring[(size_t)row * a.A + k] = v;
  }
  bool arrives = r >= a.D;
  if (a.P != 0.f) {
    const uint4 w = philox4x32_10(make_uint4(0u, (uint32_t)RMBX_ACTUATION_PLANE_HOLD, r, ep), a.k0, a.k1);
    arrives = arrives && !(philox_uniform(w.x) < a.P);
  }
  if (arrives) a.out[idx] = arrived;
  if (k == 0u) a.mask_out[row] = arrives ? 1 : 0;
}

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

}  // namespace
}  // namespace rmbx

extern "C" int rmbx_action_perturb(const double* action, double* out, uint8_t* mask_out, double* ring,
                                   const rmbx_actuation_params* p, const double* bias_scale,
                                   const double* noise_scale, uint64_t seed, const int32_t* episode, const int32_t* r,
                                   const uint8_t* mask_in, int n, int A, void* stream) {
  RMBX_CHECK_ARG(action && out && mask_out && ring && p && bias_scale && noise_scale && episode && r,
                 "rmbx_action_perturb: NULL pointer");
  RMBX_CHECK_ARG(n >= 1 && A >= 1, "rmbx_action_perturb: n=%d, A=%d must be at least 1", n, A);
  RMBX_CHECK_ARG(p->delay >= 0 && p->delay <= RMBX_ACTUATION_MAX_DELAY, "rmbx_action_perturb: delay %d outside [0, %d]",
                 p->delay, RMBX_ACTUATION_MAX_DELAY);
  RMBX_CHECK_ARG(p->skip >= 1, "rmbx_action_perturb: skip %d must be at least 1", p->skip);
  RMBX_CHECK_ARG(p->noise >= 0.f && std::isfinite(p->noise), "rmbx_action_perturb: noise must be finite and >= 0");
  RMBX_CHECK_ARG(p->bias >= 0.f && std::isfinite(p->bias), "rmbx_action_perturb: bias must be finite and >= 0");
  RMBX_CHECK_ARG(p->hold >= 0.f && p->hold < 1.f, "rmbx_action_perturb: hold outside [0, 1)");
  RMBX_CHECK_ARG((uint64_t)n * (uint64_t)A * (uint64_t)(p->delay + 1) <= 0x7fffffffull,
                 "rmbx_action_perturb: n * A * (delay + 1) exceeds 2^31 - 1");
  RMBX_CHECK_ARG((((uintptr_t)action | (uintptr_t)out | (uintptr_t)ring | (uintptr_t)bias_scale | (uintptr_t)noise_scale) & 7u) == 0,
                 "rmbx_action_perturb: an f64 buffer is not 8-byte aligned");
  RMBX_CHECK_ARG((((uintptr_t)episode | (uintptr_t)r) & 3u) == 0, "rmbx_action_perturb: episode / r not 4-byte aligned");
  const size_t abytes = (size_t)n * A * sizeof(double), rbytes = abytes * (size_t)(p->delay + 1);
  RMBX_CHECK_ARG(!rmbx::overlap(action, abytes, out, abytes), "rmbx_action_perturb: out overlaps action");
  RMBX_CHECK_ARG(!rmbx::overlap(ring, rbytes, out, abytes) && !rmbx::overlap(ring, rbytes, action, abytes),
                 "rmbx_action_perturb: ring overlaps action or out");

  rmbx::ActuationArgs a;
  a.action = action, a.out = out, a.mask_out = mask_out, a.ring = ring;
  a.bias_scale = bias_scale, a.noise_scale = noise_scale;
  a.S = p->noise, a.B = p->bias, a.P = p->hold;
  a.D = (uint32_t)p->delay, a.skip = (uint32_t)p->skip;
  a.k0 = (uint32_t)(seed & 0xffffffffull), a.k1 = (uint32_t)(seed >> 32);
  a.episode = episode, a.r = r, a.mask_in = mask_in;
  a.n = (uint32_t)n, a.A = (uint32_t)A;
  const uint32_t total = (uint32_t)n * (uint32_t)A;
  hipLaunchKernelGGL(rmbx::action_perturb_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}
