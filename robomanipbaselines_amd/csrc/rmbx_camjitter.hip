// Per-episode jitter rows of the cameras (the rule: include/rmbx.h, rmbx_camera_jitter_draw): a
// displacement in the mount's frame, a rotation about the camera's own axes as a unit quaternion and
// a scale of fovy, from two Philox blocks of rmbx_philox.h per camera keyed by (seed, episode) on a
// plane of its own.  The renderer reads one camera's rows through rmbx_scene_tables.cam_rows
// (rmbx_render.hip).
//
// One thread per (camera, row): it computes the two blocks and writes the row's eight f64 (ncam * n
// is a few thousand at most: the launch, not the arithmetic, is the cost).  The rotation is drawn as
// its Rodrigues vector, so the device evaluates no sine or cosine: products, sums, one f64 square
// root and four divisions, all correctly rounded, which the host restates bit for bit.  No LDS, no
// atomics, no barriers (the range guard returns).

#include "rmbx_common.h"
#include "rmbx_philox.h"

#include <cmath>
#include <cstdint>

namespace rmbx {
namespace {

struct CamJitterArgs {
  double* rows;
  const int32_t* episode;
  const uint8_t* active;
  float P, T, F;
  uint32_t k0, k1;
  uint32_t n, ncam;
};

// S * (2 u(w) - 1), the bracket in f32; exactly 0 for a strength of zero
__device__ __forceinline__ double jitter_sym(float S, uint32_t w) {
#pragma clang fp contract(off)
  if (S == 0.f) return 0.0;
  const float s = 2.f * philox_uniform(w) - 1.f;
  return (double)S * (double)s;
}

__global__ void __launch_bounds__(256) camera_jitter_draw_kernel(CamJitterArgs a) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n * a.ncam) return;
  const uint32_t c = i / a.n, row = i - c * a.n;
  if (a.active && !a.active[row]) return;
  const uint32_t ep = (uint32_t)a.episode[row];
  const uint32_t plane = (uint32_t)RMBX_CAMERA_JITTER_PLANE;
  const uint4 w0 = philox4x32_10(make_uint4(2u * c, plane, 0u, ep), a.k0, a.k1);
  const uint4 w1 = philox4x32_10(make_uint4(2u * c + 1u, plane, 0u, ep), a.k0, a.k1);
  double* const out = a.rows + 8 * (size_t)i;  // [ncam][n][8]
  out[0] = jitter_sym(a.P, w0.x);
  out[1] = jitter_sym(a.P, w0.y);
  out[2] = jitter_sym(a.P, w0.z);
  const double r0 = jitter_sym(a.T, w1.x), r1 = jitter_sym(a.T, w1.y), r2 = jitter_sym(a.T, w1.z);
  // |r|^2 first, then the 1: the small terms' roundings stay small and the sum to 1 is rounded once,
  // which keeps | |q| - 1 | within an ulp of 1.0 (1 + r0 r0 + ... rounds three times at the size of 1)
  const double rr = r0 * r0 + r1 * r1 + r2 * r2;
  const double nrm = sqrt(1.0 + rr);
  out[3] = 1.0 / nrm;
  out[4] = r0 / nrm;
  out[5] = r1 / nrm;
  out[6] = r2 / nrm;
  out[7] = 1.0 + jitter_sym(a.F, w0.w);
}

}  // namespace
}  // namespace rmbx

extern "C" int rmbx_camera_jitter_draw(uint64_t seed, const int32_t* episode, const rmbx_camera_jitter_params* p,
                                       int ncam, double* rows, const uint8_t* active, int n, void* stream) {
  RMBX_CHECK_ARG(episode && p && rows, "rmbx_camera_jitter_draw: NULL pointer");
  RMBX_CHECK_ARG(n >= 1, "rmbx_camera_jitter_draw: n=%d must be at least 1", n);
  RMBX_CHECK_ARG(ncam >= 1 && ncam <= RMBX_CAMERA_JITTER_MAX_CAMERAS, "rmbx_camera_jitter_draw: ncam=%d outside [1, %d]",
                 ncam, RMBX_CAMERA_JITTER_MAX_CAMERAS);
  RMBX_CHECK_ARG((long long)n * ncam < (1ll << 31), "rmbx_camera_jitter_draw: n * ncam too large");
  // (a NaN fails every comparison, an infinity the upper one)
  RMBX_CHECK_ARG(p->pos >= 0.f && p->pos <= 0.5f, "rmbx_camera_jitter_draw: pos outside [0, 0.5]");
  // (the bound as the host forms T from R = 30: radians(R) = R * (pi / 180), halved)
  RMBX_CHECK_ARG(p->tan_half_rot >= 0.f && p->tan_half_rot <= (float)std::tan(30.0 * (3.141592653589793 / 180.0) / 2.0),
                 "rmbx_camera_jitter_draw: tan_half_rot outside [0, tan(15 deg)] (rot outside [0, 30] degrees)");
  RMBX_CHECK_ARG(p->fovy >= 0.f && p->fovy < 0.5f, "rmbx_camera_jitter_draw: fovy outside [0, 0.5)");
  RMBX_CHECK_ARG(((uintptr_t)rows & 7u) == 0, "rmbx_camera_jitter_draw: rows is not 8-byte aligned");
  RMBX_CHECK_ARG(((uintptr_t)episode & 3u) == 0, "rmbx_camera_jitter_draw: episode is not 4-byte aligned");

  rmbx::CamJitterArgs a;
  a.rows = rows, a.episode = episode, a.active = active;
  a.P = p->pos, a.T = p->tan_half_rot, a.F = p->fovy;
  a.k0 = (uint32_t)(seed & 0xffffffffull), a.k1 = (uint32_t)(seed >> 32);
  a.n = (uint32_t)n, a.ncam = (uint32_t)ncam;
  const uint32_t total = (uint32_t)n * (uint32_t)ncam;
  hipLaunchKernelGGL(rmbx::camera_jitter_draw_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}
