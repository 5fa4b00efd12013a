// Per-episode sampler noise: Philox4x32-10 keyed by the run's seed and counted by (block, plane,
// draw, episode), turned into standard normals by Box-Muller (the rule: include/rmbx.h,
// rmbx_philox_normal).  A noise element is a pure function of (seed, episode, draw, plane, i), so
// a row does not depend on its position in the batch, the batch size or the launch it is part of.
//
// One thread per Philox block = four outputs = 16 bytes.  At the DiffusionPolicy shapes (x0 + 99
// noise planes = 100 planes x 2048 rows x 112 f32 = 91.75 MB, measured 2.27 TB/s) the stores are the
// bulk of the work: a whole block at a 16-byte aligned address leaves as one dwordx4 store; a row
// tail (L % 4 != 0) and the blocks of rows that start off a 16-byte boundary leave as dword stores
// of the elements inside the row.  The grid is capped near 2048 workgroups (8 per CU) and strides
// over the rest.  No LDS, no atomics.  The generator and Box-Muller are in rmbx_philox.h.

#include "rmbx_common.h"
#include "rmbx_philox.h"

#include <climits>
#include <cstdint>

namespace rmbx {
namespace {

// grid.y = plane; grid.x strides over the n * nb blocks of a plane (nb = ceil(L / 4)).
// row_len = L (normals) or 4 * nb (raw words): the length of an output row in elements.
__global__ void __launch_bounds__(256) philox_normal_kernel(uint32_t k0, uint32_t k1,
                                                            const int32_t* __restrict__ episode,
                                                            const int32_t* __restrict__ draw, uint32_t plane_first,
                                                            uint32_t* __restrict__ out, uint32_t n, uint32_t nb,
                                                            uint32_t row_len, int kind) {
  const uint32_t plane = plane_first + blockIdx.y;
  uint32_t* const plane_out = out + (size_t)blockIdx.y * n * row_len;
  const uint32_t total = n * nb;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const uint32_t row = idx / nb;
    const uint32_t j = idx - row * nb;
    const uint4 w = philox4x32_10(make_uint4(j, plane, (uint32_t)draw[row], (uint32_t)episode[row]), k0, k1);
    uint4 v = w;
    if (kind == 0) {
      const float2 a = box_muller(w.x, w.y);
      const float2 b = box_muller(w.z, w.w);
      v = make_uint4(__float_as_uint(a.x), __float_as_uint(a.y), __float_as_uint(b.x), __float_as_uint(b.y));
    }
    const uint32_t e0 = 4u * j;
    uint32_t* const dst = plane_out + (size_t)row * row_len + e0;
    if (e0 + 4u <= row_len && ((uintptr_t)dst & 15u) == 0) {
      *reinterpret_cast<uint4*>(dst) = v;
    } else {
      // the elements of the block that lie inside the row, one dword each
      if (e0 + 0u < row_len) dst[0] = v.x;
      if (e0 + 1u < row_len) dst[1] = v.y;
      if (e0 + 2u < row_len) dst[2] = v.z;
      if (e0 + 3u < row_len) dst[3] = v.w;
    }
  }
}

}  // namespace
}  // namespace rmbx

extern "C" int rmbx_philox_normal(uint64_t seed, const int32_t* episode, const int32_t* draw, int plane0, int nplane,
                                  void* out, int n, int L, int kind, void* stream) {
  RMBX_CHECK_ARG(episode && draw && out, "rmbx_philox_normal: NULL pointer");
  RMBX_CHECK_ARG(n >= 1 && L >= 1 && nplane >= 1, "rmbx_philox_normal: n, L and nplane must be at least 1");
  RMBX_CHECK_ARG(plane0 >= 0 && plane0 <= INT_MAX - nplane, "rmbx_philox_normal: plane0 out of range");
  RMBX_CHECK_ARG(kind == 0 || kind == 1, "rmbx_philox_normal: unknown kind %d", kind);
  RMBX_CHECK_ARG(((uintptr_t)out & 3u) == 0, "rmbx_philox_normal: out must be 4-byte aligned");
  const uint32_t nb = ((uint32_t)L + 3u) / 4u;
  RMBX_CHECK_ARG((uint64_t)n * nb <= 0x7fffffffull, "rmbx_philox_normal: n * ceil(L / 4) exceeds 2^31 - 1");
  const uint32_t per_plane = (uint32_t)n * nb;
  const uint32_t row_len = kind == 0 ? (uint32_t)L : 4u * nb;
  // at most 65535 planes per launch (grid.y); near 2048 workgroups per launch, the rest by stride
  for (int p = 0; p < nplane; p += 65535) {
    const uint32_t ny = (uint32_t)(nplane - p < 65535 ? nplane - p : 65535);
    uint32_t gx = (per_plane + 255u) / 256u;
    if ((uint64_t)gx * ny > 2048u) gx = ny >= 2048u ? 1u : 2048u / ny;
    uint32_t* const o = static_cast<uint32_t*>(out) + (size_t)p * (uint32_t)n * row_len;
    hipLaunchKernelGGL(rmbx::philox_normal_kernel, dim3(gx, ny), dim3(256), 0, (hipStream_t)stream,
                       (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), episode, draw, (uint32_t)(plane0 + p),
                       o, (uint32_t)n, nb, row_len, kind);
    RMBX_CHECK_LAUNCH();
  }
  return RMBX_OK;
}
