// Per-episode perturbation of the camera frame the policy reads (the rule: include/rmbx.h,
// rmbx_image_perturb): episode-constant lighting (brightness, contrast, channel gains) and occluder,
// per-frame sensor noise, all from the Philox rule of rmbx_philox.h keyed by (seed, episode, draw,
// plane), written as the perturbed 8-bit frame and / or one of the renderer's five policy forms.
//
// A streaming kernel.  grid.y strides over the rows (env slots), grid.x over the units of a row, so
// a workgroup stays inside one row while it walks grid.x: the row's episode constants (four Philox
// blocks of wave-uniform counters) are computed once per row a workgroup visits, not per element.
// Wide path (W % 4 == 0, buffers on their natural boundaries): a unit is 12 elements = 4 pixels of
// one image line = 3 Philox blocks = three dwords in; pixel, channel and block boundaries coincide.
// It stores three dwords of rgb_out, and the policy form as 16 / 8-byte pieces (NCHW: four pixels of
// a channel; space-to-depth: the six channels each of two cells, and their zero tail on odd lines).
// Element path (any other width, L % 4 != 0, rows off a 4-byte boundary): a unit is one Philox
// block, handled byte by byte.  The grid is capped near 2048 workgroups.  No LDS, no atomics.

#include "rmbx_common.h"
#include "rmbx_philox.h"

#include <hip/hip_bf16.h>

#include <cmath>
#include <cstdint>

namespace rmbx {
namespace {

struct PerturbArgs {
  const uint8_t* rgb;
  uint8_t* rgb_out;
  void* policy;
  int policy_dtype;
  float B, C, G, sigma;
  int occ_h, occ_w;
  float mean[3], std[3];
  uint32_t k0, k1;
  const int32_t* episode;
  const int32_t* draw;
  uint32_t camera;
  const uint8_t* active;
  uint32_t n, H, W;
};

// the constants of one row (episode): wave-uniform
struct RowConst {
  uint32_t ep, dr;
  float b, c, g0, g1, g2;
  int y0, y1, x0, x1;  // the occluder [y0, y1) x [x0, x1); empty when there is none
  float o0, o1, o2;
};

__device__ __forceinline__ RowConst row_const(const PerturbArgs& a, uint32_t row) {
#pragma clang fp contract(off)
  RowConst r;
  r.ep = (uint32_t)a.episode[row];
  r.dr = (uint32_t)a.draw[row];
  r.b = 0.f;
  r.c = r.g0 = r.g1 = r.g2 = 1.f;
  r.y0 = r.y1 = r.x0 = r.x1 = 0;
  r.o0 = r.o1 = r.o2 = 0.f;
  if (a.B != 0.f || a.C != 0.f || a.G != 0.f) {
    const uint4 p = philox4x32_10(make_uint4(0u, (uint32_t)RMBX_PERTURB_PLANE_PHOTO, 0u, r.ep), a.k0, a.k1);
    const uint4 q = philox4x32_10(make_uint4(1u, (uint32_t)RMBX_PERTURB_PLANE_PHOTO, 0u, r.ep), a.k0, a.k1);
    r.b = a.B * (2.f * philox_uniform(p.x) - 1.f);
    r.c = 1.f + a.C * (2.f * philox_uniform(p.y) - 1.f);
    r.g0 = 1.f + a.G * (2.f * philox_uniform(p.z) - 1.f);
    r.g1 = 1.f + a.G * (2.f * philox_uniform(p.w) - 1.f);
    r.g2 = 1.f + a.G * (2.f * philox_uniform(q.x) - 1.f);
  }
  if (a.occ_h > 0) {
    const uint32_t plane = (uint32_t)RMBX_PERTURB_PLANE_OCC + a.camera;
    const uint4 p = philox4x32_10(make_uint4(0u, plane, 0u, r.ep), a.k0, a.k1);
    const uint4 q = philox4x32_10(make_uint4(1u, plane, 0u, r.ep), a.k0, a.k1);
    r.y0 = (int)(philox_uniform(p.x) * (float)((int)a.H - a.occ_h + 1));
    r.x0 = (int)(philox_uniform(p.y) * (float)((int)a.W - a.occ_w + 1));
    r.y1 = r.y0 + a.occ_h;
    r.x1 = r.x0 + a.occ_w;
    r.o0 = (float)(p.z >> 24);
    r.o1 = (float)(p.w >> 24);
    r.o2 = (float)(q.x >> 24);
  }
  return r;
}

// steps 1..8 of the rule for one element of channel k
__device__ __forceinline__ uint32_t perturb_elem(const PerturbArgs& a, const RowConst& r, uint32_t u, int k,
                                                 bool in_occ, float z) {
#pragma clang fp contract(off)
  float v = (float)u;
  if (a.C != 0.f) {
    v = (v - 127.5f) * r.c;
    v = v + 127.5f;
  }
  if (a.G != 0.f) v = v * (k == 0 ? r.g0 : k == 1 ? r.g1 : r.g2);
  if (a.B != 0.f) v = v + r.b;
  if (in_occ) v = k == 0 ? r.o0 : k == 1 ? r.o1 : r.o2;
  if (a.sigma > 0.f) v = v + a.sigma * z;
  return (uint32_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
}

// the renderer's policy value of an 8-bit pixel (store_policy, rmbx_render.hip)
__device__ __forceinline__ float policy_value(const PerturbArgs& a, uint32_t u, int k) {
#pragma clang fp contract(off)
  return ((float)u / 255.0f - a.mean[k]) / a.std[k];
}

__device__ __forceinline__ uint32_t bf16_bits(float v) {
  return (uint32_t)__bfloat16_as_ushort(__float2bfloat16(v));
}

// Wide path.  upr = W * H / 4 units per row; unit q holds pixels 4q .. 4q+3 of line y = 4q / W.
__global__ void __launch_bounds__(256) image_perturb_wide_kernel(PerturbArgs a, uint32_t upr) {
  const uint32_t L = a.H * a.W * 3u, hw = a.H * a.W;
  const uint32_t noise_plane = (uint32_t)RMBX_PERTURB_PLANE_NOISE + a.camera;
  for (uint32_t row = blockIdx.y; row < a.n; row += gridDim.y) {
    if (a.active && !a.active[row]) continue;
    const RowConst r = row_const(a, row);
    const uint8_t* const src = a.rgb + (size_t)row * L;
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < upr; q += gridDim.x * 256u) {
      const uint32_t p0 = 4u * q, y = p0 / a.W, x = p0 - y * a.W;
      const uint32_t* const s = reinterpret_cast<const uint32_t*>(src + (size_t)12u * q);
      const uint32_t in[3] = {s[0], s[1], s[2]};
      float z[12];
      if (a.sigma > 0.f) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const uint4 w = philox4x32_10(make_uint4(3u * q + t, noise_plane, r.dr, r.ep), a.k0, a.k1);
          const float2 za = box_muller(w.x, w.y), zb = box_muller(w.z, w.w);
          z[4 * t] = za.x, z[4 * t + 1] = za.y, z[4 * t + 2] = zb.x, z[4 * t + 3] = zb.y;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 12; ++t) z[t] = 0.f;
      }
      const bool occ_y = (int)y >= r.y0 && (int)y < r.y1;
      uint32_t u[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) {
        const int px = (int)x + e / 3;
        const bool in_occ = occ_y && px >= r.x0 && px < r.x1;
        u[e] = perturb_elem(a, r, (in[e >> 2] >> (8 * (e & 3))) & 0xffu, e % 3, in_occ, z[e]);
      }
      if (a.rgb_out) {
        uint32_t* const d = reinterpret_cast<uint32_t*>(a.rgb_out + (size_t)row * L + (size_t)12u * q);
#pragma unroll
        for (int t = 0; t < 3; ++t) d[t] = u[4 * t] | (u[4 * t + 1] << 8) | (u[4 * t + 2] << 16) | (u[4 * t + 3] << 24);
      }
      if (!a.policy) continue;
      if (a.policy_dtype == 0) {
        float* const o = reinterpret_cast<float*>(a.policy) + (size_t)row * 3u * hw + p0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          *reinterpret_cast<float4*>(o + (size_t)k * hw) = make_float4(policy_value(a, u[k], k), policy_value(a, u[3 + k], k),
                                                                         policy_value(a, u[6 + k], k), policy_value(a, u[9 + k], k));
      } else if (a.policy_dtype == 1) {
        uint16_t* const o = reinterpret_cast<uint16_t*>(a.policy) + (size_t)row * 3u * hw + p0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          *reinterpret_cast<uint2*>(o + (size_t)k * hw) =
              make_uint2(bf16_bits(policy_value(a, u[k], k)) | (bf16_bits(policy_value(a, u[3 + k], k)) << 16),
                         bf16_bits(policy_value(a, u[6 + k], k)) | (bf16_bits(policy_value(a, u[9 + k], k)) << 16));
      } else {
        // space-to-depth: pixels (x, x+1) and (x+2, x+3) fill channels 6 * (y & 1) .. + 5 of two
        // neighbouring cells; an odd line also writes the cells' zero channels 12..15
        const uint32_t Hs = a.H >> 1, Ws = a.W >> 1;
        const size_t cell = ((size_t)row * Hs + (y >> 1)) * Ws + (x >> 1);
        const bool odd = y & 1u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t* const v = u + 6 * h;
          if (a.policy_dtype == 4) {
            uint8_t* const o = reinterpret_cast<uint8_t*>(a.policy) + (cell + h) * 16u;
            if (!odd) {
              *reinterpret_cast<uint32_t*>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
              *reinterpret_cast<uint16_t*>(o + 4) = (uint16_t)(v[4] | (v[5] << 8));
            } else {
              *reinterpret_cast<uint16_t*>(o + 6) = (uint16_t)(v[0] | (v[1] << 8));
              *reinterpret_cast<uint2*>(o + 8) = make_uint2(v[2] | (v[3] << 8) | (v[4] << 16) | (v[5] << 24), 0u);
            }
          } else if (a.policy_dtype == 2) {
            uint32_t* const o = reinterpret_cast<uint32_t*>(a.policy) + (cell + h) * 8u;
            uint32_t w[3];
#pragma unroll
            for (int t = 0; t < 3; ++t)
              w[t] = bf16_bits(policy_value(a, v[2 * t], (2 * t) % 3)) | (bf16_bits(policy_value(a, v[2 * t + 1], (2 * t + 1) % 3)) << 16);
            if (!odd) {
              *reinterpret_cast<uint2*>(o) = make_uint2(w[0], w[1]);
              o[2] = w[2];
            } else {
              o[3] = w[0];
              *reinterpret_cast<uint4*>(o + 4) = make_uint4(w[1], w[2], 0u, 0u);
            }
          } else {
            float* const o = reinterpret_cast<float*>(a.policy) + (cell + h) * 16u;
            float f[6];
#pragma unroll
            for (int t = 0; t < 6; ++t) f[t] = policy_value(a, v[t], t % 3);
            if (!odd) {
              *reinterpret_cast<float4*>(o) = make_float4(f[0], f[1], f[2], f[3]);
              *reinterpret_cast<float2*>(o + 4) = make_float2(f[4], f[5]);
            } else {
              *reinterpret_cast<float2*>(o + 6) = make_float2(f[0], f[1]);
              *reinterpret_cast<float4*>(o + 8) = make_float4(f[2], f[3], f[4], f[5]);
              *reinterpret_cast<float4*>(o + 12) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
          }
        }
      }
    }
  }
}

// Element path.  upr = ceil(L / 4) units per row; unit j is Philox block j: elements 4j .. 4j+3 < L.
__global__ void __launch_bounds__(256) image_perturb_elem_kernel(PerturbArgs a, uint32_t upr) {
  const uint32_t L = a.H * a.W * 3u, hw = a.H * a.W;
  const uint32_t noise_plane = (uint32_t)RMBX_PERTURB_PLANE_NOISE + a.camera;
  for (uint32_t row = blockIdx.y; row < a.n; row += gridDim.y) {
    if (a.active && !a.active[row]) continue;
    const RowConst r = row_const(a, row);
    const uint8_t* const src = a.rgb + (size_t)row * L;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < upr; j += gridDim.x * 256u) {
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.sigma > 0.f) {
        const uint4 w = philox4x32_10(make_uint4(j, noise_plane, r.dr, r.ep), a.k0, a.k1);
        const float2 za = box_muller(w.x, w.y), zb = box_muller(w.z, w.w);
        z[0] = za.x, z[1] = za.y, z[2] = zb.x, z[3] = zb.y;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t e = 4u * j + t;
        if (e >= L) break;
        const uint32_t pix = e / 3u, k = e - 3u * pix, y = pix / a.W, x = pix - y * a.W;
        const bool in_occ = (int)y >= r.y0 && (int)y < r.y1 && (int)x >= r.x0 && (int)x < r.x1;
        const uint32_t u = perturb_elem(a, r, src[e], (int)k, in_occ, z[t]);
        if (a.rgb_out) a.rgb_out[(size_t)row * L + e] = (uint8_t)u;
        if (!a.policy) continue;
        if (a.policy_dtype == 0) {
          reinterpret_cast<float*>(a.policy)[((size_t)row * 3u + k) * hw + pix] = policy_value(a, u, (int)k);
        } else if (a.policy_dtype == 1) {
          reinterpret_cast<__hip_bfloat16*>(a.policy)[((size_t)row * 3u + k) * hw + pix] =
              __float2bfloat16(policy_value(a, u, (int)k));
        } else {
          const uint32_t Hs = a.H >> 1, Ws = a.W >> 1;
          const size_t base = (((size_t)row * Hs + (y >> 1)) * Ws + (x >> 1)) * 16u;
          const uint32_t ch = ((y & 1u) * 2u + (x & 1u)) * 3u + k;
          const bool tail = k == 0u && (y & 1u) && (x & 1u);  // once per cell: its zero channels
          if (a.policy_dtype == 2) {
            __hip_bfloat16* const o = reinterpret_cast<__hip_bfloat16*>(a.policy) + base;
            o[ch] = __float2bfloat16(policy_value(a, u, (int)k));
            if (tail)
              for (int c = 12; c < 16; ++c) o[c] = __float2bfloat16(0.0f);
          } else if (a.policy_dtype == 3) {
            float* const o = reinterpret_cast<float*>(a.policy) + base;
            o[ch] = policy_value(a, u, (int)k);
            if (tail)
              for (int c = 12; c < 16; ++c) o[c] = 0.0f;
          } else {
            uint8_t* const o = reinterpret_cast<uint8_t*>(a.policy) + base;
            o[ch] = (uint8_t)u;
            if (tail)
              for (int c = 12; c < 16; ++c) o[c] = 0;
          }
        }
      }
    }
  }
}

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

}  // namespace
}  // namespace rmbx

extern "C" int rmbx_image_perturb(const uint8_t* rgb, uint8_t* rgb_out, void* policy, int policy_dtype,
                                  const rmbx_perturb_params* p, uint64_t seed, const int32_t* episode,
                                  const int32_t* draw, int camera, const uint8_t* active, int n, int H, int W,
                                  void* stream) {
  RMBX_CHECK_ARG(rgb && p && episode && draw, "rmbx_image_perturb: NULL pointer");
  RMBX_CHECK_ARG(rgb_out || policy, "rmbx_image_perturb: neither rgb_out nor policy is given");
  RMBX_CHECK_ARG(n >= 1 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192,
                 "rmbx_image_perturb: n=%d, image %dx%d outside n >= 1, 1..8192", n, H, W);
  RMBX_CHECK_ARG((uint64_t)n * (uint64_t)H * (uint64_t)W * 3u <= 0x7fffffffull,
                 "rmbx_image_perturb: n * H * W * 3 exceeds 2^31 - 1");
  RMBX_CHECK_ARG(policy_dtype >= 0 && policy_dtype <= 4,
                 "rmbx_image_perturb: policy_dtype must be 0 (f32), 1 (bf16), 2 (bf16 s2d), 3 (f32 s2d) or 4 (u8 s2d)");
  RMBX_CHECK_ARG(!policy || policy_dtype < 2 || (H % 2 == 0 && W % 2 == 0),
                 "rmbx_image_perturb: space-to-depth policy output needs an even image size");
  RMBX_CHECK_ARG(camera >= 0 && camera <= 255, "rmbx_image_perturb: camera %d outside [0, 255]", camera);
  RMBX_CHECK_ARG(p->brightness >= 0.f && p->brightness <= 255.f, "rmbx_image_perturb: brightness outside [0, 255]");
  RMBX_CHECK_ARG(p->contrast >= 0.f && p->contrast < 1.f, "rmbx_image_perturb: contrast outside [0, 1)");
  RMBX_CHECK_ARG(p->gain >= 0.f && p->gain < 1.f, "rmbx_image_perturb: gain outside [0, 1)");
  RMBX_CHECK_ARG(p->noise_sigma >= 0.f && std::isfinite(p->noise_sigma), "rmbx_image_perturb: noise_sigma must be finite and >= 0");
  RMBX_CHECK_ARG(p->occ_h >= 0 && p->occ_h <= H && p->occ_w >= 0 && p->occ_w <= W,
                 "rmbx_image_perturb: occluder %dx%d outside the %dx%d image", p->occ_h, p->occ_w, H, W);
  if (policy)
    for (int k = 0; k < 3; ++k)
      RMBX_CHECK_ARG(std::isfinite(p->mean[k]) && std::isfinite(p->std[k]) && p->std[k] != 0.f,
                     "rmbx_image_perturb: mean / std of channel %d must be finite, std non-zero", k);
  const size_t elems = (size_t)n * H * W * 3;
  const size_t esz = policy_dtype == 0 || policy_dtype == 3 ? 4 : policy_dtype == 4 ? 1 : 2;
  const size_t pbytes = (policy_dtype < 2 ? elems : (size_t)n * (H / 2) * (W / 2) * 16) * esz;
  RMBX_CHECK_ARG(!policy || ((uintptr_t)policy & (esz - 1)) == 0, "rmbx_image_perturb: policy is not aligned to its element");
  RMBX_CHECK_ARG(!rgb_out || rgb_out == rgb || !rmbx::overlap(rgb, elems, rgb_out, elems),
                 "rmbx_image_perturb: rgb_out overlaps rgb (only rgb_out == rgb is allowed)");
  RMBX_CHECK_ARG(!policy || !rmbx::overlap(rgb, elems, policy, pbytes), "rmbx_image_perturb: policy overlaps rgb");
  RMBX_CHECK_ARG(!policy || !rgb_out || !rmbx::overlap(rgb_out, elems, policy, pbytes),
                 "rmbx_image_perturb: policy overlaps rgb_out");

  rmbx::PerturbArgs a;
  a.rgb = rgb, a.rgb_out = rgb_out, a.policy = policy, a.policy_dtype = policy_dtype;
  a.B = p->brightness, a.C = p->contrast, a.G = p->gain, a.sigma = p->noise_sigma;
  a.occ_h = p->occ_h, a.occ_w = p->occ_w;
  for (int k = 0; k < 3; ++k) a.mean[k] = p->mean[k], a.std[k] = p->std[k];
  a.k0 = (uint32_t)(seed & 0xffffffffull), a.k1 = (uint32_t)(seed >> 32);
  a.episode = episode, a.draw = draw, a.camera = (uint32_t)camera, a.active = active;
  a.n = (uint32_t)n, a.H = (uint32_t)H, a.W = (uint32_t)W;
  // the wide path: four pixels of one line per unit, every buffer on the boundary of its widest access
  const bool wide = W % 4 == 0 && ((uintptr_t)rgb & 3u) == 0 && ((uintptr_t)rgb_out & 3u) == 0 &&
                    ((uintptr_t)policy & 15u) == 0;
  const uint32_t L = (uint32_t)H * W * 3u;
  const uint32_t upr = wide ? L / 12u : (L + 3u) / 4u;
  // near 2048 workgroups: a row per grid.y while the rows last, the units of a row over grid.x
  const uint32_t gy = (uint32_t)n < 2048u ? (uint32_t)n : 2048u;
  uint32_t gx = (upr + 255u) / 256u;
  const uint32_t cap = 2048u / gy > 1u ? 2048u / gy : 1u;
  if (gx > cap) gx = cap;
  if (wide)
    hipLaunchKernelGGL(rmbx::image_perturb_wide_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, a, upr);
  else
    hipLaunchKernelGGL(rmbx::image_perturb_elem_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, a, upr);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}
