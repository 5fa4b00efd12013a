// SARNN policy step (policy/sarnn/SarnnPolicy.py:133-152 of the reference), the branch that reaches
// predicted_state: attention encoder + spatial softmax per (env, camera), then LSTMCell + state
// decoder per env.
//
// sarnn_attention_kernel: one workgroup per (env, camera).  The three valid 3x3 convolutions
// (3 -> 16 -> 32 -> K, LeakyReLU(0.3) after each) run band by band: a band of B rows of the last map
// needs B + 2 rows of the 32-channel map, B + 4 of the 16-channel map and B + 6 image rows, all held
// in LDS (the halo rows are recomputed by the next band; nothing but the image is read from and
// nothing but the K key points is written to global memory).  Two LDS regions are reused within a
// band: the image band's becomes the 32-channel band's, the 16-channel band's the K-channel band's.
// Work is dealt to waves as (8 output channels) x (64 pixels): a lane owns a pixel, the
// output-channel group is wave-uniform, so the weights (packed [group][cin][tap][channel], include/
// rmbx.h) come through the scalar cache, adjacent channel pairs feed packed FMAs and each LDS value
// read feeds 8 FMAs.  After each band the
// wave that owns attention channel k folds the band into its running (max, sum, sum x, sum y) of
// softmax(map / T): fixed lane assignment, butterfly reductions, bands in order, so the result is
// reproducible and independent of the batch size.
//
// sarnn_lstm_kernel: one workgroup per env; thread j owns hidden unit j (its four gates), then the
// first state_dim threads apply the decoder to the new h.

#include "rmbx_common.h"

#include <cstdint>

namespace rmbx {
namespace {

// 16 waves = 4 per SIMD: one workgroup fills a CU (its LDS admits one); measured at 1024 envs, S = 64,
// K = 5: 0.95 ms per call, against 1.16 ms with 512 threads and 1.08 / 1.30 ms with 4-row bands
constexpr int kAttThreads = 1024;
constexpr int kAttMaxK = 16;
constexpr int kAttMaxBand = 8;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kOcg = 8;  // output channels per lane task of the first two convolutions

// LDS regions of a band of `band` rows of the S-6 map: A holds the 16-channel band, later the K-channel
// band; B holds the image band, later the 32-channel band
__host__ __device__ inline size_t att_region_a(int S, int K, int band) {
  const size_t c1 = (size_t)16 * (band + 4) * (S - 2), c3 = (size_t)K * band * (S - 6);
  return c1 > c3 ? c1 : c3;
}
__host__ __device__ inline size_t att_region_b(int S, int band) {
  const size_t in = (size_t)3 * (band + 6) * S, c2 = (size_t)32 * (band + 2) * (S - 4);
  return in > c2 ? in : c2;
}

// output channels per lane task of the last convolution: its K channels in (K + 7) / 8 equal groups,
// rounded up to an even size (include/rmbx.h states the same rule for the packed weights)
__host__ __device__ inline int att_ocg3(int K) {
  const int g = (K + 7) / 8;
  return (((K + g - 1) / g) + 1) & ~1;
}

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : v * 0.3f; }

// valid 3x3 convolution + bias + LeakyReLU of an LDS band: in [CIN][hin][win] -> out [cout][hin-2][win-2];
// wp = packed weights [groups][CIN][9][OCG] (zero beyond cout)
template <int CIN, int OCG, int NW>
__device__ __forceinline__ void conv_band(const float* __restrict__ in, float* __restrict__ out,
                                          const float* __restrict__ wp, const float* __restrict__ bias, int cout,
                                          int hin, int win, int wave, int lane) {
  const int hout = hin - 2, wout = win - 2;
  const int npix = hout * wout;
  const int nchunk = (npix + 63) >> 6;
  const int ntask = nchunk * ((cout + OCG - 1) / OCG);
  for (int task = wave; task < ntask; task += NW) {
    const int g = task / nchunk;  // wave-uniform
    const int oc0 = g * OCG;
    const int p = (task - g * nchunk) * 64 + lane;
    const int pp = p < npix ? p : npix - 1;  // idle lanes of the last chunk read a valid pixel
    const int r = pp / wout, c = pp - r * wout;
    float acc[OCG];
#pragma unroll
    for (int j = 0; j < OCG; ++j) acc[j] = bias[oc0 + j < cout ? oc0 + j : cout - 1];
    const float* src = in + r * win + c;
    const float* wg = wp + (size_t)g * CIN * 9 * OCG;
#pragma unroll 1  // one input channel's 9 * OCG weights fill the scalar registers
    for (int ci = 0; ci < CIN; ++ci) {
      float x[9];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) x[ky * 3 + kx] = src[(ci * hin + ky) * win + kx];
      const float* wc = wg + ci * 9 * OCG;
#pragma unroll
      for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < OCG; ++j) acc[j] = fmaf(x[k], wc[k * OCG + j], acc[j]);
    }
    if (p < npix) {
#pragma unroll
      for (int j = 0; j < OCG; ++j)
        if (oc0 + j < cout) out[(oc0 + j) * npix + p] = leaky(acc[j]);
    }
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NT, int OCG3>
__global__ void __launch_bounds__(NT)
    sarnn_attention_kernel(const float* __restrict__ images, const float* __restrict__ w1,
                           const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                           const float* __restrict__ w3, const float* __restrict__ b3, float* __restrict__ keys,
                           int ncam, int S, int K, int band, float inv_t) {
  constexpr int NW = NT / 64;
  constexpr int NK = (kAttMaxK + NW - 1) / NW;  // attention channels whose running softmax a wave keeps
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int cam = blockIdx.x % ncam;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S3 = S - 6;
  float* s_a = lds;                                 // 16-channel band, then the K-channel band
  float* s_b = lds + att_region_a(S, K, band);      // image band, then the 32-channel band
  const float* img = images + (size_t)blockIdx.x * 3 * S * S;
  w1 += cam * 16 * 3 * 9;
  b1 += cam * 16;
  w2 += cam * 32 * 16 * 9;
  b2 += cam * 32;
  w3 += cam * ((K + OCG3 - 1) / OCG3) * OCG3 * 32 * 9;
  b3 += cam * K;
  const float denom = (float)(S3 - 1);  // positions are col / (S3 - 1), a correctly rounded f32 division

  // running softmax statistics of channels wave, wave + NW, ... (identical in every lane)
  float m_run[NK], s_run[NK], sx_run[NK], sy_run[NK];
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    m_run[i] = -INFINITY;
    s_run[i] = sx_run[i] = sy_run[i] = 0.f;
  }

  for (int o = 0; o < S3; o += band) {
    const int nb = S3 - o < band ? S3 - o : band;
    const int hin = nb + 6;
    __syncthreads();  // the previous band's softmax has read region A, its last convolution region B
    for (int ch = 0; ch < 3; ++ch) {
      const float* g = img + ((size_t)ch * S + o) * S;
      for (int i = tid; i < hin * S; i += NT) s_b[ch * hin * S + i] = g[i];
    }
    __syncthreads();
    conv_band<3, kOcg, NW>(s_b, s_a, w1, b1, 16, hin, S, wave, lane);
    __syncthreads();
    conv_band<16, kOcg, NW>(s_a, s_b, w2, b2, 32, hin - 2, S - 2, wave, lane);
    __syncthreads();
    conv_band<32, OCG3, NW>(s_b, s_a, w3, b3, K, hin - 4, S - 4, wave, lane);
    __syncthreads();
    const int npix = nb * S3;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int k = wave + i * NW;
      if (k < K) {  // wave-uniform
        const float* v = s_a + k * npix;
        float m = -INFINITY;
        for (int p = lane; p < npix; p += 64) m = fmaxf(m, v[p]);
        m = wave_max(m);
        float s = 0.f, sx = 0.f, sy = 0.f;
        for (int p = lane; p < npix; p += 64) {
          const int r = p / S3, c = p - r * S3;
          const float e = expf((v[p] - m) * inv_t);
          s += e;
          sx = fmaf(e, (float)c / denom, sx);
          sy = fmaf(e, (float)(o + r) / denom, sy);
        }
        s = wave_sum(s);
        sx = wave_sum(sx);
        sy = wave_sum(sy);
        const float mn = fmaxf(m_run[i], m);
        const float fa = expf((m_run[i] - mn) * inv_t);  // 0 for the first band (m_run = -inf)
        const float fb = expf((m - mn) * inv_t);
        s_run[i] = s_run[i] * fa + s * fb;
        sx_run[i] = sx_run[i] * fa + sx * fb;
        sy_run[i] = sy_run[i] * fa + sy * fb;
        m_run[i] = mn;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int k = wave + i * NW;
      if (k < K) {
        float* dst = keys + ((size_t)blockIdx.x * K + k) * 2;
        dst[0] = sx_run[i] / s_run[i];
        dst[1] = sy_run[i] / s_run[i];
      }
    }
  }
}

template <int NT, int OCG3>
int launch_attention(const float* images, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, float* keys, int n_env, int ncam, int S, int K, int band,
                     size_t lds, float inv_t, hipStream_t stream) {
  RMBX_CHECK_HIP(hipFuncSetAttribute((const void*)sarnn_attention_kernel<NT, OCG3>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sarnn_attention_kernel<NT, OCG3>), dim3(n_env * ncam), dim3(NT), lds, stream, images, w1, b1,
                     w2, b2, w3, b3, keys, ncam, S, K, band, inv_t);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}

constexpr int kLstmThreads = 128;
constexpr int kLstmMaxIn = 256;

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

__global__ void __launch_bounds__(kLstmThreads)
    sarnn_lstm_kernel(const float* __restrict__ state, const float* __restrict__ keys, float* __restrict__ h,
                      float* __restrict__ c, const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                      const float* __restrict__ b_ih, const float* __restrict__ b_hh, const float* __restrict__ w_dec,
                      const float* __restrict__ b_dec, const uint8_t* __restrict__ active, float* __restrict__ pred,
                      int state_dim, int key_dim, int hidden) {
  __shared__ float s_x[kLstmMaxIn];
  __shared__ float s_h[kLstmThreads];
  const int env = blockIdx.x;
  if (active && !active[env]) return;  // uniform over the workgroup
  const int tid = threadIdx.x;
  const int nin = state_dim + key_dim;
  for (int i = tid; i < nin; i += kLstmThreads)
    s_x[i] = i < state_dim ? state[(size_t)env * state_dim + i] : keys[(size_t)env * key_dim + (i - state_dim)];
  if (tid < hidden) s_h[tid] = h[(size_t)env * hidden + tid];
  __syncthreads();
  float hn = 0.f;
  if (tid < hidden) {
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = q * hidden + tid;
      const float* wi = w_ih + (size_t)row * nin;
      const float* wh = w_hh + (size_t)row * hidden;
      float a = 0.f, b = 0.f;
      for (int i = 0; i < nin; ++i) a = fmaf(s_x[i], wi[i], a);
      for (int i = 0; i < hidden; ++i) b = fmaf(s_h[i], wh[i], b);
      g[q] = (a + b_ih[row]) + (b + b_hh[row]);
    }
    const float cn = sigmoidf(g[1]) * c[(size_t)env * hidden + tid] + sigmoidf(g[0]) * tanhf(g[2]);
    hn = sigmoidf(g[3]) * tanhf(cn);
    c[(size_t)env * hidden + tid] = cn;
    h[(size_t)env * hidden + tid] = hn;
  }
  __syncthreads();  // every thread has read the old h
  if (tid < hidden) s_h[tid] = hn;
  __syncthreads();
  for (int s = tid; s < state_dim; s += kLstmThreads) {
    const float* wd = w_dec + (size_t)s * hidden;
    float a = 0.f;
    for (int i = 0; i < hidden; ++i) a = fmaf(s_h[i], wd[i], a);
    pred[(size_t)env * state_dim + s] = a + b_dec[s];
  }
}

}  // namespace
}  // namespace rmbx

extern "C" int rmbx_sarnn_attention(const float* images, const float* w1, const float* b1, const float* w2,
                                    const float* b2, const float* w3, const float* b3, float* keys, int n_env,
                                    int ncam, int S, int K, float temperature, void* stream) {
  RMBX_CHECK_ARG(n_env >= 0, "rmbx_sarnn_attention: n_env = %d must be >= 0", n_env);
  // an empty batch has no device memory behind it: its per-env pointers may be NULL
  RMBX_CHECK_ARG(images || n_env == 0, "rmbx_sarnn_attention: images is NULL");
  RMBX_CHECK_ARG(w1 && b1 && w2 && b2 && w3 && b3, "rmbx_sarnn_attention: a weight or bias pointer is NULL");
  RMBX_CHECK_ARG(keys || n_env == 0, "rmbx_sarnn_attention: keys is NULL");
  RMBX_CHECK_ARG(ncam >= 1 && ncam <= 4, "rmbx_sarnn_attention: ncam = %d outside [1, 4]", ncam);
  RMBX_CHECK_ARG(S >= 8 && S <= 128, "rmbx_sarnn_attention: S = %d outside [8, 128]", S);
  RMBX_CHECK_ARG(K >= 1 && K <= rmbx::kAttMaxK, "rmbx_sarnn_attention: K = %d outside [1, %d]", K, rmbx::kAttMaxK);
  RMBX_CHECK_ARG(temperature > 0.f && temperature <= 3.0e38f,
                 "rmbx_sarnn_attention: temperature = %g must be positive and finite", (double)temperature);
  RMBX_CHECK_ARG((long long)n_env * ncam <= 0x7fffffffLL, "rmbx_sarnn_attention: n_env * ncam exceeds the grid limit");
  int band = S - 6 < rmbx::kAttMaxBand ? S - 6 : rmbx::kAttMaxBand;
  auto lds_bytes = [&](int b) { return (rmbx::att_region_a(S, K, b) + rmbx::att_region_b(S, b)) * sizeof(float); };
  while (band > 1 && lds_bytes(band) > (size_t)rmbx::kLdsBytes) --band;
  const size_t lds = lds_bytes(band);
  RMBX_CHECK_ARG(lds <= (size_t)rmbx::kLdsBytes, "rmbx_sarnn_attention: S = %d, K = %d needs %zu bytes of LDS", S, K, lds);
  if (n_env == 0) return RMBX_OK;
  const float inv_t = 1.f / temperature;
  hipStream_t st = (hipStream_t)stream;
#define RMBX_SARNN_LAUNCH(OCG3)                                                                                  \
  return rmbx::launch_attention<rmbx::kAttThreads, OCG3>(images, w1, b1, w2, b2, w3, b3, keys, n_env, ncam, S, K, \
                                                         band, lds, inv_t, st)
  switch (rmbx::att_ocg3(K)) {
    case 2: RMBX_SARNN_LAUNCH(2);
    case 4: RMBX_SARNN_LAUNCH(4);
    case 6: RMBX_SARNN_LAUNCH(6);
    default: RMBX_SARNN_LAUNCH(8);
  }
#undef RMBX_SARNN_LAUNCH
}

extern "C" int rmbx_sarnn_lstm_step(const float* state, const float* keys, float* h, float* c, const float* w_ih,
                                    const float* w_hh, const float* b_ih, const float* b_hh, const float* w_dec,
                                    const float* b_dec, const uint8_t* active, float* pred, int n_env, int state_dim,
                                    int key_dim, int hidden, void* stream) {
  RMBX_CHECK_ARG(n_env >= 0, "rmbx_sarnn_lstm_step: n_env = %d must be >= 0", n_env);
  // an empty batch has no device memory behind it: its per-env pointers may be NULL
  RMBX_CHECK_ARG(state || n_env == 0, "rmbx_sarnn_lstm_step: state is NULL");
  RMBX_CHECK_ARG((h && c) || n_env == 0, "rmbx_sarnn_lstm_step: h or c is NULL");
  RMBX_CHECK_ARG(w_ih && w_hh && b_ih && b_hh && w_dec && b_dec,
                 "rmbx_sarnn_lstm_step: a weight or bias pointer is NULL");
  RMBX_CHECK_ARG(pred || n_env == 0, "rmbx_sarnn_lstm_step: pred is NULL");
  RMBX_CHECK_ARG(hidden >= 1 && hidden <= rmbx::kLstmThreads, "rmbx_sarnn_lstm_step: hidden = %d outside [1, %d]",
                 hidden, rmbx::kLstmThreads);
  RMBX_CHECK_ARG(state_dim >= 1, "rmbx_sarnn_lstm_step: state_dim = %d must be >= 1", state_dim);
  RMBX_CHECK_ARG(key_dim >= 0, "rmbx_sarnn_lstm_step: key_dim = %d must be >= 0", key_dim);
  RMBX_CHECK_ARG(keys || key_dim == 0 || n_env == 0, "rmbx_sarnn_lstm_step: keys is NULL");
  RMBX_CHECK_ARG(state_dim <= rmbx::kLstmMaxIn && key_dim <= rmbx::kLstmMaxIn - state_dim,
                 "rmbx_sarnn_lstm_step: state_dim + key_dim = %d exceeds %d", state_dim + key_dim, rmbx::kLstmMaxIn);
  if (n_env == 0) return RMBX_OK;
  hipLaunchKernelGGL(rmbx::sarnn_lstm_kernel, dim3(n_env), dim3(rmbx::kLstmThreads), 0, (hipStream_t)stream, state,
                     keys, h, c, w_ih, w_hh, b_ih, b_hh, w_dec, b_dec, active, pred, state_dim, key_dim, hidden);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}
