// Episode streaming (--num_episodes): per-slot phase report, bad-state closure and the recycle of
// finished env slots -- record, assign the next episode, re-arm (include/rmbx.h).
//
// Latency-bound bookkeeping over n_env slots: plain C++, no atomics, vector stores only.  The
// recycle runs as ONE workgroup that walks the slots in chunks of 256 with a running base, so the
// slot -> episode assignment is the exclusive prefix sum of the done flags in slot order.

#include <cstring>

#include "rmbx_common.h"

#pragma clang fp contract(off)

namespace rmbx {

static inline hipStream_t stream_of(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kChunk = 256;

__global__ void sched_phases_kernel(const rmbx_sched_t* __restrict__ s, int32_t* __restrict__ prev,
                                    int32_t* __restrict__ phase, uint8_t* __restrict__ entered, int n_env) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env) return;
  const int32_t p = s[e].phase;
  phase[e] = p;
  entered[e] = p != prev[e] ? 1 : 0;
  prev[e] = p;
}

__global__ void sched_close_bad_kernel(rmbx_sched_t* __restrict__ s, const double* __restrict__ time,
                                       const int32_t* __restrict__ bad_resets, double* __restrict__ last_elapsed,
                                       int n_pre, int n_env) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_env) return;
  rmbx_sched_t v = s[e];
  if (v.done) return;
  if (bad_resets[e] > 0) {
    v.done = 1;
    v.phase = n_pre + 1;
    v.success = 0;
    v.result_reward = 0.0;
    v.duration = last_elapsed[e];
    s[e] = v;
  } else {
    last_elapsed[e] = v.phase == n_pre ? time[e] - v.phase_start : 0.0;
  }
}

__global__ void __launch_bounds__(kChunk) episode_recycle_kernel(rmbx_stream_buffers b) {
  __shared__ int32_t scan[kChunk];
  __shared__ int32_t list_slot[kChunk];
  __shared__ int32_t list_old[kChunk];  // local index of the finished episode
  __shared__ int32_t list_new[kChunk];  // local index of the assigned episode, -1 = queue empty
  const int t = threadIdx.x;
  const int32_t next0 = b.counters[0];
  const int32_t finished0 = b.counters[1];
  __syncthreads();  // every thread has read the counters before thread 0 rewrites them
  int32_t base = 0;
  for (int c0 = 0; c0 < b.n_env; c0 += kChunk) {
    const int s = c0 + t;
    int32_t old_ep = -1;
    if (s < b.n_env && b.sched[s].done) old_ep = b.slot_episode[s];
    const int32_t flag = old_ep >= 0 ? 1 : 0;
    // inclusive Hillis-Steele scan of the flags
    scan[t] = flag;
    __syncthreads();
    for (int off = 1; off < kChunk; off <<= 1) {
      const int32_t add = t >= off ? scan[t - off] : 0;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    const int32_t count = scan[kChunk - 1];
    const int32_t rank = scan[t] - flag;  // exclusive, within the chunk
    if (flag) {
      const int32_t old_local = old_ep - b.episode_base;
      const int32_t new_local = next0 + base + rank;
      const bool assign = new_local < b.n_episodes;
      const rmbx_sched_t v = b.sched[s];
      if (old_local >= 0 && old_local < b.n_episodes) {
        rmbx_episode_record_t r;
        memset(&r, 0, sizeof(r));
        r.episode = old_ep;
        r.slot = s;
        r.world_idx = b.world_idx[old_local];
        r.rollout_time_idx = v.rollout_time_idx;
        r.success = v.success;
        r.bad_state = b.bad_resets[s] > 0 ? 1 : 0;
        r.reward = v.result_reward;
        r.duration = v.duration;
        b.results[old_local] = r;
      }
      list_slot[rank] = s;
      list_old[rank] = (old_local >= 0 && old_local < b.n_episodes) ? old_local : -1;
      list_new[rank] = assign ? new_local : -1;
      if (assign) {
        rmbx_sched_t z;
        memset(&z, 0, sizeof(z));  // phase 0 from time 0 (rmbx_sched_reset)
        b.sched[s] = z;
        b.time[s] = 0.0;
        b.grip_cmd[s] = 0.0;
        b.bad_resets[s] = 0;
        b.last_elapsed[s] = 0.0;
        b.slot_episode[s] = b.episode_base + new_local;
      } else {
        b.slot_episode[s] = -1;
      }
      b.recycled[s] = assign ? 1 : 0;
    } else if (s < b.n_env) {
      b.recycled[s] = 0;
    }
    __syncthreads();
    // rows of the finished slots, all threads over the elements of one row at a time
    for (int j = 0; j < count; ++j) {
      const int slot = list_slot[j];
      const int32_t old_local = list_old[j], new_local = list_new[j];
      double* qpos = b.qpos + (size_t)slot * b.nq;
      if (b.final_qpos && old_local >= 0) {
        double* dst = b.final_qpos + (size_t)old_local * b.nq;
        for (int i = t; i < b.nq; i += kChunk) dst[i] = qpos[i];
      }
      if (new_local < 0) continue;
      const double* wp = b.world_pos + (size_t)new_local * 3;
      for (int i = t; i < b.nq; i += kChunk) {
        double q = b.qpos0[i];
        if (b.world_qadr >= 0 && i >= b.world_qadr && i < b.world_qadr + 3) q = wp[i - b.world_qadr];
        qpos[i] = q;
      }
      for (int i = t; i < b.nv; i += kChunk) {
        b.qvel[(size_t)slot * b.nv + i] = 0.0;
        b.qacc_ws[(size_t)slot * b.nv + i] = 0.0;
      }
      for (int i = t; i < b.nu; i += kChunk) b.ctrl[(size_t)slot * b.ctrl_stride + i] = b.ctrl0[i];
      if (t < 4) b.stats[(size_t)slot * 4 + t] = 0;
      if (t < 6) b.q_cmd[(size_t)slot * 6 + t] = b.motion0[t];
      if (t >= 6 && t < 15) b.target_R[(size_t)slot * 9 + (t - 6)] = b.motion0[t];
      if (t >= 15 && t < 18) b.target_p[(size_t)slot * 3 + (t - 15)] = b.motion0[t];
      if (b.world_body >= 0 && t >= 32 && t < 35)
        b.body_pos[((size_t)slot * b.nbody + b.world_body) * 3 + (t - 32)] = wp[t - 32];
    }
    base += count;
    __syncthreads();  // the lists and the scan array are rewritten by the next chunk
  }
  if (t == 0) {
    const int32_t left = b.n_episodes - next0;
    b.counters[0] = next0 + (base < left ? base : (left > 0 ? left : 0));
    b.counters[1] = finished0 + base;
  }
}

}  // namespace rmbx

using namespace rmbx;

extern "C" {

int rmbx_sched_phases(const rmbx_sched_t* sched, int32_t* prev_phase, int32_t* phase, uint8_t* entered,
                      int n_env, void* stream) {
  RMBX_CHECK_ARG(sched && prev_phase && phase && entered && n_env >= 0, "rmbx_sched_phases: bad arguments");
  if (n_env == 0) return RMBX_OK;
  hipLaunchKernelGGL(sched_phases_kernel, dim3((n_env + 255) / 256), dim3(256), 0, stream_of(stream), sched,
                     prev_phase, phase, entered, n_env);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}

int rmbx_sched_close_bad(rmbx_sched_t* sched, const double* time, const int32_t* bad_resets,
                         double* last_elapsed, int n_pre, int n_env, void* stream) {
  RMBX_CHECK_ARG(sched && time && bad_resets && last_elapsed && n_env >= 0 && n_pre >= 0,
                 "rmbx_sched_close_bad: bad arguments");
  if (n_env == 0) return RMBX_OK;
  hipLaunchKernelGGL(sched_close_bad_kernel, dim3((n_env + 255) / 256), dim3(256), 0, stream_of(stream), sched,
                     time, bad_resets, last_elapsed, n_pre, n_env);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}

int rmbx_episode_recycle(const rmbx_stream_buffers* b, void* stream) {
  RMBX_CHECK_ARG(b != nullptr, "rmbx_episode_recycle: bufs is NULL");
  RMBX_CHECK_ARG(b->sched && b->slot_episode && b->recycled && b->counters && b->results && b->world_idx &&
                     b->world_pos,
                 "rmbx_episode_recycle: a schedule / queue pointer is NULL");
  RMBX_CHECK_ARG(b->time && b->qpos && b->qvel && b->qacc_ws && b->ctrl && b->body_pos && b->stats && b->qpos0 &&
                     b->ctrl0,
                 "rmbx_episode_recycle: an engine pointer is NULL");
  RMBX_CHECK_ARG(b->q_cmd && b->grip_cmd && b->target_R && b->target_p && b->motion0 && b->bad_resets &&
                     b->last_elapsed,
                 "rmbx_episode_recycle: a motion pointer is NULL");
  RMBX_CHECK_ARG(b->n_env >= 0 && b->n_episodes >= 0 && b->nq > 0 && b->nv >= 0 && b->nu >= 0 &&
                     b->ctrl_stride >= b->nu && b->nbody > 0,
                 "rmbx_episode_recycle: bad sizes");
  RMBX_CHECK_ARG(b->world_body < b->nbody && (b->world_qadr < 0 || b->world_qadr + 3 <= b->nq),
                 "rmbx_episode_recycle: world_body / world_qadr out of range");
  RMBX_CHECK_ARG(b->world_body < 0 || b->world_qadr < 0, "rmbx_episode_recycle: world_body and world_qadr both set");
  if (b->n_env == 0) return RMBX_OK;
  hipLaunchKernelGGL(episode_recycle_kernel, dim3(1), dim3(kChunk), 0, stream_of(stream), *b);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}

}  // extern "C"
