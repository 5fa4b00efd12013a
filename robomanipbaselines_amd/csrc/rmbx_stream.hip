// Episode streaming (--num_episodes): per-slot phase report, bad-state closure and the recycle of
// finished env slots -- record, assign the next episode, re-arm (include/rmbx.h).
//
// Latency-bound bookkeeping over n_env slots: plain C++, no atomics, vector stores only.  The
// recycle runs as ONE workgroup that walks the slots in chunks of 256 with a running base, so the
// slot -> episode assignment is the exclusive prefix sum of the done flags in slot order.
//
// Episode trace (--trace_dir, rmbx_episode_trace): the same one-workgroup scan gives every slot
// that keeps this step its row of the chunk; the rows themselves (about 14 KB each in the Cable
// scene, up to n_env of them per step) are copied by a second kernel on a grid of its own.

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

// Row index of every slot (the row rule of include/rmbx.h) and the scalar fields of the rows.
__global__ void __launch_bounds__(kChunk) episode_trace_index_kernel(rmbx_trace_buffers b) {
  __shared__ int32_t scan[kChunk];
  const int t = threadIdx.x;
  const int32_t used0 = b.rows[0];
  __syncthreads();  // every thread has read the counter before thread 0 rewrites it
  int32_t base = 0;
  for (int c0 = 0; c0 < b.n_env; c0 += kChunk) {
    const int s = c0 + t;
    int32_t ep = -1, k = 0;
    bool keep = false, ended = false;
    rmbx_sched_t v;
    memset(&v, 0, sizeof(v));
    if (s < b.n_env) {
      ep = b.slot_episode ? b.slot_episode[s] : b.episode_base + s;
      bool take = ep >= 0 && (!b.stepped || b.stepped[s] != 0);
      if (take && b.select) {
        const int64_t local = (int64_t)ep - b.episode_base;
        take = local >= 0 && local < b.n_episodes && b.select[local] != 0;
      }
      if (take) {
        if (b.trace_episode[s] != ep) {
          b.trace_episode[s] = ep;
          k = 0;
        } else {
          k = b.trace_step[s];
        }
        k += 1;
        b.trace_step[s] = k;
        v = b.sched[s];
        ended = v.done != 0 || v.phase > b.n_pre;
        keep = k % b.stride == 0 || ended;
      }
    }
    const int32_t flag = keep ? 1 : 0;
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
    if (s < b.n_env) {
      int32_t row = -1;
      if (keep) {
        const int64_t r = (int64_t)used0 + base + rank;
        if (r >= 0 && r < b.capacity) {
          row = (int32_t)r;
          b.out_episode[row] = ep;
          b.out_slot[row] = s;
          b.out_step[row] = k;
          b.out_phase[row] = v.phase;
          b.out_rollout_time_idx[row] = v.rollout_time_idx;
          uint8_t f = 0;
          if (ended) f |= RMBX_TRACE_DONE;
          if (v.success) f |= RMBX_TRACE_SUCCESS;
          if (ended && b.bad_resets && b.bad_resets[s] > 0) f |= RMBX_TRACE_BAD_STATE;
          b.out_flags[row] = f;
          b.out_time[row] = b.time[s];
          b.out_reward[row] = b.reward[s];
        }
      }
      b.slot_row[s] = row;
    }
    base += count;
    __syncthreads();  // the scan array is rewritten by the next chunk
  }
  if (t == 0) {
    const int64_t total = (int64_t)used0 + base;
    if (total > b.capacity) {
      b.rows[0] = b.capacity;
      b.rows[1] = 1;
    } else {
      b.rows[0] = (int32_t)total;
    }
  }
}

struct alignas(16) trace_u128 {
  uint64_t lo, hi;
};

// len 8-byte words from src to dst by the nt threads of a block.  Both rows start on 8 bytes; where
// they sit alike within 16 bytes (always, for an even row length on 16-byte aligned arrays) one
// leading word brings both to a 16-byte boundary, the body moves 16 bytes per access and an odd
// last word follows; rows that sit differently (odd length, slot and row of different parity) move
// 8 bytes per access.
__device__ __forceinline__ void trace_copy_words(const double* __restrict__ src, double* __restrict__ dst, int len,
                                                 int t, int nt) {
  const uint64_t* s = reinterpret_cast<const uint64_t*>(src);
  uint64_t* d = reinterpret_cast<uint64_t*>(dst);
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s), da = reinterpret_cast<uintptr_t>(d);
  if (((sa ^ da) & 15) == 0) {
    int head = (sa & 15) ? 1 : 0;
    if (head > len) head = len;
    const int pairs = (len - head) >> 1;
    const trace_u128* s2 = reinterpret_cast<const trace_u128*>(s + head);
    trace_u128* d2 = reinterpret_cast<trace_u128*>(d + head);
    for (int i = t; i < pairs; i += nt) d2[i] = s2[i];
    if (t == 0 && head) d[0] = s[0];
    if (t == nt - 1 && head + 2 * pairs < len) d[len - 1] = s[len - 1];
  } else {
    for (int i = t; i < len; i += nt) d[i] = s[i];
  }
}

constexpr int kTraceArrays = 7;  // ctrl, qpos, qvel, gxpos, gxmat, xpos, xquat
constexpr int kTraceThreads = 256;

// Block (s, a) copies array a of slot s to the row the index kernel gave the slot.
__global__ void __launch_bounds__(kTraceThreads) episode_trace_copy_kernel(rmbx_trace_buffers b) {
  const int s = blockIdx.x;
  const int32_t row = b.slot_row[s];
  if (row < 0) return;
  const double* src;
  double* dst;
  int len;
  size_t src_stride;
  switch (blockIdx.y) {
    case 0: src = b.ctrl; dst = b.out_ctrl; len = b.nu; src_stride = b.ctrl_stride; break;
    case 1: src = b.qpos; dst = b.out_qpos; len = b.nq; src_stride = b.nq; break;
    case 2: src = b.qvel; dst = b.out_qvel; len = b.nv; src_stride = b.nv; break;
    case 3: src = b.gxpos; dst = b.out_gxpos; len = b.ngeom * 3; src_stride = len; break;
    case 4: src = b.gxmat; dst = b.out_gxmat; len = b.ngeom * 9; src_stride = len; break;
    case 5: src = b.xpos; dst = b.out_xpos; len = b.nbody * 3; src_stride = len; break;
    default: src = b.xquat; dst = b.out_xquat; len = b.nbody * 4; src_stride = len; break;
  }
  trace_copy_words(src + (size_t)s * src_stride, dst + (size_t)row * len, len, threadIdx.x, kTraceThreads);
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

int rmbx_episode_trace(const rmbx_trace_buffers* b, void* stream) {
  RMBX_CHECK_ARG(b != nullptr, "rmbx_episode_trace: bufs is NULL");
  RMBX_CHECK_ARG(b->sched && b->time && b->reward, "rmbx_episode_trace: a schedule / time / reward pointer is NULL");
  RMBX_CHECK_ARG(b->ctrl && b->qpos && b->qvel && b->gxpos && b->gxmat && b->xpos && b->xquat,
                 "rmbx_episode_trace: an engine pointer is NULL");
  RMBX_CHECK_ARG(b->trace_episode && b->trace_step && b->slot_row, "rmbx_episode_trace: a per-slot state pointer is NULL");
  RMBX_CHECK_ARG(b->out_episode && b->out_slot && b->out_step && b->out_phase && b->out_rollout_time_idx &&
                     b->out_flags && b->out_time && b->out_reward && b->out_ctrl && b->out_qpos && b->out_qvel &&
                     b->out_gxpos && b->out_gxmat && b->out_xpos && b->out_xquat && b->rows,
                 "rmbx_episode_trace: a chunk pointer is NULL");
  RMBX_CHECK_ARG(b->stride >= 1, "rmbx_episode_trace: stride must be at least 1 (got %d)", b->stride);
  RMBX_CHECK_ARG(b->capacity >= 1, "rmbx_episode_trace: capacity must be at least 1 (got %d)", b->capacity);
  RMBX_CHECK_ARG(b->n_env >= 0 && b->n_episodes >= 0 && b->n_pre >= 0,
                 "rmbx_episode_trace: negative n_env / n_episodes / n_pre");
  RMBX_CHECK_ARG(b->nq > 0 && b->nv > 0 && b->nu > 0 && b->ngeom > 0 && b->nbody > 0,
                 "rmbx_episode_trace: nq, nv, nu, ngeom and nbody must be positive");
  RMBX_CHECK_ARG(b->ctrl_stride >= b->nu, "rmbx_episode_trace: ctrl_stride is smaller than nu");
  if (b->n_env == 0) return RMBX_OK;
  hipLaunchKernelGGL(episode_trace_index_kernel, dim3(1), dim3(kChunk), 0, stream_of(stream), *b);
  RMBX_CHECK_LAUNCH();
  hipLaunchKernelGGL(episode_trace_copy_kernel, dim3(b->n_env, kTraceArrays), dim3(kTraceThreads), 0,
                     stream_of(stream), *b);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}

}  // extern "C"
