// Per-episode rollout metrics (--episode_metrics, rmbx_episode_metrics): every slot in RolloutPhase
// folds its env-step into the row of the episode it holds -- the slot rule of include/rmbx.h.
//
// Latency-bound bookkeeping over n_env slots: plain C++, one thread per slot, no atomics, no LDS,
// vector stores only.  An episode is held by one slot at a time, so its row and the slot's history
// are read and written by one thread, in step order; f64 throughout, no contraction.

#include "rmbx_common.h"

#pragma clang fp contract(off)

namespace rmbx {

static inline hipStream_t metrics_stream_of(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kMetricsThreads = 256;

__device__ __forceinline__ double metrics_max(double cur, double x) { return x > cur ? x : cur; }

__device__ __forceinline__ double metrics_norm3(double x, double y, double z) {
  return sqrt((x * x + y * y) + z * z);
}

__global__ void __launch_bounds__(kMetricsThreads) episode_metrics_kernel(rmbx_metrics_buffers b) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= b.n_env) return;
  if (b.active && b.active[s] == 0) return;
  const rmbx_sched_t v = b.sched[s];
  if (v.phase != b.n_pre || v.done) return;
  const int32_t ep = b.slot_episode ? b.slot_episode[s] : b.episode_base + s;
  const int64_t local = (int64_t)ep - b.episode_base;
  if (local < 0 || local >= b.n_episodes) return;
  rmbx_episode_metrics_t* row = b.table + local;
  rmbx_episode_metrics_t r = *row;
  if (b.bad_resets && b.bad_resets[s] > 0) {
    if (r.steps != 0) row->flags = r.flags | RMBX_METRICS_BAD_STATE;
    return;
  }
  const int32_t k = r.steps + 1;
  const double* qpos = b.qpos + (size_t)s * b.nq;
  const double* qvel = b.qvel + (size_t)s * b.nv;
  const double* ctrl = b.ctrl + (size_t)s * b.ctrl_stride;
  const double* sd = b.sensordata + (size_t)s * 6;
  const double* ee = b.ee_pos + (size_t)s * b.ee_stride;
  double* h = b.hist + (size_t)s * RMBX_METRICS_HIST;  // p'(3) q'(6) u'(6) u''(6)
  double p[3], q[6], u[6];
  for (int i = 0; i < 3; ++i) p[i] = ee[i];
  for (int j = 0; j < 6; ++j) {
    q[j] = qpos[b.arm_qadr[j]];
    u[j] = ctrl[j];
  }
  if (k == 1) r.episode = ep;
  if (r.first_success_step == 0 && b.reward[s] > 0.0) r.first_success_step = k;
  r.peak_force = metrics_max(r.peak_force, metrics_norm3(sd[0], sd[1], sd[2]));
  r.peak_torque = metrics_max(r.peak_torque, metrics_norm3(sd[3], sd[4], sd[5]));
  for (int j = 0; j < 6; ++j) {
    r.peak_joint_speed = metrics_max(r.peak_joint_speed, fabs(qvel[b.arm_dof[j]]));
    r.peak_tracking_error = metrics_max(r.peak_tracking_error, fabs(u[j] - q[j]));
  }
  if (k >= 2) {
    r.ee_path += metrics_norm3(p[0] - h[0], p[1] - h[1], p[2] - h[2]);
    double dq = 0.0;
    for (int j = 0; j < 6; ++j) dq += fabs(q[j] - h[3 + j]);
    r.joint_path += dq;
  }
  if (k >= 3) {
    double rough = 0.0;
    for (int j = 0; j < 6; ++j) {
      const double d = (u[j] - 2.0 * h[9 + j]) + h[15 + j];
      rough += d * d;
    }
    r.cmd_roughness += rough;
  }
  r.steps = k;
  for (int i = 0; i < 3; ++i) h[i] = p[i];
  for (int j = 0; j < 6; ++j) {
    h[15 + j] = k == 1 ? u[j] : h[9 + j];
    h[9 + j] = u[j];
    h[3 + j] = q[j];
  }
  *row = r;
}

}  // namespace rmbx

using namespace rmbx;

extern "C" {

int rmbx_episode_metrics(const rmbx_metrics_buffers* b, void* stream) {
  RMBX_CHECK_ARG(b != nullptr, "rmbx_episode_metrics: bufs is NULL");
  RMBX_CHECK_ARG(b->sched && b->reward, "rmbx_episode_metrics: a schedule / reward pointer is NULL");
  RMBX_CHECK_ARG(b->qpos && b->qvel && b->ctrl && b->sensordata && b->ee_pos,
                 "rmbx_episode_metrics: an engine pointer is NULL");
  RMBX_CHECK_ARG(b->table && b->hist, "rmbx_episode_metrics: the table / history pointer is NULL");
  RMBX_CHECK_ARG(b->n_env >= 0 && b->n_episodes >= 0 && b->n_pre >= 0,
                 "rmbx_episode_metrics: negative n_env / n_episodes / n_pre");
  RMBX_CHECK_ARG(b->nq > 0 && b->nv > 0, "rmbx_episode_metrics: nq and nv must be positive");
  RMBX_CHECK_ARG(b->nu >= 6, "rmbx_episode_metrics: nu must be at least 6, the arm's actuators (got %d)", b->nu);
  RMBX_CHECK_ARG(b->ctrl_stride >= b->nu, "rmbx_episode_metrics: ctrl_stride is smaller than nu");
  RMBX_CHECK_ARG(b->ee_stride >= 3, "rmbx_episode_metrics: ee_stride must be at least 3 (got %d)", b->ee_stride);
  for (int j = 0; j < 6; ++j) {
    RMBX_CHECK_ARG(b->arm_qadr[j] >= 0 && b->arm_qadr[j] < b->nq,
                   "rmbx_episode_metrics: arm_qadr[%d] = %d is out of range [0, %d)", j, b->arm_qadr[j], b->nq);
    RMBX_CHECK_ARG(b->arm_dof[j] >= 0 && b->arm_dof[j] < b->nv,
                   "rmbx_episode_metrics: arm_dof[%d] = %d is out of range [0, %d)", j, b->arm_dof[j], b->nv);
  }
  if (b->n_env == 0) return RMBX_OK;
  hipLaunchKernelGGL(episode_metrics_kernel, dim3((b->n_env + kMetricsThreads - 1) / kMetricsThreads),
                     dim3(kMetricsThreads), 0, metrics_stream_of(stream), *b);
  RMBX_CHECK_LAUNCH();
  return RMBX_OK;
}

}  // extern "C"
