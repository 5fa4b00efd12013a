"""Measure the cost of the episode trace (--trace_dir): Cable x n envs, SARNN and ACT, streaming.

(a) ms per env-step of run_streaming() capped at --steps env-steps with tracing off, at stride 1
    with every episode, and at stride = --skip, the three alternated --runs times; with the host
    time of the flushes (one every 16 steps) and the rows and bytes that went to the trace directory.
(b) the trace kernels alone: rmbx_episode_trace on the run's own buffers with every slot writing a
    row, HIP events around --kernel_calls calls, against the bytes it moves (a row read + a row written).

Prints one JSON line per measurement; --log appends them to a file.

    python scripts/prof_trace.py --num_envs 1024 --policies Sarnn Act --log profiles/trace_cost.log
"""

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compose(policy):
    from robomanipbaselines_amd.envs.operation.OperationMujocoUR5eCable import OperationMujocoUR5eCable

    if policy == "Sarnn":
        from robomanipbaselines_amd.policy.sarnn.rollout_sarnn import RolloutSarnn as P
    else:
        from robomanipbaselines_amd.policy.act.rollout_act import RolloutAct as P

    class Rollout(OperationMujocoUR5eCable, P):
        pass

    return Rollout


def quiet_run(ro):
    out, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        return ro.run()
    finally:
        sys.stdout.close()
        sys.stdout = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=1024)
    ap.add_argument("--policies", nargs="+", default=["Sarnn", "Act"], choices=["Sarnn", "Act"])
    ap.add_argument("--steps", type=int, default=96, help="env-steps per run (a multiple of 16: whole poll periods)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernel_calls", type=int, default=64)
    ap.add_argument("--trace_root", type=str, default=None, help="where the traces go (default: a temporary directory)")
    ap.add_argument("--log", type=str, default=None)
    a = ap.parse_args()
    n = a.num_envs
    os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", "0")
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    root = a.trace_root or tempfile.mkdtemp(prefix="rmbx_trace_")
    for policy in a.policies:
        ro = compose(policy)(argv=["--num_envs", str(n), "--num_episodes", str(n), "--world_idx_list", "0", "1", "2", "3",
                                   "4", "5", "--max_steps", str(a.steps)])
        skip = int(ro.args.skip)
        modes = (("off", None), ("stride1", 1), (f"stride{skip}", skip))
        ro.args.max_steps = 32  # warm-up: allocations, first launches
        quiet_run(ro)
        ro.args.max_steps = a.steps
        ms = {m: [] for m, _ in modes}
        for i in range(a.runs):
            for mode, stride in modes:
                d = os.path.join(root, f"{policy}_{mode}_{i}")
                ro.args.trace_dir, ro.args.trace_stride = (None, 1) if stride is None else (d, stride)
                ro.result = {k: [] for k in ("success", "reward", "duration")}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = quiet_run(ro)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                rec = {"part": "loop", "policy": policy, "mode": mode, "run": i, "n": n, "steps": steps,
                       "ms_per_step": round(1e3 * wall / steps, 4)}
                if stride is not None:
                    w = ro.last_trace
                    fl = np.array(w.flush_seconds[:-1] or w.flush_seconds)  # (the last one is finish()'s remainder)
                    rec.update(rows=w.rows_written, row_bytes=w.trace.row_bytes,
                               trace_mib=round(w.rows_written * w.trace.row_bytes / 2**20, 1),
                               flush_ms_mean=round(1e3 * float(fl.mean()), 3), flush_ms_max=round(1e3 * float(fl.max()), 3),
                               flushes=len(w.flush_seconds))
                    shutil.rmtree(d, ignore_errors=True)
                ms[mode].append(rec["ms_per_step"])
                emit(rec)
        off = np.array(ms["off"])
        emit({"part": "loop", "summary": True, "policy": policy, "n": n, "steps": a.steps,
              **{m + "_ms_per_step": v for m, v in ms.items()}, "off_spread_ms": round(float(off.max() - off.min()), 4),
              **{m + "_minus_off_ms": round(float(np.median(v) - np.median(off)), 4) for m, v in ms.items() if m != "off"}})
        # (b) the kernels alone, every slot writing a row
        from robomanipbaselines_amd import kernels as K

        tr = K.EpisodeTrace(ro.sched, ro.env.engine, n, len(ro.pre_durations))
        ro.sched.zero_()  # nobody is done: the slots keep stepping
        reward = torch.zeros(n, dtype=torch.float64, device=ro.device)
        for _ in range(3):
            tr.record(None, reward)
        tr.rows.zero_()
        times = []
        for c in range(a.kernel_calls):
            if c % K.TRACE_POLL_STEPS == 0:
                tr.rows.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.record(None, reward)
            e1.record()
            times.append((e0, e1))
        torch.cuda.synchronize()
        assert tr.rows.cpu().tolist()[1] == 0
        us = np.array([1e3 * x.elapsed_time(y) for x, y in times])
        moved = 2 * n * tr.row_bytes
        emit({"part": "kernel", "policy": policy, "n": n, "row_bytes": tr.row_bytes, "calls": a.kernel_calls,
              "us_per_call_median": round(float(np.median(us)), 2), "us_per_call_min": round(float(us.min()), 2),
              "us_per_call_max": round(float(us.max()), 2), "bytes_moved_per_call": moved,
              "gb_per_s_at_median": round(moved / float(np.median(us)) / 1e3, 1)})
        del ro, tr
        torch.cuda.empty_cache()
    if a.trace_root is None:
        shutil.rmtree(root, ignore_errors=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
