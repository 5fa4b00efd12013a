"""Measure the streaming rollout (--num_episodes) against the lockstep loop: SARNN on the cable
scene, whose policy is cheap, so the loop's own cost shows.

(a) overhead: M = n episodes, nobody succeeds, so both loops step every slot for the full
    episode: ms per env-step of run_streaming() against run(), alternated, --runs each.
(b) benefit: M = 4 n episodes, success forced for half of them (odd episodes) at an
    episode-seeded time in [2 s, 20 s] of the rollout phase by a reward wrapper that belongs to this
    script: wall time of one streaming run against four lockstep rounds at --env_offset 0, n, 2n, 3n.

Prints one JSON line per measurement and a summary line; --log appends them to a file.

    python scripts/bench_stream.py --num_envs 1024 --runs 3 --log profiles/stream_bench.log
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compose():
    from robomanipbaselines_amd.envs.operation.OperationMujocoUR5eCable import OperationMujocoUR5eCable
    from robomanipbaselines_amd.policy.sarnn.rollout_sarnn import RolloutSarnn

    class Rollout(OperationMujocoUR5eCable, RolloutSarnn):
        pass

    return Rollout


class ForcedSuccess:
    """Reward wrapper: episode e (odd) succeeds from t_e seconds of RolloutPhase on, t_e in [2, 20]
    seeded by e.  Reads the episode of each slot from rollout.slot_episode (streaming) or from the
    env offset (lockstep)."""

    def __init__(self, ro):
        self.ro, self.inner, self.enabled = ro, ro.env._get_reward, False
        self.n_pre = len(ro.pre_durations)
        self.local = torch.arange(ro.n, dtype=torch.int64, device=ro.device)
        ro.env._get_reward = self

    def __call__(self):
        r = self.inner()
        sched = getattr(self.ro, "sched", None)
        if not self.enabled or sched is None:
            return r
        ro = self.ro
        ep = ro.slot_episode.to(torch.int64) if ro.args.num_episodes is not None else ro.args.env_offset + self.local
        t_e = 2.0 + 18.0 * ((ep * 2654435761) % 4294967296).to(torch.float64) / 4294967296.0
        phase = sched.view(torch.int32)[:, 0]
        start = sched.view(torch.float64)[:, 2]
        hit = (phase == self.n_pre) & (ep % 2 == 1) & (ro.env.engine.time - start >= t_e)
        return torch.where(hit, torch.ones_like(r), r)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, steps


def quiet_run(ro):
    """ro.run() without the per-episode result lines."""
    out, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        return ro.run()
    finally:
        sys.stdout.close()
        sys.stdout = out


def lockstep(ro, offset):
    ro.args.num_episodes = None
    ro.args.env_offset = ro.env.env_offset = offset
    ro.result = {k: [] for k in ("success", "reward", "duration")}
    return quiet_run(ro)


def streaming(ro, M):
    ro.args.num_episodes, ro.args.episode_offset = M, 0
    ro.args.env_offset = ro.env.env_offset = 0
    ro.result = {k: [] for k in ("success", "reward", "duration")}
    return quiet_run(ro)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max_duration", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=4, help="(b): M = rounds x n")
    ap.add_argument("--benefit_runs", type=int, default=3)
    ap.add_argument("--skip_benefit", action="store_true")
    ap.add_argument("--skip_overhead", action="store_true")
    ap.add_argument("--phases", action="store_true", help="per-phase split of a lockstep round and a streaming run")
    ap.add_argument("--phase_steps", type=int, default=None, help="cap on the env-steps of each --phases run")
    ap.add_argument("--log", type=str, default=None)
    a = ap.parse_args()
    n = a.num_envs
    os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", "0")
    ro = compose()(argv=["--num_envs", str(n), "--num_episodes", str(n), "--max_duration", str(a.max_duration),
                         "--world_idx_list", "0", "1", "2", "3", "4", "5"])
    wrap = ForcedSuccess(ro)
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    # warm-up of both loops (allocations, first launches)
    ro.args.max_steps = 64
    streaming(ro, n)
    lockstep(ro, 0)
    ro.args.max_steps = None
    # (a) overhead
    ms = {"lockstep": [], "streaming": []}
    for i in range(0 if a.skip_overhead else a.runs):
        for mode in ("lockstep", "streaming"):
            wall, steps = timed((lambda: lockstep(ro, 0)) if mode == "lockstep" else (lambda: streaming(ro, n)))
            ms[mode].append(1e3 * wall / steps)
            emit({"part": "overhead", "mode": mode, "run": i, "n": n, "steps": steps, "wall_s": round(wall, 4),
                  "ms_per_step": round(ms[mode][-1], 4)})
    lo, stv = np.array(ms["lockstep"] or [0.0]), np.array(ms["streaming"] or [0.0])
    emit({"part": "overhead", "summary": True, "n": n, "lockstep_ms_per_step": [round(x, 4) for x in lo],
          "streaming_ms_per_step": [round(x, 4) for x in stv], "lockstep_spread_ms": round(float(lo.max() - lo.min()), 4),
          "streaming_minus_lockstep_ms": round(float(np.median(stv) - np.median(lo)), 4)})
    # (b) benefit
    if not a.skip_benefit:
        wrap.enabled = True
        M = a.rounds * n
        walls = {"lockstep_rounds": [], "streaming": []}
        for i in range(a.benefit_runs):
            wall_l, steps_l = 0.0, 0
            succ_l = 0
            for k in range(a.rounds):
                w, s = timed(lambda: lockstep(ro, k * n))
                wall_l, steps_l = wall_l + w, steps_l + s
                succ_l += sum(ro.result["success"])
            walls["lockstep_rounds"].append(wall_l)
            emit({"part": "benefit", "mode": "lockstep_rounds", "run": i, "n": n, "episodes": M, "steps": steps_l,
                  "wall_s": round(wall_l, 3), "successes": succ_l})
            wall_s, steps_s = timed(lambda: streaming(ro, M))
            walls["streaming"].append(wall_s)
            emit({"part": "benefit", "mode": "streaming", "run": i, "n": n, "episodes": M, "steps": steps_s,
                  "wall_s": round(wall_s, 3), "successes": sum(ro.result["success"]),
                  "bad_state_episodes": ro.bad_state_episodes})
        emit({"part": "benefit", "summary": True, "n": n, "episodes": M,
              "lockstep_rounds_wall_s": [round(x, 3) for x in walls["lockstep_rounds"]],
              "streaming_wall_s": [round(x, 3) for x in walls["streaming"]],
              "speedup_median": round(float(np.median(walls["lockstep_rounds"]) / np.median(walls["streaming"])), 3)})
    # where a step's time goes once the slots have desynchronised: the policy / render / physics /
    # glue split (common/phase_timer.py) of one lockstep round and of a streaming run of the same length
    if a.phases:
        from robomanipbaselines_amd.common.phase_timer import PhaseTimer

        wrap.enabled = True
        ro.args.max_steps = a.phase_steps
        for mode in ("lockstep", "streaming"):
            timer = PhaseTimer()
            ro.attach_phase_timer(timer)
            steps = lockstep(ro, 0) if mode == "lockstep" else streaming(ro, a.rounds * n)
            split, total = timer.summary()
            ro.attach_phase_timer(None)
            # the physics segment of every env-step, averaged over buckets of 64 steps: how its cost
            # moves with the phases the slots are in
            phys = [e0.elapsed_time(e1) for (label, e0), (_, e1) in zip(timer.marks, timer.marks[1:])
                    if label == "physics"]
            buckets = [round(float(np.mean(phys[i:i + 64])), 3) for i in range(0, len(phys), 64)]
            emit({"part": "phases", "mode": mode, "n": n, "steps": steps, "window_ms_per_step": round(total / steps, 4),
                  **{k + "_ms_per_step": round(v / steps, 4) for k, v in sorted(split.items())},
                  "physics_ms_by_64_steps": buckets})
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
