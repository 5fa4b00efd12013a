#!/usr/bin/env python
"""Cost of --dynamics: one run of the bench_policy.py Act workload (Cable x1024, fp32, synthetic
weights, 96 timed RolloutPhase steps after 8 warm-up steps) with the phase split of
common/phase_timer.py, so that the `physics` phase (rmbx_engine_step, 8 substeps) can be compared
between trees and flags.  The package is imported from ROOT, so the same script times another
checkout (the parent commit's tree with its own built library) from this one:

    python scripts/prof_dynamics.py ROOT TAG [--dynamics KEY=VALUE ...]

Prints one JSON line.  BASELINE.md, the --dynamics section; raw runs: profiles/dynamics_bench_ab.txt."""
import importlib
import json
import os
import sys
import time

root, tag = sys.argv[1], sys.argv[2]
extra = sys.argv[3:]
sys.path.insert(0, root)
sys.path.insert(0, root + "/scripts")
import torch  # noqa: E402

import bench_policy as BP  # noqa: E402
import robomanipbaselines_amd  # noqa: E402
from robomanipbaselines_amd.common.phase_timer import PhaseTimer  # noqa: E402

STEPS, WARM = 96, 8


def main():
    a = BP.parse_args(["Act", "--precision", "fp32", "--num_envs", "1024", "--steps", str(STEPS), "--warmup", str(WARM)]
                      + extra)
    mod, cls = BP.POLICIES[a.policy]
    Pol = getattr(importlib.import_module(mod), cls)

    class Rollout(BP.ENVS[a.env], Pol):
        pass

    ro = Rollout(argv=BP.rollout_argv(a))
    ro.args.world_idx_list = [g % 6 for g in range(a.num_envs)]
    ro.reset()
    ro._active = None
    while ro.phase_idx < len(ro.pre_durations):
        ro.step_once()
    for _ in range(WARM):
        ro.step_once()
    timer = PhaseTimer()
    ro.attach_phase_timer(timer)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(STEPS):
        ro.step_once()
    torch.cuda.synchronize()
    dt = time.time() - t0
    ph, _ = timer.summary()
    print(json.dumps({"tag": tag, "package": os.path.relpath(robomanipbaselines_amd.__file__), "dynamics": extra[1:] or None,
                      "ms_per_step": round(dt * 1e3 / STEPS, 3),
                      "phases_ms_per_env_step": {k: round(v / STEPS, 4) for k, v in sorted(ph.items())},
                      "bad_resets": int(ro.env.bad_resets.sum())}), flush=True)


if __name__ == "__main__":
    main()
