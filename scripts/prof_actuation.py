"""Cost of rmbx_action_perturb alone at the benchmark's shape, 1024 rows x 7 action dimensions, every
component on (noise, bias, delay 2, hold), plus single components and the zero spec for orientation.
Device events around blocks of 50 calls, median of 9 blocks; one JSON line per spec (BASELINE.md §3;
profiles/actuation_bench_ab.txt).  At 7168 elements the figure is a launch, not arithmetic.

    python scripts/prof_actuation.py [--n 1024] [--A 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robomanipbaselines_amd import kernels as K  # noqa: E402

DEV = "cuda:0"
ALL = dict(noise=0.05, bias=0.05, delay=2, hold=0.05)
SPECS = {"all": ALL, "noise": dict(noise=0.05), "bias": dict(bias=0.05), "delay": dict(delay=2), "hold": dict(hold=0.05),
         "none": {}}


def measure(n, A, spec, reps=50, blocks=9):
    kw = SPECS[spec]
    D = kw.get("delay", 0)
    f64 = dict(dtype=torch.float64, device=DEV)
    action = torch.randn((n, A), **f64)
    out, ring = torch.zeros((n, A), **f64), torch.zeros((n, D + 1, A), **f64)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    bs, ns = torch.full((A,), 0.005, **f64), torch.full((A,), 0.005, **f64)
    ep = torch.arange(n, dtype=torch.int32, device=DEV)
    r = torch.zeros(n, dtype=torch.int32, device=DEV)

    def call():
        K.action_perturb(action, 3, ep, r, ring, bs, ns, out, mask, skip=3, **kw)
        r.add_(1)

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) / reps * 1e3)
    a = np.array(t)
    return {"n": n, "A": A, "spec": spec, "us_per_call_median": round(float(np.median(a)), 2),
            "us_min_max": [round(float(a.min()), 2), round(float(a.max()), 2)],
            "note": "the call and the r += 1 that follows it, enqueued back to back"}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1024)
    p.add_argument("--A", type=int, default=7)
    a = p.parse_args()
    for spec in SPECS:
        print(json.dumps(measure(a.n, a.A, spec)), flush=True)


if __name__ == "__main__":
    main()
