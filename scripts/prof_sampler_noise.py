"""Noise preparation per inference of the diffusion samplers: --sampler_noise batch's randn + copy_
into the graph's static buffers against --sampler_noise episode's one rmbx_philox_normal launch
(plus the draw counter's increment), at DP x2048 (100 planes), DP3 x1024 (1 plane) and two more
shapes.  Device events around blocks of 20 calls, the two forms alternated, median of 15 blocks; one
JSON line per shape (profiles/sampler_noise_prep.log).

    python scripts/prof_sampler_noise.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robomanipbaselines_amd import kernels as K  # noqa: E402

DEV = "cuda:0"


def measure(B, nn_, reps=20, blocks=15):
    shape = (B, 16, 7)
    planes = torch.zeros((1 + nn_,) + shape, device=DEV)
    xb, nb = planes[0], (planes[1:] if nn_ else None)
    ep = torch.arange(B, dtype=torch.int32, device=DEV)
    dr = torch.zeros(B, dtype=torch.int32, device=DEV)

    def batch():
        x0 = torch.randn(shape, device=DEV)
        noise = torch.randn((nn_,) + shape, device=DEV) if nn_ else None
        xb.copy_(x0)
        if nb is not None:
            nb.copy_(noise)

    def episode():
        K.philox_normal(3, ep, dr, planes)
        dr.add_(1)

    for f in (batch, episode):
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    t = {"batch": [], "episode": []}
    for _ in range(blocks):
        for name, f in (("batch", batch), ("episode", episode)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    mb = planes.numel() * 4 / 1e6
    out = {"B": B, "planes": 1 + nn_, "MB": round(mb, 2)}
    for name in t:
        a = np.array(t[name])
        out[name + "_us_median"] = round(float(np.median(a)), 2)
        out[name + "_us_min_max"] = [round(float(a.min()), 2), round(float(a.max()), 2)]
    out["episode_GBps"] = round(mb / 1e3 / (out["episode_us_median"] * 1e-6), 1)
    return out


if __name__ == "__main__":
    for B, nn_ in ((2048, 99), (1024, 0), (2048, 0), (3, 99)):
        print(json.dumps(measure(B, nn_)), flush=True)
