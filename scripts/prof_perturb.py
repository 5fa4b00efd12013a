"""Cost of rmbx_image_perturb alone at the benchmark's frame, 1024 x 480 x 640 x 3, every component on:
the 8-bit space-to-depth policy form ACT fp32 reads and the rgb_out frame the policies that crop or
resize read, plus single components for orientation.  Device events around blocks of 5 calls, median of
9 blocks; one JSON line per form with the time and the achieved bytes / s (read + written)
(profiles/perturb_kernel.txt).

    python scripts/prof_perturb.py [--n 1024]
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
ALL = dict(brightness=20.0, contrast=0.3, gain=0.2, noise=6.0, occ_h=120, occ_w=160)
SPECS = {"all": ALL, "noise": dict(noise=6.0), "photo+occluder": dict(ALL, noise=0.0), "none": {}}


def measure(n, H, W, form, spec, reps=5, blocks=9):
    rgb = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=DEV)
    ep = torch.arange(n, dtype=torch.int32, device=DEV)
    dr = torch.zeros(n, dtype=torch.int32, device=DEV)
    if form == "rgb_out":
        out = dict(rgb_out=torch.empty_like(rgb))
        written = rgb.numel()
    else:
        pol = torch.empty((n, H // 2, W // 2, 16), dtype=torch.uint8, device=DEV)
        out = dict(policy=pol, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
        written = pol.numel()

    def call():
        K.image_perturb(rgb, 3, ep, dr, 0, **out, **SPECS[spec])
        dr.add_(3)

    for _ in range(3):
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
        t.append(e0.elapsed_time(e1) / reps)
    a = np.array(t)
    med = float(np.median(a))
    return {"n": n, "H": H, "W": W, "form": form, "spec": spec, "ms_median": round(med, 4),
            "ms_min_max": [round(float(a.min()), 4), round(float(a.max()), 4)],
            "GB_read": round(rgb.numel() / 1e9, 3), "GB_written": round(written / 1e9, 3),
            "TBps": round((rgb.numel() + written) / 1e12 / (med * 1e-3), 3),
            "philox_blocks_G": round(rgb.numel() / 4 / 1e9, 3) if SPECS[spec].get("noise") else 0.0}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1024)
    a = p.parse_args()
    for form in ("u8_s2d", "rgb_out"):
        for spec in SPECS:
            print(json.dumps(measure(a.n, 480, 640, form, spec)), flush=True)


if __name__ == "__main__":
    main()
