"""What the renderer's shadows cost: per-call time of the rollout's camera renders (Cable, 1024 envs,
480 x 640, the 8-bit space-to-depth policy output) with shadows off and on, with the
static-background cache enabled and disabled (RMBX_RENDER_CACHE), for the front (world-fixed) and the
hand camera, after a short scripted motion that spreads the arms over the table.  HIP events, three
alternations of all variants in one process; median and spread (min .. max) per variant.

--off_only: time only the shadows-off variants (for the A/B of the default path against another
build of the library: run it alternately with RMBX_LIB_VARIANT=<name> set and unset)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robomanipbaselines_amd.envs.ur5e_cable import BatchedMujocoUR5eCableEnv  # noqa: E402
from robomanipbaselines_amd.render import Renderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--num_envs", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--off_only", action="store_true")
args = ap.parse_args()

n, dev = args.num_envs, "cuda:0"
env = BatchedMujocoUR5eCableEnv(n, dev)
env.reset()
# scripted motion: every env's arm driven from the initial pose towards its own target over the table
rng = np.random.default_rng(0)
delta = torch.tensor(rng.uniform(-1.0, 1.0, (n, 6)) * [0.4, 0.3, 0.5, 0.6, 0.3, 0.8], dtype=torch.float64, device=dev)
ctrl0 = env.engine.ctrl.clone()
for k in range(12):
    act = ctrl0.clone()
    act[:, :6] += delta * (k + 1) / 12
    env.step(act)
H, W = env.renderer.height, env.renderer.width
renderers = {"off": env.renderer}
if not args.off_only:
    renderers["on"] = Renderer(env.arrays, dev, width=W, height=H, shadows=True)
pol = torch.empty((n, H // 2, W // 2, 16), dtype=torch.uint8, device=dev)
rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.reps


variants = [(cam, sh, cache) for cam in ("front", "hand") for sh in renderers for cache in ("1", "0")]
res = {v: [] for v in variants}
for rnd in range(args.rounds):
    for cam, sh, cache in variants:
        os.environ["RMBX_RENDER_CACHE"] = cache
        r = renderers[sh]
        r.render(env.engine, cam, policy=pol)  # (warm: the cache of this variant is built)
        res[(cam, sh, cache)].append(timed(lambda: r.render(env.engine, cam, policy=pol)))
os.environ.pop("RMBX_RENDER_CACHE")
print(json.dumps({"lib": os.environ.get("RMBX_LIB_VARIANT", "in-tree"), "num_envs": n, "image": [H, W],
                  "rounds": args.rounds, "reps": args.reps}), flush=True)
for (cam, sh, cache), v in res.items():
    print(json.dumps({"camera": cam, "shadows": sh, "cache": "enabled" if cache == "1" else "disabled",
                      "ms_per_call_median": round(statistics.median(v), 3), "min": round(min(v), 3),
                      "max": round(max(v), 3)}), flush=True)
if not args.off_only:
    for cam in ("front", "hand"):
        renderers["off"].render(env.engine, cam, rgb=rgb)
        off = rgb.clone()
        renderers["on"].render(env.engine, cam, rgb=rgb)
        torch.cuda.synchronize()
        ch = ((rgb.int() - off.int()).abs().amax(-1) > 2).float().mean().item()
        print(json.dumps({"camera": cam, "pixels_the_shadow_changes": round(ch, 5)}), flush=True)
