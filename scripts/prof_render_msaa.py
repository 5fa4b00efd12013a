"""What 4 samples per pixel cost: per-call time of the rollout's camera renders (Cable, 1024 envs,
480 x 640, the 8-bit space-to-depth policy output) at samples 1 and 4, with shadows off and on, for the
front (world-fixed) and the hand camera, after the short scripted motion of prof_render_shadows.py.
The single-sample call is timed with the static-background cache enabled and disabled
(RMBX_RENDER_CACHE); a 4-sample or shadowed call does not use it.  The policy output alone asks for no
depth, so a 4-sample call is four sample passes and the resolve; `with_depth` adds the depth output
and with it the pixel-centre pass.  HIP events, alternations of all variants in one process; median
and spread (min .. max) per variant."""
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
args = ap.parse_args()

n, dev = args.num_envs, "cuda:0"
env = BatchedMujocoUR5eCableEnv(n, dev)
env.reset()
rng = np.random.default_rng(0)
delta = torch.tensor(rng.uniform(-1.0, 1.0, (n, 6)) * [0.4, 0.3, 0.5, 0.6, 0.3, 0.8], dtype=torch.float64, device=dev)
ctrl0 = env.engine.ctrl.clone()
for k in range(12):
    act = ctrl0.clone()
    act[:, :6] += delta * (k + 1) / 12
    env.step(act)
H, W = env.renderer.height, env.renderer.width
renderers = {(s, sh): Renderer(env.arrays, dev, width=W, height=H, samples=s, shadows=sh)
             for s in (1, 4) for sh in (False, True)}
pol = torch.empty((n, H // 2, W // 2, 16), dtype=torch.uint8, device=dev)
depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.reps


variants = [(cam, s, sh, cache, wd) for cam in ("front", "hand") for (s, sh) in renderers
            for cache in (("1", "0") if (s, sh) == (1, False) else ("0",)) for wd in ((False, True) if s == 4 else (False,))]
res = {v: [] for v in variants}
for rnd in range(args.rounds):
    for v in variants:
        cam, s, sh, cache, wd = v
        os.environ["RMBX_RENDER_CACHE"] = cache
        r = renderers[(s, sh)]
        kw = dict(policy=pol, depth=depth) if wd else dict(policy=pol)
        r.render(env.engine, cam, **kw)  # (warm: the cache of this variant is built)
        res[v].append(timed(lambda: r.render(env.engine, cam, **kw)))
os.environ.pop("RMBX_RENDER_CACHE")
print(json.dumps({"lib": os.environ.get("RMBX_LIB_VARIANT", "in-tree"), "num_envs": n, "image": [H, W],
                  "rounds": args.rounds, "reps": args.reps}), flush=True)
for (cam, s, sh, cache, wd), t in res.items():
    print(json.dumps({"camera": cam, "samples": s, "shadows": "on" if sh else "off",
                      "cache": "enabled" if cache == "1" else "disabled / not used", "with_depth": wd,
                      "ms_per_call_median": round(statistics.median(t), 3), "min": round(min(t), 3),
                      "max": round(max(t), 3)}), flush=True)
for cam in ("front", "hand"):
    renderers[(1, False)].render(env.engine, cam, rgb=rgb)
    one = rgb.clone()
    renderers[(4, False)].render(env.engine, cam, rgb=rgb)
    torch.cuda.synchronize()
    d = (rgb.int() - one.int()).abs().amax(-1)
    print(json.dumps({"camera": cam, "pixels_moved_by_more_than_2_levels": round((d > 2).float().mean().item(), 5),
                      "by_more_than_16": round((d > 16).float().mean().item(), 5)}), flush=True)
