"""Cost of camera jitter rows in the renderer at the benchmark's shape: the Cable scene, 1024 envs,
640 x 480, the policy's 8-bit space-to-depth output; per camera (front: world-fixed, static-background
cache; hand: on the wrist, no cache) the render call with nothing bound, with identity rows bound, with
drawn rows bound and the cache valid, and with drawn rows re-drawn for other episodes before every call
(every env's cache rebuilt: what a recycled slot pays once per episode); plus the draw kernel alone.
Device events around blocks of calls, median of 7 blocks; one JSON line per case (the
--camera_jitter section; profiles/camera_jitter_bench_ab.txt).

    python scripts/prof_camera_jitter.py [--n 1024] [--cameras front hand]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robomanipbaselines_amd import kernels as K  # noqa: E402
from robomanipbaselines_amd import model as MD  # noqa: E402
from robomanipbaselines_amd.common import camera_jitter as CJ  # noqa: E402
from robomanipbaselines_amd.engine import PhysicsEngine  # noqa: E402
from robomanipbaselines_amd.envs.ur5e_cable import CABLE_INIT_QPOS  # noqa: E402
from robomanipbaselines_amd.render import Renderer  # noqa: E402

DEV = "cuda:0"
SPEC = CJ.CameraJitterSpec(pos=float(np.float32(0.02)), rot=3.0, fovy=float(np.float32(0.05)))


def timed(call, reps, blocks=7):
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
    return round(float(np.median(a)), 4), [round(float(a.min()), 4), round(float(a.max()), 4)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1024)
    p.add_argument("--cameras", nargs="+", default=["front", "hand"])
    p.add_argument("--reps", type=int, default=10)
    a = p.parse_args()
    n = a.n
    arrays = MD.load("ur5e_cable")
    eng = PhysicsEngine(arrays, n, DEV)
    q = np.tile(arrays["qpos0"], (n, 1))
    q[:, :14] = CABLE_INIT_QPOS
    q[:, :6] += 0.05 * np.random.default_rng(0).standard_normal((n, 6))  # the arms differ from env to env
    eng.qpos.copy_(torch.from_numpy(q))
    eng.forward()
    torch.cuda.synchronize()
    H, W = 480, 640
    policy = torch.empty((n, H // 2, W // 2, 16), dtype=torch.uint8, device=DEV)
    ncam = len(arrays["names_cam"])
    episode = torch.arange(n, dtype=torch.int32, device=DEV)
    P, T, F = (float(x) for x in SPEC.strengths())
    rows = torch.tensor(CJ.IDENTITY, dtype=torch.float64, device=DEV).repeat(ncam, n, 1).contiguous()

    def draw():
        K.camera_jitter_draw(3, episode, rows, pos=P, tan_half_rot=T, fovy=F)

    med, mm = timed(draw, 50)
    print(json.dumps({"case": "draw kernel alone", "n": n, "ncam": ncam, "ms_per_call_median": med, "ms_min_max": mm}), flush=True)
    for cam in a.cameras:
        rnd = Renderer(arrays, DEV, width=W, height=H)

        def render():
            rnd.render(eng, cam, policy=policy)

        def redraw_and_render():
            episode.add_(n)  # other episodes: every env's row changes, every cache is rebuilt
            draw()
            render()

        cases = []
        cases.append(("nothing bound", timed(render, a.reps)))
        rows.copy_(torch.tensor(CJ.IDENTITY, dtype=torch.float64, device=DEV).expand(ncam, n, 8))
        rnd.bind_camera_rows(rows)
        cases.append(("identity rows bound", timed(render, a.reps)))
        draw()
        cases.append(("drawn rows bound", timed(render, a.reps)))
        cases.append(("drawn rows, re-drawn before every call", timed(redraw_and_render, a.reps)))
        rnd.bind_camera_rows(None)
        cases.append(("nothing bound, again", timed(render, a.reps)))
        for name, (med, mm) in cases:
            print(json.dumps({"case": name, "camera": cam, "n": n, "size": [H, W], "static_cache": cam != "hand",
                              "ms_per_call_median": med, "ms_min_max": mm}), flush=True)


if __name__ == "__main__":
    main()
