"""Numpy model of the episode-trace kernel (include/rmbx.h: rmbx_episode_trace, the row rule),
shared by the host and the GPU tests, and the synthetic buffers the kernel is driven with."""

import numpy as np

from robomanipbaselines_amd import _native as N
from robomanipbaselines_amd.common.episode_trace import FIELDS

# synthetic dimensions: every per-slot row has an odd number of doubles somewhere (nq = 11, nu = 7 of
# a row stride of 8, ngeom * 3 = 15, nbody * 3 = 9), so the 16-byte copy has heads and tails
DIMS = {"nq": 11, "nv": 9, "nu": 7, "ngeom": 5, "nbody": 3}
CTRL_STRIDE = 8
N_PRE = 4  # phase index of RolloutPhase in the synthetic schedules: phase 5 is past it
# the Cable scene's (assets/ur5e_cable.npz)
CABLE_DIMS = {"nq": 69, "nv": 68, "nu": 7, "ngeom": 104, "nbody": 55}

FILL = {np.dtype(np.int32): -77, np.dtype(np.uint8): 0xAB, np.dtype(np.float64): -12345.5}


def new_chunk(rows, dims):
    """Chunk arrays of `rows` rows filled with the guard values of FILL."""
    return {name: np.full((rows,) + shape(dims), FILL[np.dtype(dt)], dtype=dt) for name, (dt, shape) in FIELDS.items()}


def make_state(n, dims, ctrl_stride, seed=0):
    """Per-slot trace state at its start and the random engine arrays of one step."""
    st = {"trace_episode": np.full(n, -1, np.int32), "trace_step": np.zeros(n, np.int32),
          "rows": np.zeros(2, np.int32)}
    st.update(step_inputs(n, dims, ctrl_stride, np.random.default_rng(seed)))
    return st


def step_inputs(n, dims, ctrl_stride, rng):
    """The arrays one env-step leaves: schedule, time, reward and the engine rows (random)."""
    sched = np.zeros(n, dtype=N.SCHED_DTYPE)
    sched["phase"] = rng.integers(0, 6, n)
    sched["rollout_time_idx"] = rng.integers(0, 900, n)
    sched["done"] = rng.random(n) < 0.3
    sched["success"] = rng.random(n) < 0.5
    d = dims
    return {"sched": sched, "time": rng.random(n) * 30, "reward": rng.random(n),
            "bad_resets": (rng.random(n) < 0.3).astype(np.int32),
            "ctrl": rng.random((n, ctrl_stride)), "qpos": rng.random((n, d["nq"])), "qvel": rng.random((n, d["nv"])),
            "gxpos": rng.random((n, d["ngeom"], 3)), "gxmat": rng.random((n, d["ngeom"], 9)),
            "xpos": rng.random((n, d["nbody"], 3)), "xquat": rng.random((n, d["nbody"], 4))}


def trace_model(st, chunk, capacity, dims, slot_episode=None, stepped=None, select=None, episode_base=0,
                n_episodes=0, stride=1, bad_resets=True):
    """rmbx_episode_trace on copies: returns (trace_episode, trace_step, rows, chunk).  `chunk` may
    have more than `capacity` rows (guard rows the call must not touch)."""
    te, ts, rows = st["trace_episode"].copy(), st["trace_step"].copy(), st["rows"].copy()
    chunk = {k: v.copy() for k, v in chunk.items()}
    n = len(te)
    used = int(rows[0])
    for s in range(n):
        ep = int(slot_episode[s]) if slot_episode is not None else episode_base + s
        if ep < 0 or (stepped is not None and not stepped[s]):
            continue
        if select is not None:
            local = ep - episode_base
            if not (0 <= local < n_episodes) or not select[local]:
                continue
        if te[s] != ep:
            te[s], ts[s] = ep, 0
        ts[s] += 1
        k = int(ts[s])
        v = st["sched"][s]
        ended = bool(v["done"]) or v["phase"] > N_PRE  # the episode ended with this step
        if not (k % stride == 0 or ended):
            continue
        if used >= capacity:
            rows[1] = 1
            continue
        r = used
        used += 1
        chunk["episode"][r], chunk["slot"][r], chunk["step"][r] = ep, s, k
        chunk["phase"][r], chunk["rollout_time_idx"][r] = v["phase"], v["rollout_time_idx"]
        flags = (1 if ended else 0) | (2 if v["success"] else 0)
        if ended and bad_resets and st["bad_resets"][s] > 0:
            flags |= 4
        chunk["flags"][r] = flags
        chunk["time"][r], chunk["reward"][r] = st["time"][s], st["reward"][s]
        chunk["ctrl"][r] = st["ctrl"][s, :dims["nu"]]
        for f in ("qpos", "qvel", "gxpos", "gxmat", "xpos", "xquat"):
            chunk[f][r] = st[f][s]
    rows[0] = used
    return te, ts, rows, chunk


def synthetic_rows(dims, episodes, steps, slot=0, seed=0):
    """Host rows {field: array} as a flush would hand them over: for each step of `steps` one row of
    every episode of `episodes` (step-major), random payloads."""
    rng = np.random.default_rng(seed)
    rows = len(episodes) * len(steps)
    out = {}
    for name, (dt, shape) in FIELDS.items():
        if np.dtype(dt) == np.float64:
            out[name] = rng.random((rows,) + shape(dims))
        else:
            out[name] = np.zeros((rows,) + shape(dims), dtype=dt)
    out["episode"][:] = np.tile(np.asarray(episodes, np.int32), len(steps))
    out["step"][:] = np.repeat(np.asarray(steps, np.int32), len(episodes))
    out["slot"][:] = slot + np.tile(np.arange(len(episodes), dtype=np.int32), len(steps))
    return out


def records(episodes):
    g = np.asarray(episodes)
    rec = np.zeros(len(g), dtype=N.EPISODE_DTYPE)
    rec["episode"], rec["slot"], rec["world_idx"] = g, g % 2, g % 3
    rec["success"], rec["reward"], rec["duration"] = g % 3 == 1, (g % 3 == 1).astype(np.float64), 0.032 * (g + 1)
    rec["rollout_time_idx"] = 30 + g
    return rec


def header(dims=DIMS, **over):
    h = {"policy": "Mlp", "env": "MujocoUR5eCable", "model_name": "ur5e_cable", "image_size": [48, 64],
         "camera_names": ["front", "side", "hand"], "seed": 0, "world_idx_list": [0], "world_random_scale": None,
         "skip": 3, "stride": 1, "shadows": "off", "offsamples": "1", "dims": dict(dims)}
    h.update(over)
    return h
