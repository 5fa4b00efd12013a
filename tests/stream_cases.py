"""Numpy models of the episode-streaming kernels (include/rmbx.h: rmbx_sched_phases,
rmbx_sched_close_bad, rmbx_episode_recycle), shared by the host and the GPU tests, and the
synthetic buffers the recycle kernel is driven with."""

import numpy as np

from robomanipbaselines_amd import _native as N

NQ, NV, NU, CTRL_STRIDE, NBODY = 11, 9, 7, 8, 5


def sched_phases_model(sched, prev_phase):
    """(phase, entered, new prev_phase) of rmbx_sched_phases."""
    phase = sched["phase"].astype(np.int32)
    return phase, (phase != prev_phase).astype(np.uint8), phase.copy()


def close_bad_model(sched, time, bad_resets, last_elapsed, n_pre):
    """rmbx_sched_close_bad on copies: returns (sched, last_elapsed)."""
    sched, last_elapsed = sched.copy(), last_elapsed.copy()
    for e in range(len(sched)):
        if sched["done"][e]:
            continue
        if bad_resets[e] > 0:
            sched["done"][e], sched["phase"][e], sched["success"][e] = 1, n_pre + 1, 0
            sched["result_reward"][e], sched["duration"][e] = 0.0, last_elapsed[e]
        else:
            last_elapsed[e] = time[e] - sched["phase_start"][e] if sched["phase"][e] == n_pre else 0.0
    return sched, last_elapsed


def make_state(n, M, done, next_local, episode_base=10, seed=0, world_body=2, world_qadr=-1):
    """Synthetic schedule / engine / motion / queue buffers (numpy, random contents) for n slots
    and M queued episodes of which `next_local` have been handed out; done: bool [n]."""
    rng = np.random.default_rng(seed + 7 * n + M)
    sched = np.zeros(n, dtype=N.SCHED_DTYPE)
    sched["phase"] = np.where(done, 5, rng.integers(0, 5, n))
    sched["rollout_time_idx"] = rng.integers(0, 900, n)
    sched["done"] = done
    sched["success"] = rng.integers(0, 2, n)
    sched["has_success_time"] = sched["success"]
    for f in ("phase_start", "success_time", "result_reward", "duration"):
        sched[f] = rng.random(n)
    # the slots hold distinct episodes among those already handed out
    slot_episode = (episode_base + rng.permutation(max(next_local, n))[:n]).astype(np.int32)
    results = np.zeros(M, dtype=N.EPISODE_DTYPE)
    results["episode"] = -1
    st = {
        "sched": sched, "slot_episode": slot_episode, "recycled": np.full(n, 7, np.uint8),
        "counters": np.array([next_local, 3], np.int32), "results": results,
        "final_qpos": np.full((M, NQ), -1.0), "world_idx": rng.integers(0, 6, M).astype(np.int32),
        "world_pos": rng.random((M, 3)), "time": rng.random(n) * 30, "qpos": rng.random((n, NQ)),
        "qvel": rng.random((n, NV)), "qacc_ws": rng.random((n, NV)), "ctrl": rng.random((n, CTRL_STRIDE)),
        "body_pos": rng.random((n, NBODY, 3)), "stats": rng.integers(0, 9, (n, 4)).astype(np.int32),
        "qpos0": rng.random(NQ), "ctrl0": rng.random(NU), "q_cmd": rng.random((n, 6)), "grip_cmd": rng.random((n, 1)),
        "target_R": rng.random((n, 9)), "target_p": rng.random((n, 3)), "motion0": rng.random(18),
        "bad_resets": rng.integers(0, 2, n).astype(np.int32), "last_elapsed": rng.random(n),
        "episode_base": episode_base, "world_body": world_body, "world_qadr": world_qadr,
    }
    return st


def recycle_model(st):
    """rmbx_episode_recycle on a deep copy of `st` (make_state): finished slots are recorded, given
    the next episodes in increasing slot order and re-armed; returns the new state."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    n, M, base = len(st["sched"]), len(st["results"]), st["episode_base"]
    nxt = int(st["counters"][0])
    handed = 0
    for s in range(n):
        ep = int(st["slot_episode"][s])
        if not st["sched"]["done"][s] or ep < 0:
            st["recycled"][s] = 0
            continue
        old = ep - base
        r = st["results"][old]
        r["episode"], r["slot"], r["world_idx"] = ep, s, st["world_idx"][old]
        r["rollout_time_idx"], r["success"] = st["sched"]["rollout_time_idx"][s], st["sched"]["success"][s]
        r["bad_state"] = 1 if st["bad_resets"][s] > 0 else 0
        r["reward"], r["duration"] = st["sched"]["result_reward"][s], st["sched"]["duration"][s]
        st["final_qpos"][old] = st["qpos"][s]
        new = nxt + handed
        handed += 1
        if new >= M:
            st["slot_episode"][s] = -1
            st["recycled"][s] = 0
            continue
        st["sched"][s] = np.zeros((), dtype=N.SCHED_DTYPE)
        st["time"][s] = 0.0
        st["qpos"][s] = st["qpos0"]
        st["qvel"][s] = 0.0
        st["qacc_ws"][s] = 0.0
        st["ctrl"][s, :NU] = st["ctrl0"]
        st["stats"][s] = 0
        st["q_cmd"][s], st["target_R"][s], st["target_p"][s] = st["motion0"][:6], st["motion0"][6:15], st["motion0"][15:]
        st["grip_cmd"][s] = 0.0
        st["bad_resets"][s] = 0
        st["last_elapsed"][s] = 0.0
        if st["world_body"] >= 0:
            st["body_pos"][s, st["world_body"]] = st["world_pos"][new]
        if st["world_qadr"] >= 0:
            st["qpos"][s, st["world_qadr"]: st["world_qadr"] + 3] = st["world_pos"][new]
        st["slot_episode"][s] = base + new
        st["recycled"][s] = 1
    st["counters"][0] = nxt + min(handed, max(M - nxt, 0))
    st["counters"][1] += handed
    return st


STATE_KEYS = ("sched", "slot_episode", "recycled", "counters", "results", "final_qpos", "time", "qpos", "qvel",
              "qacc_ws", "ctrl", "body_pos", "stats", "q_cmd", "grip_cmd", "target_R", "target_p", "bad_resets",
              "last_elapsed")
