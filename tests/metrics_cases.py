"""Numpy / plain-Python f64 model of rmbx_episode_metrics (the slot rule of include/rmbx.h), the
synthetic buffers the kernel is driven with, and the known answers of the host-side summary
helpers; shared by the host and the GPU tests.

The model is written from the header alone: plain Python loops over Python floats (IEEE doubles,
one rounding per operation, no contraction; math.sqrt is correctly rounded), in the kernel's
order."""

import math

import numpy as np

from robomanipbaselines_amd import _native as N

NQ, NV, NU, CTRL_STRIDE, EE_STRIDE, EE_OFF = 11, 9, 7, 8, 17, 5
ARM_QADR = (1, 2, 4, 5, 7, 10)
ARM_DOF = (0, 2, 3, 5, 6, 8)
N_PRE = 3
HIST = 21

F64_FIELDS = ("peak_force", "peak_torque", "peak_joint_speed", "peak_tracking_error", "ee_path", "joint_path",
              "cmd_roughness")
INT_FIELDS = ("episode", "steps", "first_success_step", "flags")
BITWISE_FIELDS = INT_FIELDS + ("peak_joint_speed", "peak_tracking_error", "joint_path", "cmd_roughness")
SQRT_PEAKS = ("peak_force", "peak_torque")
SQRT_SUM = "ee_path"
U = 2.0 ** -53  # unit roundoff of f64


def _norm3(x, y, z):
    return math.sqrt((x * x + y * y) + z * z)


def _max(cur, x):
    return x if x > cur else cur


def empty_table(n_episodes):
    return np.zeros(n_episodes, dtype=N.METRICS_DTYPE)


def metrics_model(table, hist, call, n_pre=N_PRE, episode_base=0, arm_qadr=ARM_QADR, arm_dof=ARM_DOF):
    """One call of rmbx_episode_metrics on copies of (table, hist).  call: dict of the per-slot
    arrays sched (N.SCHED_DTYPE), active / slot_episode / bad_resets (arrays or None), reward, qpos
    [n, nq], qvel [n, nv], ctrl [n, >= 6], sensordata [n, 6], ee [n, 3].  Returns (table, hist,
    counted): counted[s] is True where slot s passed rule 1 (whether or not the guard stopped it)."""
    table, hist = table.copy(), hist.copy()
    sched = call["sched"]
    n = len(sched)
    counted = np.zeros(n, bool)
    for s in range(n):
        if call["active"] is not None and call["active"][s] == 0:
            continue
        if int(sched["phase"][s]) != n_pre or sched["done"][s]:
            continue
        ep = int(call["slot_episode"][s]) if call["slot_episode"] is not None else episode_base + s
        local = ep - episode_base
        if local < 0 or local >= len(table):
            continue
        counted[s] = True
        r = table[local]
        if call["bad_resets"] is not None and call["bad_resets"][s] > 0:
            if r["steps"] != 0:
                r["flags"] |= 1
            continue
        k = int(r["steps"]) + 1
        f = [float(x) for x in call["sensordata"][s]]
        q = [float(call["qpos"][s][a]) for a in arm_qadr]
        v = [float(call["qvel"][s][a]) for a in arm_dof]
        u = [float(call["ctrl"][s][j]) for j in range(6)]
        p = [float(x) for x in call["ee"][s]]
        h = [float(x) for x in hist[s]]
        if k == 1:
            r["episode"] = ep
        if r["first_success_step"] == 0 and float(call["reward"][s]) > 0.0:
            r["first_success_step"] = k
        r["peak_force"] = _max(float(r["peak_force"]), _norm3(f[0], f[1], f[2]))
        r["peak_torque"] = _max(float(r["peak_torque"]), _norm3(f[3], f[4], f[5]))
        speed, err = float(r["peak_joint_speed"]), float(r["peak_tracking_error"])
        for j in range(6):
            speed = _max(speed, abs(v[j]))
            err = _max(err, abs(u[j] - q[j]))
        r["peak_joint_speed"], r["peak_tracking_error"] = speed, err
        if k >= 2:
            r["ee_path"] = float(r["ee_path"]) + _norm3(p[0] - h[0], p[1] - h[1], p[2] - h[2])
            dq = 0.0
            for j in range(6):
                dq = dq + abs(q[j] - h[3 + j])
            r["joint_path"] = float(r["joint_path"]) + dq
        if k >= 3:
            rough = 0.0
            for j in range(6):
                d = (u[j] - 2.0 * h[9 + j]) + h[15 + j]
                rough = rough + d * d
            r["cmd_roughness"] = float(r["cmd_roughness"]) + rough
        r["steps"] = k
        hist[s, 0:3] = p
        hist[s, 15:21] = u if k == 1 else h[9:15]
        hist[s, 9:15] = u
        hist[s, 3:9] = q
    return table, hist, counted


# -- synthetic calls of the GPU test ----------------------------------------------------------------
N_EPISODES, EPISODE_BASE, N_CALLS = 9, 10, 7


def make_calls(n, addressed, seed=0):
    """N_CALLS consecutive calls for n slots with fresh random state each.  addressed: True = through
    a slot_episode map (streaming), False = slot_episode NULL (lockstep: slot s is episode
    EPISODE_BASE + s).  Slot kinds, by slot index (those below n exist):
      0 counted in every call (one NaN force row, call 2)     1 inactive (its row stays empty)
      2 bad_resets > 0 from call 3 on (after counted steps)   3 changes episode between calls 3 and 4
      4 in a pre-motion phase for two calls, then counted     5 done
      6 slot_episode -1                                       7 / 8 an episode above / below the table
      9 bad_resets > 0 from the start (its row stays empty)   256 counted (the second block)
      the rest: random phase / mask, episodes outside the table.
    With slot_episode NULL the kinds that need the map (3, 6, 7, 8) are plain counted slots, slot 8
    is past RolloutPhase and slots >= N_EPISODES fall outside the table by their index."""
    rng = np.random.default_rng(100 * n + seed + (7 if addressed else 0))
    calls = []
    for c in range(N_CALLS):
        sched = np.zeros(n, dtype=N.SCHED_DTYPE)
        sched["phase"] = N_PRE
        active = np.ones(n, np.uint8)
        bad = np.zeros(n, np.int32)
        ep = 100 + np.arange(n, dtype=np.int32)  # outside the table
        rest = np.arange(n) >= 10
        sched["phase"][rest] = rng.integers(0, N_PRE + 2, int(rest.sum()))
        active[rest] = rng.integers(0, 2, int(rest.sum()))
        for s, e in ((0, 10), (1, 11), (2, 12), (3, 13 if c < 3 else 14), (4, 15), (5, 16), (6, -1), (7, 19), (8, 3),
                     (9, 17), (256, 18)):
            if s < n:
                ep[s] = e
        if n > 1:
            active[1] = 0
        if n > 2 and c >= 3:
            bad[2] = 1 + c
        if n > 4 and c < 2:
            sched["phase"][4] = N_PRE - 1
        if n > 5:
            sched["done"][5] = 1
        if n > 8 and not addressed:
            sched["phase"][8] = N_PRE + 1
        if n > 9:
            bad[9] = 1
        if n > 256:
            sched["phase"][256], active[256] = N_PRE, 1
        sd = rng.normal(0, 20, (n, 6))
        if c == 2:
            sd[0, 1] = np.nan
        calls.append({
            "sched": sched, "active": active, "slot_episode": ep if addressed else None, "bad_resets": bad,
            "reward": np.where(rng.random(n) < 0.3, 1.0, 0.0) * (c >= 2), "qpos": rng.normal(0, 1, (n, NQ)),
            "qvel": rng.normal(0, 2, (n, NV)), "ctrl": rng.normal(0, 1, (n, CTRL_STRIDE)), "sensordata": sd,
            "ee_buf": rng.normal(0, 0.5, (n, EE_STRIDE)),
        })
        calls[-1]["ee"] = calls[-1]["ee_buf"][:, EE_OFF: EE_OFF + 3]
    return calls


def sqrt_field_bars(table):
    """The derived bars of the fields that take a square root, relative to the model's value: one
    rounding per operation is assumed, so a norm differs from the model's by at most a few u
    (three squares, two adds, the root) and a sum of K of them by 4 K u; a peak is one of them."""
    return {"peak_force": 4 * U, "peak_torque": 4 * U, "ee_path": 4 * np.maximum(table["steps"], 1) * U}


# -- known answers of the host-side helpers ---------------------------------------------------------
Z95 = 1.959963984540054
WILSON_0_OF_10 = (0.0, Z95 * Z95 / (10 + Z95 * Z95))  # p = 0: [0, z^2 / (n + z^2)]
_H = Z95 / (2 * math.sqrt(100 + Z95 * Z95))  # p = 1/2: 1/2 +- z / (2 sqrt(n + z^2))
WILSON_50_OF_100 = (0.5 - _H, 0.5 + _H)
