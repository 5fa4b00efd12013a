"""Shared cases of the --dynamics tests (tests/test_dynamics.py on the host, tests/test_dynamics_gpu.py
on the device): the scale rows handed to the engine, the states each row's own scaled oracle warms, an
independent scalar restatement of the draw, and the start of the test-power check."""

import functools

import numpy as np

SEED = 0x1234567855AA33CC
# episodes of the draw tests: 0, a retired slot's -1 and the largest i32 among them
EPISODES = np.array([0, 1, -1, 2**31 - 1, 7, 1000003, 5999], dtype=np.int32)
STRENGTHS = dict(friction=0.3, damping=0.5, mass=0.25, gain=0.1)

INIT = [np.pi, -np.pi / 2, -0.75 * np.pi, -0.25 * np.pi, np.pi / 2, np.pi / 2]

# the rows of the engine tests (friction, damping, mass, gain): nominal, each factor alone, all four
ROWS = np.array([
    [1.0, 1.0, 1.0, 1.0],
    [0.5, 1.0, 1.0, 1.0],
    [1.0, 2.0, 1.0, 1.0],
    [1.0, 1.0, 2.0, 1.0],
    [1.0, 1.0, 1.0, 0.8],
    [2.0, 0.5, 0.5, 1.25],
], dtype=np.float64)
WARM = (0, 5, 10)  # env-steps each row's own scaled oracle runs before the comparison starts

# engine-vs-oracle bars on identical states, those of tests/test_engine_gpu.py (BAR_QACC, BAR_SENSOR,
# BAR_QVEL1, BAR_QPOS1, BAR_TRAJ_ALL and the mass-matrix / actuator tolerances of
# test_forward_matches_oracle), restated: a scaled env is held to what the nominal model is held to
BAR_QACC = 1e-9
BAR_SENSOR = 1e-11
BAR_QVEL1 = 1e-10
BAR_QPOS1 = 1e-12
BAR_TRAJ_ALL = 1e-9
M_RTOL, M_ATOL = 1e-10, 1e-12
ACT_TOL = 1e-12


def f32(x):
    return float(np.float32(x))


# -- an independent restatement of the draw: scalar Python integers, no numpy arrays ---------------------
def philox_block(c0, c1, c2, c3, seed):
    """Philox4x32-10 of counter (c0, c1, c2, c3) under the 64-bit key seed, on Python ints."""
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    k0, k1 = seed & mask, (seed >> 32) & mask
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & mask, (p0 >> 32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return c0, c1, c2, c3


def scale_row(seed, episode, strengths):
    """One row of the rule of include/rmbx.h (rmbx_dynamics_draw) for f32 strengths [4], with exact
    rational arithmetic up to the one f64 rounding of each operation."""
    from fractions import Fraction

    w = philox_block(0, 0x40000700, 0, int(episode) & 0xFFFFFFFF, int(seed))
    row = []
    for S, word in zip(strengths, w):
        S = np.float32(S)
        if S == 0:
            row.append(1.0)
            continue
        u = Fraction(2 * (word >> 9) + 1, 2**24)  # ((w >> 9) + 0.5) * 2^-23, exact in f32
        sym = 2 * u - 1  # exact in f32: an odd multiple of 2^-23 below 1 in magnitude
        assert float(np.float32(float(sym))) == float(sym)
        prod = Fraction(float(S)) * sym  # 24 x 24 bits: exact in f64
        assert Fraction(float(prod)) == prod
        row.append(1.0 + float(prod))  # the one rounding
    return row


# -- scaled oracles ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cable():
    from robomanipbaselines_amd import model as MD
    from robomanipbaselines_amd.common import dynamics as DY
    from robomanipbaselines_amd.envs.ur5e_base import ARM_JOINTS

    arrays = MD.load("ur5e_cable")
    return arrays, DY.object_bodies(arrays, ARM_JOINTS[0])


def oracle_for(row):
    """An OracleEnv of the cable model scaled by `row`, as the engine scales an env."""
    from oracle.dyn import OracleEnv
    from robomanipbaselines_amd.common import dynamics as DY

    arrays, group = cable()
    return OracleEnv(DY.scaled_arrays(arrays, row, group))


def start_state(arrays, ctrl_offset, grip):
    qpos = arrays["qpos0"].copy()
    qpos[:6] = INIT
    ctrl = np.concatenate([np.array(INIT) + ctrl_offset, [grip]])
    return qpos, ctrl


@functools.lru_cache(maxsize=None)
def states():
    """(t, qpos, qvel, qacc_ws, ctrl) per row of ROWS: the nominal start under ctrl = INIT + offsets,
    warmed WARM[i % 3] env-steps by the row's own scaled oracle.  Computed once."""
    arrays, _ = cable()
    rng = np.random.default_rng(11)
    out = []
    for i, row in enumerate(ROWS):
        o = oracle_for(row)
        qpos, ctrl = start_state(arrays, rng.normal(0, 0.05, 6), float(rng.uniform(100, 255)))
        o.set_state(0.0, qpos, np.zeros(o.nv), np.zeros(o.nv), ctrl)
        for _ in range(WARM[i % len(WARM)]):
            assert o.step(8) == 0
        t, qp, qv, qa = o.state()
        out.append((t, qp, qv, qa, ctrl))
    return out


def oracle_at(row, state):
    o = oracle_for(row)
    t, qp, qv, qa, c = state
    o.set_state(t, qp, qv, qa, c)
    return o


@functools.lru_cache(maxsize=None)
def trajectories(steps):
    """qpos [rows, steps, nq] of each row's scaled oracle from states(), and of the NOMINAL oracle from
    the same states: how far the scaling moves each row.  Computed once."""
    scaled, nominal = [], []
    for row, s in zip(ROWS, states()):
        for dst, r in ((scaled, row), (nominal, ROWS[0])):
            o, traj = oracle_at(r, s), []
            for _ in range(steps):
                assert o.step(8) == 0
                traj.append(o.state()[1].copy())
            dst.append(np.array(traj))
    return np.array(scaled), np.array(nominal)
