"""Shared cases of the --camera_jitter tests (tests/test_camera_jitter.py on the host,
tests/test_camera_jitter_gpu.py on the device): the draw's episodes and strengths, an independent
scalar restatement of the draw, the jitter rows handed to the renderer (identity, each component
alone, the spec's extremes, a drawn one), the synthetic scene they are rendered on, and a camera built
from rotation matrices -- not from the restated quaternion product -- for the known answers and the
oracle.  Plain module: importing it needs neither torch nor a GPU."""

import math

import numpy as np

import render_cases as RC
from dynamics_cases import philox_block

SEED = 0x0F1E2D3C4B5A6978
PLANE = 0x40000800
# episodes of the draw tests: 0, a retired slot's -1 and the largest i32 among them
EPISODES = np.array([0, 1, -1, 2**31 - 1, 7, 1000003, 5999], dtype=np.int32)
STRENGTHS = dict(pos=0.02, rot=3.0, fovy=0.05)
T_MAX = np.float32(math.tan(math.radians(30.0) / 2.0))  # the largest tan_half_rot the call accepts
W, H = 96, 72


def f32(x):
    return float(np.float32(x))


# -- an independent restatement of the draw: scalar Python integers, exact rationals -----------------------
def _sym(S, word):
    """(double)S * (double)(2 u(w) - 1) with the bracket in f32: both factors and the product are exact."""
    from fractions import Fraction

    S = np.float32(S)
    if S == 0:
        return 0.0
    sym = 2 * Fraction(2 * (word >> 9) + 1, 2**24) - 1  # exact in f32
    assert float(np.float32(float(sym))) == float(sym)
    prod = Fraction(float(S)) * sym  # 24 x 24 bits: exact in f64
    assert Fraction(float(prod)) == prod
    return float(prod)


def jitter_row(seed, episode, camera, P, T, F):
    """One row of the rule of include/rmbx.h (rmbx_camera_jitter_draw) for f32 strengths, on Python
    floats (IEEE f64, one rounding per operation, math.sqrt correctly rounded)."""
    ep = int(episode) & 0xFFFFFFFF
    w0 = philox_block(2 * camera, PLANE, 0, ep, int(seed))
    w1 = philox_block(2 * camera + 1, PLANE, 0, ep, int(seed))
    d = [_sym(P, w0[k]) for k in range(3)]
    r = [_sym(T, w1[k]) for k in range(3)]
    rr = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    nrm = math.sqrt(1.0 + rr)
    return d + [1.0 / nrm, r[0] / nrm, r[1] / nrm, r[2] / nrm, 1.0 + _sym(F, w0[3])]


def norm_deviation_ulps(q):
    """max over the quaternions q [..., 4] of | |q| - 1 | in units of the ulp of 1.0 (2^-52), measured
    exactly: the sum of squares S as a rational, |q| - 1 = (S - 1) / (|q| + 1) with |q| + 1 = 2 to far
    below the unit.  (An f64 norm has roundings of its own of the size it would be measuring.)"""
    from fractions import Fraction

    worst = Fraction(0)
    for v in np.asarray(q, np.float64).reshape(-1, 4):
        worst = max(worst, abs(sum(Fraction(float(x)) ** 2 for x in v) - 1) / 2)
    return float(worst * 2**52)


# -- rows ----------------------------------------------------------------------------------------------------
IDENTITY = np.array([0.0, 0, 0, 1, 0, 0, 0, 1])


def row(d=(0.0, 0.0, 0.0), r=(0.0, 0.0, 0.0), s=1.0):
    """A row from a displacement, a Rodrigues vector (axis * tan(angle / 2)) and a fovy scale."""
    r = np.asarray(r, np.float64)
    n = np.sqrt(1.0 + r @ r)
    return np.concatenate([np.asarray(d, np.float64), [1.0 / n], r / n, [float(s)]])


def rows_for_the_renderer(drawn):
    """[7, 8]: identity, a pure displacement, a pure rotation, a pure fovy scale, every component just
    inside the spec's extremes (pos 0.5, rot 30 degrees per axis, fovy 0.5), a drawn row, identity."""
    t = float(T_MAX) * 0.999
    return np.stack([IDENTITY, row(d=(0.4, -0.3, 0.2)), row(r=(0.2, -0.25, 0.1)), row(s=1.45),
                     row(d=(-0.499, 0.499, -0.499), r=(t, -t, t), s=0.5001), np.asarray(drawn, np.float64), IDENTITY])


# -- the synthetic scene --------------------------------------------------------------------------------------
def texture():
    rng = np.random.default_rng(11)
    i, j = np.arange(16)[:, None, None], np.arange(16)[None, :, None]
    img = 128 + 90 * np.sin(i * 0.8 + np.arange(3)) * np.cos(j * 0.6) + rng.integers(-15, 15, (16, 16, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def synthetic(n_env=7, cam_pos=(0.05, -0.02, 0.1), cam_quat=None):
    """A sphere (on body 1, which moves: it sits elsewhere in every env), a turned box, a turned
    cylinder and a tilted, textured infinite plane behind them (all welded to the world), seen by a
    world camera that is itself offset and rolled.  Returns (arrays, gxpos [n, 4, 3], gxmat [4, 9])."""
    if cam_quat is None:
        a = math.radians(10.0)
        cam_quat = (math.cos(a / 2), 0.0, 0.0, math.sin(a / 2))  # rolled 10 degrees about its view axis
    objs = [(2, (0.25, 0, 0), (-0.7, 0.35, -2.6), (0.9, 0.3, 0.2)),
            (6, (0.25, 0.15, 0.2), (0.6, -0.3, -2.4), (0.8, 0.8, 0.2)),
            (5, (0.15, 0.3, 0), (0.55, 0.5, -2.8), (0.3, 0.4, 0.9)),
            (0, (0, 0, 0.1), (0, 0, -4.0), (1.0, 1.0, 1.0))]
    a, pos, gm = RC.scene(objs, cam_pos=cam_pos, cam_quat=cam_quat, welded=[0, 1, 1, 1])
    gm[1] = RC.rot((1, 1, 0.5), 35)
    gm[2] = RC.rot((1, 0.2, 0), 60)
    gm[3] = RC.rot((1, 0, 0), 25)
    matinfo = [[0.5, 0.3, 1, 1, 0, 0.0], [0.0, 0.5, 1, 1, 0, 0.1], [0.3, 0.6, 1, 1, 0, 0.0], [0.2, 0.4, 3, 3, 1, 0.0]]
    RC.add_materials(a, [(0, texture())], [-1, -1, -1, 0], matinfo, sky=((0.3, 0.5, 0.9), (0.9, 0.9, 0.8)))
    gx = np.tile(pos[None], (n_env, 1, 1))
    gx[:, 0, 0] += 0.08 * np.arange(n_env)  # the sphere moves from env to env
    gx[:, 0, 2] -= 0.05 * np.arange(n_env)
    return a, gx, gm


# -- a jittered camera from rotation matrices (independent of the quaternion product) ---------------------
def quat2mat(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rodrigues(axis, angle):
    """The rotation matrix of `angle` radians about a unit axis: I + sin K + (1 - cos) K^2."""
    x, y, z = (float(v) for v in axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def row_rotation(r):
    """The rotation matrix of a row's quaternion through its axis and angle (no quaternion algebra)."""
    qw, v = float(r[3]), np.asarray(r[4:7], np.float64)
    n = float(np.linalg.norm(v))
    if n == 0:
        return np.eye(3)
    return rodrigues(v / n, 2.0 * math.atan2(n, qw))


def mat2quat(R):
    """A unit quaternion of a rotation matrix (the trace branch: the test cameras turn far less than 180)."""
    w = 0.5 * math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2])
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def camera_by_matrices(arrays, c, r):
    """A copy of the arrays whose camera c is the jittered one, from the statement of the rule in words:
    the mount-frame position plus d, the camera's rotation matrix times the row's rotation (about the
    camera's own axes: on the right), fovy times s.  Agrees with common.camera_jitter.jittered_arrays
    to rounding, by another route."""
    a = dict(arrays)
    pos = np.array(arrays["cam_pos"], np.float64, copy=True)
    quat = np.array(arrays["cam_quat"], np.float64, copy=True)
    fovy = np.array(arrays["cam_fovy"], np.float64, copy=True)
    pos[c] = pos[c] + np.asarray(r[:3], np.float64)
    quat[c] = mat2quat(quat2mat(quat[c]) @ row_rotation(r))
    fovy[c] = fovy[c] * float(r[7])
    a["cam_pos"], a["cam_quat"], a["cam_fovy"] = pos, quat, fovy
    return a


# the oracle comparison's row: a few centimetres, a few degrees, a few per cent -- what a real mount does
ORACLE_ROW = row(d=(0.03, -0.02, 0.015), r=(math.tan(math.radians(2.0) / 2), -math.tan(math.radians(1.5) / 2),
                                             math.tan(math.radians(1.0) / 2)), s=1.04)
ORACLE_ENV = 2


def project(P, fovy_deg, w=W, h=H):
    """Pixel coordinates (x right, y down; centres at +0.5) of a camera-frame point (the camera looks
    along -z, y up): the pinhole with focal length (h / 2) / tan(fovy / 2) pixels."""
    f = (h / 2) / math.tan(math.radians(fovy_deg) / 2)
    return np.array([w / 2 + f * P[0] / -P[2], h / 2 - f * P[1] / -P[2]])
