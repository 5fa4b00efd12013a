"""Per-episode jitter of each camera's pose and field of view (--camera_jitter; the rule:
include/rmbx.h, rmbx_camera_jitter_draw): the spec and its parser, the rule restated on the host
(numpy, no device: reports and tests), the composition of a row with a camera, and the CameraJitter
object a rollout owns.

A row (dx, dy, dz, qw, qx, qy, qz, s) of a camera and an episode is a pure function of (seed, episode,
camera index), so an episode sees the same cameras in any env slot, slot count, shard or re-run, and
`rows(seed, episodes, spec, ncam)` gives a study the offsets to regress success on without a device
read-back.  The generator is the one of common/perturb.py, on a plane of its own.
"""

import dataclasses
import math

import numpy as np

from .perturb import _MASK, _philox, _uniform

PLANE = 0x40000800  # include/rmbx.h RMBX_CAMERA_JITTER_PLANE
KEYS = ("pos", "rot", "fovy")
# the closed / half-open ranges of the strengths: pos metres, rot degrees, fovy relative
RANGES = {"pos": (0.5, True), "rot": (30.0, True), "fovy": (0.5, False)}
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


@dataclasses.dataclass(frozen=True)
class CameraJitterSpec:
    pos: float = 0.0  # metres: each displacement component lies in (-pos, pos)
    rot: float = 0.0  # degrees: each Rodrigues component lies in (-tan(rot / 2), tan(rot / 2))
    fovy: float = 0.0  # relative: fovy is scaled by a factor in (1 - fovy, 1 + fovy)

    def as_dict(self):
        return {k: float(getattr(self, k)) for k in KEYS}

    def tan_half_rot(self):
        """T, the f32 parameter the kernel reads for the rotation: float32(tan(radians(rot) / 2))."""
        return np.float32(math.tan(math.radians(self.rot) / 2.0))

    def strengths(self):
        """(P, T, F): the three f32 parameters of rmbx_camera_jitter_params."""
        return np.float32(self.pos), self.tan_half_rot(), np.float32(self.fovy)

    def enabled(self):
        return any(getattr(self, k) != 0.0 for k in KEYS)

    def __str__(self):
        return " ".join(f"{k}={v:g}" for k, v in self.as_dict().items())


def spec_from_dict(d):
    """The spec of a result file or a trace header (as_dict)."""
    return parse_spec([f"{k}={v!r}" for k, v in dict(d).items()])


def parse_spec(items):
    """KEY=VALUE strings -> CameraJitterSpec.  ValueError for an unknown or repeated key, a malformed
    value or a value outside its range (pos [0, 0.5], rot [0, 30], fovy [0, 0.5))."""
    if isinstance(items, str):
        items = [items]
    seen = {}
    for item in items:
        key, sep, text = str(item).partition("=")
        if not sep or not key or not text:
            raise ValueError(f"--camera_jitter takes KEY=VALUE, not {item!r}")
        if key not in KEYS:
            raise ValueError(f"--camera_jitter: unknown key {key!r}; the keys are {', '.join(KEYS)}")
        if key in seen:
            raise ValueError(f"--camera_jitter: {key} is given twice")
        try:
            value = float(text)
        except ValueError:
            raise ValueError(f"--camera_jitter: {key}={text!r} is not a number") from None
        # the kernel's parameters are f32: the spec holds the f32 value (for rot, the degrees T derives
        # from), and the range holds for it
        with np.errstate(over="ignore"):
            stored = float(np.float32(value))
        hi, closed = RANGES[key]
        inside = math.isfinite(stored) and value >= 0.0 and (stored <= hi if closed else stored < hi)
        if not inside:
            raise ValueError(f"--camera_jitter: {key}={text} outside [0, {hi:g}{']' if closed else ')'}")
        seen[key] = stored
    return CameraJitterSpec(**seen)


def _sym(S, w):
    """(double)S * (double)(2 u(w) - 1), the bracket in f32; exactly 0 for a strength of zero."""
    if S == 0.0:
        return np.zeros(np.shape(w), dtype=np.float64)
    sym = np.float32(2.0) * _uniform(w) - np.float32(1.0)
    return np.float64(S) * sym.astype(np.float64)


def rows(seed, episodes, spec, ncam):
    """f64 [ncam, n, 8]: the jitter rows (d, q, s) of i32 episode indices [n] for cameras 0..ncam-1,
    bit for bit what rmbx_camera_jitter_draw writes (include/rmbx.h): block 2c gives d and s, block
    2c + 1 the Rodrigues vector r, q = (1, r) / sqrt(1 + |r|^2), every f64 operation rounded once in
    the kernel's order."""
    ep = np.atleast_1d(np.asarray(episodes, dtype=np.int64)) & _MASK
    P, T, F = spec.strengths()
    out = np.empty((int(ncam), len(ep), 8), dtype=np.float64)
    for c in range(int(ncam)):
        w0 = _philox(2 * c, PLANE, 0, ep, seed)
        w1 = _philox(2 * c + 1, PLANE, 0, ep, seed)
        for k in range(3):
            out[c, :, k] = _sym(P, w0[k])
        r0, r1, r2 = (_sym(T, w1[k]) for k in range(3))
        nrm = np.sqrt(1.0 + (r0 * r0 + r1 * r1 + r2 * r2))  # |r|^2 first, then the 1, as the kernel
        out[c, :, 3] = 1.0 / nrm
        out[c, :, 4] = r0 / nrm
        out[c, :, 5] = r1 / nrm
        out[c, :, 6] = r2 / nrm
        out[c, :, 7] = 1.0 + _sym(F, w0[3])
    return out


def compose(cam_pos, cam_quat, cam_fovy, row):
    """(pos', quat', fovy') of a camera under one row, in the renderer's order of operations
    (include/rmbx.h): pos' = pos + d; quat' = quat (x) q, the Hamilton product with the sums left to
    right; fovy' = float32(float64(float32(fovy)) * s).  f64, f64, f32."""
    p = np.asarray(cam_pos, dtype=np.float64)
    a0, a1, a2, a3 = (np.float64(v) for v in cam_quat)
    row = np.asarray(row, dtype=np.float64)
    b0, b1, b2, b3 = row[3:7]
    pos = p + row[:3]
    quat = np.array([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                     a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1,
                     a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], dtype=np.float64)
    fovy = np.float32(np.float64(np.float32(cam_fovy)) * row[7])
    return pos, quat, fovy


def jittered_arrays(arrays, camera_index, row):
    """A copy of the model arrays with cam_pos, cam_quat and cam_fovy of camera `camera_index` replaced
    by the values an env with this row renders with: what an unbound renderer, or the CPU oracle, is
    handed as the reference of a jittered env.  cam_fovy holds the f32 value the kernel uses."""
    c = int(camera_index)
    a = dict(arrays)
    pos = np.array(arrays["cam_pos"], dtype=np.float64, copy=True)
    quat = np.array(arrays["cam_quat"], dtype=np.float64, copy=True)
    fovy = np.array(arrays["cam_fovy"], dtype=np.float64, copy=True)
    pos[c], quat[c], f = compose(pos[c], quat[c], fovy[c], row)
    fovy[c] = np.float64(f)
    a["cam_pos"], a["cam_quat"], a["cam_fovy"] = pos, quat, fovy
    return a


class CameraJitter:
    """The device side of --camera_jitter for one rollout: the [ncam, n, 8] row tensor the renderer
    reads, bound at construction, and the draw that rewrites rows of it.  Nothing here synchronises
    with the host after construction."""

    def __init__(self, spec, seed, renderer, n_env, device):
        import torch

        self.spec, self.seed = spec, int(seed) & (2**64 - 1)
        self.renderer, self.n = renderer, int(n_env)
        self.ncam = len(renderer.cam_names)
        ident = torch.tensor(IDENTITY, dtype=torch.float64, device=device)
        self.rows = ident.repeat(self.ncam, self.n, 1).contiguous()
        renderer.bind_camera_rows(self.rows)

    def draw(self, episode, active=None):
        """Write the rows of the episodes i32 [n] (device); rows with active u8 [n] == 0 keep theirs."""
        from .. import kernels as K

        P, T, F = self.spec.strengths()
        return K.camera_jitter_draw(self.seed, episode, self.rows, pos=float(P), tan_half_rot=float(T), fovy=float(F),
                                    active=active)

    def release(self):
        """Unbind: the renderer renders every env with the scene's cameras again."""
        self.renderer.bind_camera_rows(None)
