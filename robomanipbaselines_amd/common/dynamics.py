"""Per-episode randomisation of the world's physical constants (--dynamics; the rule: include/rmbx.h,
rmbx_dynamics_draw): the spec and its parser, which bodies count as objects, the rule restated on the
host (numpy, no device: reports and tests), and the Dynamics object a rollout owns.

The four scale factors of an episode (contact friction, object joint damping, object mass, servo gain)
are a pure function of (seed, episode), so an episode meets the same world in any env slot, slot count,
shard or re-run, and `scales(seed, episodes, spec)` gives a study the factors to regress success on
without a device read-back.  The generator is the one of common/perturb.py, on a plane of its own.
"""

import dataclasses
import math

import numpy as np

from .perturb import _MASK, _philox, _uniform

PLANE = 0x40000700  # include/rmbx.h RMBX_DYNAMICS_PLANE
KEYS = ("friction", "damping", "mass", "gain")  # the column order of a scale row


@dataclasses.dataclass(frozen=True)
class DynamicsSpec:
    friction: float = 0.0
    damping: float = 0.0
    mass: float = 0.0
    gain: float = 0.0

    def as_dict(self):
        return {k: float(getattr(self, k)) for k in KEYS}

    def strengths(self):
        """The four f32 strengths in column order."""
        return np.array([getattr(self, k) for k in KEYS], dtype=np.float32)

    def __str__(self):
        return " ".join(f"{k}={v:g}" for k, v in self.as_dict().items())


def spec_from_dict(d):
    """The spec of a result file or a trace header (as_dict)."""
    return parse_spec([f"{k}={v!r}" for k, v in dict(d).items()])


def parse_spec(items):
    """KEY=VALUE strings -> DynamicsSpec.  ValueError for an unknown or repeated key, a malformed
    value or a value outside [0, 1)."""
    if isinstance(items, str):
        items = [items]
    seen = {}
    for item in items:
        key, sep, text = str(item).partition("=")
        if not sep or not key or not text:
            raise ValueError(f"--dynamics takes KEY=VALUE, not {item!r}")
        if key not in KEYS:
            raise ValueError(f"--dynamics: unknown key {key!r}; the keys are {', '.join(KEYS)}")
        if key in seen:
            raise ValueError(f"--dynamics: {key} is given twice")
        try:
            value = float(text)
        except ValueError:
            raise ValueError(f"--dynamics: {key}={text!r} is not a number") from None
        # the kernel's parameters are f32: the spec holds the values it reads, and the range holds for them
        with np.errstate(over="ignore"):
            stored = float(np.float32(value))
        if not (math.isfinite(stored) and value >= 0.0 and stored < 1.0):
            raise ValueError(f"--dynamics: {key}={text} outside [0, 1)")
        seen[key] = stored
    return DynamicsSpec(**seen)


def object_bodies(arrays, arm_joint):
    """u8 [nbody]: 1 for the bodies whose mass and joint damping scale -- every body other than the
    world whose kinematic tree (body_rootid) is not the one of the body carrying joint `arm_joint`
    (the first arm joint): the scene's objects, never a link of the robot or what it carries."""
    names = [str(n) for n in arrays["names_jnt"]]
    if arm_joint not in names:
        raise ValueError(f"the model has no joint {arm_joint!r}")
    root = np.asarray(arrays["body_rootid"])
    arm_root = root[int(np.asarray(arrays["jnt_body"])[names.index(arm_joint)])]
    group = (root != arm_root).astype(np.uint8)
    group[0] = 0
    return group


def scales(seed, episodes, spec):
    """f64 [n, 4]: the scale rows (friction, damping, mass, gain) of i32 episode indices [n], bit for
    bit what rmbx_dynamics_draw writes: 1 + (double)S * (double)(2 u(w_k) - 1), the bracket in f32,
    w_k word k of block 0 at draw 0 of the plane; exactly 1 for a strength of zero."""
    ep = np.atleast_1d(np.asarray(episodes, dtype=np.int64)) & _MASK
    w = _philox(0, PLANE, 0, ep, seed)
    out = np.ones((len(ep), 4), dtype=np.float64)
    for k, S in enumerate(spec.strengths()):
        if S != 0.0:
            sym = np.float32(2.0) * _uniform(w[k]) - np.float32(1.0)
            out[:, k] = 1.0 + np.float64(S) * sym.astype(np.float64)
    return out


def scaled_arrays(arrays, row, group):
    """A copy of the model arrays with one scale row applied as an env of the engine applies it
    (include/rmbx.h): what the CPU oracle is handed as the reference of a scaled env.  The derived
    constants (body_invweight0, dof_invweight0, meaninertia) stay the model's."""
    s0, s1, s2, s3 = (np.float64(v) for v in row)
    obj = np.asarray(group).astype(bool)
    a = dict(arrays)
    fr = np.array(arrays["pair_friction"], dtype=np.float64, copy=True).reshape(-1, 3)
    fr[:, 0] = fr[:, 0] * s0
    a["pair_friction"] = fr.reshape(np.shape(arrays["pair_friction"]))
    damping = np.array(arrays["dof_damping"], dtype=np.float64, copy=True)
    dof_obj = obj[np.asarray(arrays["dof_body"])]
    damping[dof_obj] = damping[dof_obj] * s1
    a["dof_damping"] = damping
    mass = np.array(arrays["body_mass"], dtype=np.float64, copy=True)
    mass[obj] = mass[obj] * s2
    a["body_mass"] = mass
    inertia = np.array(arrays["body_inertia"], dtype=np.float64, copy=True).reshape(len(mass), -1)
    inertia[obj] = inertia[obj] * s2
    a["body_inertia"] = inertia.reshape(np.shape(arrays["body_inertia"]))
    a["act_gain"] = np.array(arrays["act_gain"], dtype=np.float64, copy=True) * s3
    bias = np.array(arrays["act_bias"], dtype=np.float64, copy=True).reshape(-1, 3)
    bias[:, 1:] = bias[:, 1:] * s3
    a["act_bias"] = bias.reshape(np.shape(arrays["act_bias"]))
    return a


class Dynamics:
    """The device side of --dynamics for one rollout: the [n, 4] scale tensor the engine reads, bound
    at construction, and the draw that rewrites rows of it.  Nothing here synchronises with the host
    after construction."""

    def __init__(self, spec, seed, engine, body_group, device):
        import torch

        self.spec, self.seed = spec, int(seed) & (2**64 - 1)
        self.engine, self.n = engine, int(engine.n_env)
        self.scale = torch.ones((self.n, 4), dtype=torch.float64, device=device)
        engine.bind_dynamics(self.scale, body_group)

    def draw(self, episode, active=None):
        """Write the rows of the episodes i32 [n] (device); rows with active u8 [n] == 0 keep theirs."""
        from .. import kernels as K

        s = self.spec
        return K.dynamics_draw(self.seed, episode, self.scale, friction=s.friction, damping=s.damping, mass=s.mass,
                               gain=s.gain, active=active)

    def release(self):
        """Unbind: the engine runs the unscaled kernels again."""
        self.engine.bind_dynamics(None)
