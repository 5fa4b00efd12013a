"""Per-episode perturbation of the command the robot executes (--actuation; the rule: include/rmbx.h,
rmbx_action_perturb): the spec and its parser, the rule restated on the host (numpy, no device:
reports and tests), and the Actuator a rollout owns.

What an episode executes is a pure function of (seed, episode, its own rollout_time_idx) and of the
actions its policy produced, so it is the same in any env slot, slot count, shard or re-run.  The
generator is the one of common/perturb.py, on planes of its own.
"""

import dataclasses
import math

import numpy as np

from .perturb import _MASK, _philox, _uniform

PLANE_BIAS, PLANE_NOISE, PLANE_HOLD = 0x40000400, 0x40000500, 0x40000600
MAX_DELAY = 64

# key -> (lowest value, highest value, highest value included)
_RANGES = {
    "noise": (0.0, math.inf, False),  # normalised action units (standard deviation)
    "bias": (0.0, math.inf, False),  # normalised action units (half width of the uniform offset)
    "delay": (0, MAX_DELAY, True),  # env-steps
    "hold": (0.0, 1.0, False),  # probability that a step's command packet is lost
}


@dataclasses.dataclass(frozen=True)
class ActuationSpec:
    noise: float = 0.0
    bias: float = 0.0
    delay: int = 0
    hold: float = 0.0

    def as_dict(self):
        return {"noise": float(self.noise), "bias": float(self.bias), "delay": int(self.delay), "hold": float(self.hold)}

    def __str__(self):
        return " ".join(f"{k}={v:g}" for k, v in self.as_dict().items())


def spec_from_dict(d):
    """The spec of a result file or a trace header (as_dict)."""
    return parse_spec([f"{k}={v!r}" for k, v in dict(d).items()])


def parse_spec(items):
    """KEY=VALUE strings -> ActuationSpec.  ValueError for an unknown or repeated key, a malformed
    value or a value out of range."""
    if isinstance(items, str):
        items = [items]
    seen = {}
    for item in items:
        key, sep, text = str(item).partition("=")
        if not sep or not key or not text:
            raise ValueError(f"--actuation takes KEY=VALUE, not {item!r}")
        if key not in _RANGES:
            raise ValueError(f"--actuation: unknown key {key!r}; the keys are {', '.join(_RANGES)}")
        if key in seen:
            raise ValueError(f"--actuation: {key} is given twice")
        lo, hi, closed = _RANGES[key]
        if key == "delay":
            try:
                value = int(text)
            except ValueError:
                raise ValueError(f"--actuation: {key}={text!r} is not an integer") from None
            if not lo <= value <= hi:
                raise ValueError(f"--actuation: {key}={text} outside [{lo:g}, {hi:g}]")
            seen[key] = value
            continue
        try:
            value = float(text)
        except ValueError:
            raise ValueError(f"--actuation: {key}={text!r} is not a number") from None
        # the kernel's parameters are f32: the spec holds the values it reads, and the range holds for them
        with np.errstate(over="ignore"):
            stored = float(np.float32(value))
        if not (math.isfinite(stored) and value >= lo and (stored <= hi if closed else stored < hi)):
            raise ValueError(f"--actuation: {key}={text} outside [{lo:g}, {hi:g}{']' if closed else ')'}")
        seen[key] = stored
    return ActuationSpec(**seen)


def scales(spec, stats):
    """(bs, ns) f64 [A]: bias and noise strength times scale_k, the factor denormalize_data multiplies
    normalised action dimension k by (kernels.denorm_coeffs: std, or range / (out_max - out_min))."""
    from ..kernels import denorm_coeffs

    scale = np.asarray(denorm_coeffs(stats)[0], dtype=np.float64)
    return np.float64(spec.bias) * scale, np.float64(spec.noise) * scale


def is_skip(r, delay, skip):
    """is_skip of the step the command arriving at rollout step r was made for (non-negative modulo)."""
    return (int(r) - int(delay)) % int(skip) != 0


# -- the rule on the host ----------------------------------------------------------------------------
def _rows(x, T, n, name):
    x = np.asarray(x, dtype=np.int64)
    if x.shape == (n,):
        return np.broadcast_to(x, (T, n))
    if x.shape != (T, n):
        raise ValueError(f"{name} must have shape {(n,)} or {(T, n)} (got {x.shape})")
    return x


def bias_uniforms(seed, episode, A):
    """f32 [n, A]: 2 * u(w_k) - 1 of the BIAS plane, w_k word k % 4 of block k / 4."""
    ep = np.atleast_1d(np.asarray(episode, dtype=np.int64)) & _MASK
    nb = (int(A) + 3) // 4
    w = _philox(np.arange(nb)[None, :], PLANE_BIAS, 0, ep[:, None], seed)  # four [n, nb]
    u = np.stack([_uniform(x) for x in w], axis=-1).reshape(len(ep), 4 * nb)[:, :A]
    return np.float32(2.0) * u - np.float32(1.0)


def host_normals(seed, episode, draw, A):
    """f32 [n, A]: the NOISE plane's Box-Muller normals of the rows, computed in f64 and rounded to
    f32 -- within the device's logf / sincospif error of the device's own (which a bitwise
    comparison is fed instead)."""
    ep = np.atleast_1d(np.asarray(episode, dtype=np.int64)) & _MASK
    dr = np.atleast_1d(np.asarray(draw, dtype=np.int64)) & _MASK
    nb = (int(A) + 3) // 4
    w = _philox(np.arange(nb)[None, :], PLANE_NOISE, dr[:, None], ep[:, None], seed)
    u = [((x >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0**-23 for x in w]
    z = np.empty((len(ep), nb, 4), dtype=np.float64)
    for pair in (0, 1):
        rad = np.sqrt(-2.0 * np.log(u[2 * pair]))
        z[..., 2 * pair] = rad * np.cos(2.0 * np.pi * u[2 * pair + 1])
        z[..., 2 * pair + 1] = rad * np.sin(2.0 * np.pi * u[2 * pair + 1])
    return z.reshape(len(ep), 4 * nb)[:, :A].astype(np.float32)


def lost(seed, episode, r, hold):
    """bool [...]: the packet of (episode, step r) is lost: u(w0) < P in f32, w0 word 0 of block 0 of
    the HOLD plane at draw r."""
    ep = np.asarray(episode, dtype=np.int64) & _MASK
    rr = np.asarray(r, dtype=np.int64) & _MASK
    return _uniform(_philox(0, PLANE_HOLD, rr, ep, seed)[0]) < np.float32(hold)


def restate(spec, seed, skip, bias_scale, noise_scale, episode, r, actions, mask_in=None, z32=None, ring=None):
    """The rule for a whole scripted action sequence: actions f64 [T, n, A], step t of every row;
    episode and r i32 [n] (the same at every step) or [T, n] (r is the row's rollout_time_idx at step
    t, as a stream has it); mask_in u8 [T, n] or None; z32 f32 [T, n, A] the normals to use (the
    device's own for a bitwise comparison; None: host_normals); ring f64 [n, D + 1, A], updated in
    place (None: zeros).  Returns (out f64 [T, n, A], NaN where nothing arrives, mask u8 [T, n])."""
    actions = np.asarray(actions, dtype=np.float64)
    T, n, A = actions.shape
    D, skip = int(spec.delay), int(skip)
    ep_all, r_all = _rows(episode, T, n, "episode"), _rows(r, T, n, "r")
    bs, ns = np.asarray(bias_scale, np.float64), np.asarray(noise_scale, np.float64)
    if ring is None:
        ring = np.zeros((n, D + 1, A), dtype=np.float64)
    out = np.full((T, n, A), np.nan, dtype=np.float64)
    mask = np.zeros((T, n), dtype=np.uint8)
    rows = np.arange(n)
    for t in range(T):
        ep, rr = ep_all[t], r_all[t]
        active = rr >= 0
        if mask_in is not None:
            active = active & (np.asarray(mask_in[t]) != 0)
        rr = np.where(active, rr, 0)
        v = actions[t].copy()
        if spec.bias != 0.0:
            v = v + bs * bias_uniforms(seed, ep, A).astype(np.float64)
        if spec.noise != 0.0:
            z = host_normals(seed, ep, rr - rr % skip, A) if z32 is None else np.asarray(z32[t], dtype=np.float32)
            v = v + ns * z.astype(np.float64)
        ring[rows[active], (rr % (D + 1))[active]] = v[active]
        arrived = ring[rows, (rr + 1) % (D + 1)]
        ok = active & (rr >= D)
        if spec.hold != 0.0:
            ok = ok & ~lost(seed, ep, rr, spec.hold)
        out[t][ok] = arrived[ok]
        mask[t] = ok
    return out, mask


class Actuator:
    """The device side of --actuation for one rollout: the rows' episode and r tensors, the delay ring,
    the scale arrays, the arriving action and its mask.  Nothing here synchronises with the host."""

    def __init__(self, spec, seed, n, action_dim, skip, stats, device):
        import torch

        self.spec, self.seed = spec, int(seed) & (2**64 - 1)
        self.n, self.A, self.skip, self.device = int(n), int(action_dim), int(skip), device
        bs, ns = scales(spec, stats)
        if bs.shape != (self.A,):
            raise ValueError(f"the action statistics have {bs.shape[0]} dimensions, the action {self.A}")
        self.bias_scale = torch.tensor(bs, dtype=torch.float64, device=device)
        self.noise_scale = torch.tensor(ns, dtype=torch.float64, device=device)
        self.ring = torch.zeros((self.n, spec.delay + 1, self.A), dtype=torch.float64, device=device)
        self.out = torch.zeros((self.n, self.A), dtype=torch.float64, device=device)
        self.mask = torch.zeros(self.n, dtype=torch.uint8, device=device)
        self.episode = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.r = torch.zeros(self.n, dtype=torch.int32, device=device)

    def set_rows(self, episode, r):
        """episode: i32 [n] device tensor, kept by reference (a stream's slot -> episode map stays
        current); r: an int for every row, or an i32 [n] (view of a) device tensor, copied."""
        import torch

        self.episode = episode
        if isinstance(r, torch.Tensor):
            self.r.copy_(r)
        else:
            self.r.fill_(int(r))

    def is_skip(self, r):
        """The is_skip motion_command gets at the host's rollout step r."""
        return is_skip(r, self.spec.delay, self.skip)

    def __call__(self, action, mask_in=None):
        """One env-step: (the arriving action f64 [n, A], its mask u8 [n]), both owned by this object;
        `action` is not written."""
        from .. import kernels as K

        s = self.spec
        return K.action_perturb(action, self.seed, self.episode, self.r, self.ring, self.bias_scale, self.noise_scale,
                                self.out, self.mask, noise=s.noise, bias=s.bias, delay=s.delay, hold=s.hold,
                                skip=self.skip, mask_in=mask_in)
