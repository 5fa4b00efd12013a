"""Per-episode perturbation of what the policy observes (--perturb; the rule: include/rmbx.h,
rmbx_image_perturb): the spec and its parser, the episode constants on the host (numpy, no device:
reports and bin/Replay.py), and the Perturber a rollout owns.

An episode's perturbation is a pure function of (seed, episode, camera, rollout_time_idx), so it is
the same in any env slot, slot count, shard or re-run, and Replay can show the frame the policy saw.
"""

import dataclasses
import math

import numpy as np

PLANE_PHOTO, PLANE_OCC, PLANE_NOISE, PLANE_STATE = 0x40000000, 0x40000100, 0x40000200, 0x40000300

# key -> (lowest value, highest value, highest value included)
_RANGES = {
    "brightness": (0.0, 255.0, True),  # levels
    "contrast": (0.0, 1.0, False),
    "gain": (0.0, 1.0, False),
    "noise": (0.0, math.inf, False),  # levels (standard deviation)
    "occluder": (0.0, 1.0, True),  # fraction of each image side
    "state_noise": (0.0, math.inf, False),  # normalised units (standard deviation)
}


@dataclasses.dataclass(frozen=True)
class PerturbSpec:
    brightness: float = 0.0
    contrast: float = 0.0
    gain: float = 0.0
    noise: float = 0.0
    occluder: float = 0.0
    state_noise: float = 0.0

    def occ_size(self, H, W):
        """(occ_h, occ_w) = (floor(f * H), floor(f * W))."""
        return int(math.floor(self.occluder * H)), int(math.floor(self.occluder * W))

    @property
    def touches_images(self):
        return any(v != 0.0 for v in (self.brightness, self.contrast, self.gain, self.noise, self.occluder))

    def as_dict(self):
        return {k: float(v) for k, v in dataclasses.asdict(self).items()}

    def __str__(self):
        return " ".join(f"{k}={v:g}" for k, v in self.as_dict().items())


def spec_from_dict(d):
    """The spec of a result file or a trace header (as_dict)."""
    return parse_spec([f"{k}={v!r}" for k, v in dict(d).items()])


def parse_spec(items):
    """KEY=VALUE strings -> PerturbSpec.  ValueError for an unknown or repeated key, a malformed
    value or a value out of range."""
    if isinstance(items, str):
        items = [items]
    seen = {}
    for item in items:
        key, sep, text = str(item).partition("=")
        if not sep or not key or not text:
            raise ValueError(f"--perturb takes KEY=VALUE, not {item!r}")
        if key not in _RANGES:
            raise ValueError(f"--perturb: unknown key {key!r}; the keys are {', '.join(_RANGES)}")
        if key in seen:
            raise ValueError(f"--perturb: {key} is given twice")
        try:
            value = float(text)
        except ValueError:
            raise ValueError(f"--perturb: {key}={text!r} is not a number") from None
        lo, hi, closed = _RANGES[key]
        if not (math.isfinite(value) and value >= lo and (value <= hi if closed else value < hi)):
            raise ValueError(f"--perturb: {key}={text} outside [{lo:g}, {hi:g}{']' if closed else ')'}")
        # the kernel's parameters are f32: the spec holds the values it reads
        seen[key] = float(np.float32(value)) if key != "occluder" else value
    return PerturbSpec(**seen)


# -- the generator on the host (Philox4x32-10, Random123; the device form is csrc/rmbx_philox.h) ------
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def _philox(block, plane, draw, episode, seed):
    """The four words of counter (block, plane, draw, episode) under key seed: uint64 arrays holding
    uint32 values, broadcast over the arguments."""
    c = [np.asarray(v, dtype=np.int64).astype(np.uint64) & np.uint64(_MASK) for v in (block, plane, draw, episode)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(seed) & _MASK, (int(seed) >> 32) & _MASK
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(_MASK)]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def _uniform(w):
    """u(w) = ((w >> 9) + 0.5) * 2^-23 in f32 (exact)."""
    return ((w >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0**-23)


def episode_params(seed, episodes, spec, camera, H, W):
    """The episode constants the kernel derives, for i32 episode indices [n] and one camera: a dict
    of b f32 [n], c f32 [n], g f32 [n, 3], y0 / x0 i32 [n], occ_h / occ_w ints and colour f32 [n, 3]
    (zeros without an occluder).  Pure numpy f32 in the kernel's order of operations."""
    if not 0 <= int(camera) <= 255:
        raise ValueError(f"camera index {camera} outside [0, 255]")
    ep = np.atleast_1d(np.asarray(episodes, dtype=np.int64)) & _MASK
    one, two = np.float32(1.0), np.float32(2.0)
    f32 = np.float32
    w = [_philox(j, PLANE_PHOTO, 0, ep, seed) for j in (0, 1)]
    w = w[0] + w[1]  # w0..w7
    sym = [two * _uniform(x) - one for x in w[:5]]
    b = f32(spec.brightness) * sym[0]
    c = one + f32(spec.contrast) * sym[1]
    g = np.stack([one + f32(spec.gain) * s for s in sym[2:5]], axis=1)
    occ_h, occ_w = spec.occ_size(H, W)
    n = len(ep)
    y0, x0, colour = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
    if occ_h > 0:
        w = [_philox(j, PLANE_OCC + int(camera), 0, ep, seed) for j in (0, 1)]
        w = w[0] + w[1]
        y0 = (_uniform(w[0]) * f32(H - occ_h + 1)).astype(np.int32)
        x0 = (_uniform(w[1]) * f32(W - occ_w + 1)).astype(np.int32)
        colour = np.stack([(x >> np.uint64(24)).astype(np.float32) for x in w[2:5]], axis=1)
    return {"b": b.astype(f32), "c": c.astype(f32), "g": g.astype(f32), "y0": y0, "x0": x0, "occ_h": occ_h,
            "occ_w": occ_w, "colour": colour}


class Perturber:
    """The device side of --perturb for one rollout: the rows' episode and draw (rollout_time_idx)
    tensors and a scratch 8-bit frame per camera.  Nothing here synchronises with the host."""

    def __init__(self, spec, seed, n, height, width, camera_names, device):
        import torch

        self.spec, self.seed = spec, int(seed) & (2**64 - 1)
        self.n, self.H, self.W, self.device = int(n), int(height), int(width), device
        self.camera_index = {cam: i for i, cam in enumerate(camera_names)}
        self.occ_h, self.occ_w = spec.occ_size(self.H, self.W)
        self.episode = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.draw = torch.zeros(self.n, dtype=torch.int32, device=device)
        self._scratch = {}
        self._z = None

    def set_rows(self, episode, draw):
        """episode: i32 [n] device tensor, kept by reference (a stream's slot -> episode map stays
        current); draw: an int for every row, or an i32 [n] (view of a) device tensor, copied."""
        import torch

        self.episode = episode
        if isinstance(draw, torch.Tensor):
            self.draw.copy_(draw)
        else:
            self.draw.fill_(int(draw))

    def _call(self, cam, rgb, **out):
        from .. import kernels as K

        s = self.spec
        return K.image_perturb(rgb, self.seed, self.episode, self.draw, self.camera_index[cam], brightness=s.brightness,
                               contrast=s.contrast, gain=s.gain, noise=s.noise, occ_h=self.occ_h, occ_w=self.occ_w, **out)

    def frame(self, cam, rgb):
        """The perturbed 8-bit frame of camera `cam` (a scratch tensor this object owns; `rgb`, the
        clean frame, is not written)."""
        import torch

        buf = self._scratch.get(cam)
        if buf is None or buf.shape != rgb.shape:
            buf = self._scratch[cam] = torch.empty_like(rgb)
        self._call(cam, rgb, rgb_out=buf)
        return buf

    def policy(self, cam, rgb, policy, mean, std):
        """Write the policy form of the perturbed frame into `policy` (the form the renderer would
        have written for the clean one)."""
        self._call(cam, rgb, policy=policy, mean=mean, std=std)
        return policy

    def state(self, s):
        """s f32 [n, state_dim] (normalised) -> s + (z * state_noise)."""
        import torch

        from .. import kernels as K

        if self.spec.state_noise == 0.0 or s.shape[-1] == 0:
            return s
        if self._z is None or tuple(self._z.shape[1:]) != tuple(s.shape):
            self._z = torch.empty((1,) + tuple(s.shape), dtype=torch.float32, device=s.device)
        K.philox_normal(self.seed, self.episode, self.draw, self._z, plane0=PLANE_STATE)
        return s + self._z[0] * self.spec.state_noise
