"""The observation-perturbation rule of include/rmbx.h (rmbx_image_perturb), restated in numpy on top
of tests/philox_cases.py.

An independent oracle for tests/test_perturb.py and tests/test_perturb_gpu.py; the package does not
import it.  Everything up to the sensor noise is f32 in the rule's order (numpy rounds each f32
operation once).  The noise term is added either with the f64 Box-Muller normals of philox_cases
(the oracle: its pre-rounding value is f64) or with normals handed in as f32 (the bitwise restatement
of what the device computes from its own normals).
"""

import numpy as np

import philox_cases as PC

PLANE_PHOTO, PLANE_OCC, PLANE_NOISE, PLANE_STATE = 0x40000000, 0x40000100, 0x40000200, 0x40000300
F = np.float32


def uniform(w):
    """u(w) = ((w >> 9) + 0.5) * 2^-23, f32 (exact)."""
    w = np.asarray(w, dtype=np.uint32)
    return ((w >> np.uint32(9)).astype(F) + F(0.5)) * F(2.0**-23)


def constants(seed, episode, camera, H, W, brightness=0.0, contrast=0.0, gain=0.0, occ_h=0, occ_w=0):
    """The episode constants of one episode: dict b, c, g [3], y0, x0, colour [3]."""
    w = PC.words(seed, episode, 0, PLANE_PHOTO, 8)  # blocks 0 and 1: w0..w7
    s = F(2.0) * uniform(w) - F(1.0)
    out = {"b": F(brightness) * s[0], "c": F(1.0) + F(contrast) * s[1], "g": F(1.0) + F(gain) * s[2:5],
           "y0": 0, "x0": 0, "colour": np.zeros(3, F)}
    if occ_h > 0:
        w = PC.words(seed, episode, 0, PLANE_OCC + camera, 8)
        u = uniform(w)
        out["y0"] = int(u[0] * F(H - occ_h + 1))  # int() truncates
        out["x0"] = int(u[1] * F(W - occ_w + 1))
        out["colour"] = (w[2:5] >> np.uint32(24)).astype(F)
    return out


def before_noise(rgb, seed, episode, camera, brightness=0.0, contrast=0.0, gain=0.0, occ_h=0, occ_w=0):
    """Steps 1..6 on u8 [n, H, W, 3] for the i32 episodes [n]: f32 [n, H, W, 3]."""
    n, H, W, _ = rgb.shape
    v = rgb.astype(F)
    for r in range(n):
        k = constants(seed, int(episode[r]), camera, H, W, brightness, contrast, gain, occ_h, occ_w)
        x = v[r]
        if contrast != 0:
            x = (x - F(127.5)) * k["c"]
            x = x + F(127.5)
        if gain != 0:
            x = x * k["g"][None, None, :]
        if brightness != 0:
            x = x + k["b"]
        x = np.ascontiguousarray(x, dtype=F)
        if occ_h > 0:
            x[k["y0"]:k["y0"] + occ_h, k["x0"]:k["x0"] + occ_w, :] = k["colour"]
        v[r] = x
    assert v.dtype == F
    return v


def quantise(v):
    """Step 8: u8 of min(max(rint(v), 0), 255) (rint: ties to even, as rintf)."""
    return np.clip(np.rint(v), 0.0, 255.0).astype(np.uint8)


def normals64(seed, episode, draw, camera, L):
    """f64 [n, L]: the oracle's sensor-noise normals of the rows."""
    w = PC.words_batch(seed, episode, draw, PLANE_NOISE + camera, 1, L)[0]
    return PC.normals_from_words(w, L)


def apply_exact(rgb, seed, episode, draw, camera, z32=None, noise=0.0, **kw):
    """The rule with the device's own normals z32 f32 [n, L] (None without noise): u8 [n, H, W, 3],
    bit for bit what the kernel must write."""
    v = before_noise(rgb, seed, episode, camera, **kw)
    if noise > 0:
        v = v + F(noise) * np.asarray(z32, dtype=F).reshape(v.shape)
        assert v.dtype == F
    return quantise(v)


def apply_oracle(rgb, seed, episode, draw, camera, noise=0.0, z64=None, **kw):
    """The independent oracle: (u8 [n, H, W, 3], pre-rounding f64 [n, H, W, 3]); the noise term is
    f64 with the f64 normals (z64: normals64 of the same rows, computed once by the caller)."""
    v = before_noise(rgb, seed, episode, camera, **kw).astype(np.float64)
    if noise > 0:
        n, H, W, _ = rgb.shape
        if z64 is None:
            z64 = normals64(seed, episode, draw, camera, H * W * 3)
        v = v + float(F(noise)) * z64.reshape(v.shape)
    return quantise(v), v


def near_tie(pre, tau):
    """Where the pre-rounding value lies within tau of a half-integer."""
    frac = pre - np.floor(pre)
    return np.abs(frac - 0.5) <= tau


# -- the policy forms (store_policy of csrc/rmbx_render.hip) -----------------------------------------
def bf16_bits(x):
    """uint16 bit patterns of f32 -> bf16, round to nearest even (finite values)."""
    b = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    b = b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))
    return (b >> np.uint64(16)).astype(np.uint16)


def nchw(x):
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))


def s2d(x):
    """[n, H, W, 3] -> [n, H/2, W/2, 16]: channel (dy * 2 + dx) * 3 + k, 12..15 zero."""
    n, H, W, _ = x.shape
    y = x.reshape(n, H // 2, 2, W // 2, 2, 3).transpose(0, 1, 3, 2, 4, 5).reshape(n, H // 2, W // 2, 12)
    return np.concatenate([y, np.zeros((n, H // 2, W // 2, 4), dtype=x.dtype)], axis=-1)


def policy_form(u8, form, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """The form `form` (0 f32 NCHW, 1 bf16 NCHW, 2 bf16 s2d, 3 f32 s2d, 4 u8 s2d) of u8 [n, H, W, 3];
    the bf16 forms as uint16 bit patterns."""
    if form == 4:
        return s2d(u8)
    v = (u8.astype(F) / F(255.0) - np.asarray(mean, F)) / np.asarray(std, F)
    assert v.dtype == F
    v = nchw(v) if form < 2 else s2d(v)
    return bf16_bits(v) if form in (1, 2) else v


def layout(x, form):
    """A per-element array [n, H, W, 3] (a mask, say) in the layout of `form`."""
    return nchw(x) if form < 2 else s2d(x)


def state_noise(s, seed, episode, draw, sigma, z32):
    """s + (z * sigma) in f32 with the device's normals z32 [n, state_dim]."""
    return np.asarray(s, F) + np.asarray(z32, F) * F(sigma)
