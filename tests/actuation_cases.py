"""The actuation rule of include/rmbx.h (rmbx_action_perturb), restated with loops on top of
tests/philox_cases.py, and the cases tests/test_actuation.py and tests/test_actuation_gpu.py share.

An independent oracle: the package does not import it, and it does not import the package.  Where the
package's restatement (common/actuation.py) carries a ring, this one keeps the history of an episode
by step and looks the command of step r - D up in it.  The bias and the arithmetic are f64 in the
rule's order (numpy rounds each operation once).  The noise term uses either normals handed in as f32
(the bitwise restatement of what the device computes from its own normals), the f64 Box-Muller
normals of philox_cases rounded to f32, or those f64 normals themselves (the oracle the device may
differ from by its logf / sincospif error only).
"""

import numpy as np

import philox_cases as PC

PLANE_BIAS, PLANE_NOISE, PLANE_HOLD = 0x40000400, 0x40000500, 0x40000600
F = np.float32
# |device f32 - f64| of a normal: the bar tests/test_sampler_noise_gpu.py holds the device normals to
NORMAL_BAR = 4e-6
SEED = 2**40 + 7
T = 12
# rows at different steps of different episodes, as a stream has them; rows 0 and 1 start their episode
EPISODES = np.array([4117, -1, 0, 2**31 - 1, 5], dtype=np.int32)
R0 = np.array([0, 0, 7, 1, 30], dtype=np.int32)
NS, AS, DS, SKIPS = (1, 5), (1, 5, 7, 8), (0, 1, 3), (1, 3)
COMPONENTS = {"noise": dict(noise=0.3), "bias": dict(bias=0.2), "delay": dict(), "hold": dict(hold=0.4),
              "all": dict(noise=0.3, bias=0.2, hold=0.4)}
RING_FILL = -7.25  # what the ring holds before the first step of a case


def f32(x):
    return float(F(x))


def uniform(w):
    """u(w) = ((w >> 9) + 0.5) * 2^-23, f32 (exact)."""
    w = np.asarray(w, dtype=np.uint32)
    return ((w >> np.uint32(9)).astype(F) + F(0.5)) * F(2.0**-23)


def scale_arrays(A, noise=0.0, bias=0.0, rng_seed=11):
    """(scale, bs, ns) f64 [A]: a denormalisation scale and the two strength x scale arrays the host
    hands the kernel."""
    scale = np.random.default_rng(rng_seed).uniform(0.05, 3.0, A)
    return scale, np.float64(f32(bias)) * scale, np.float64(f32(noise)) * scale


def actions(n, A, steps=T, rng_seed=5):
    """f64 [steps, n, A]: a scripted action sequence."""
    return np.random.default_rng(rng_seed).normal(0.0, 1.5, (steps, n, A))


def scripted(episode, r, A):
    """f64 [A]: an action that depends on (episode, r) only, all values distinct and exact in f64."""
    return (int(episode) % 997) * 0.125 + int(r) * 1.0 + np.arange(A) * 2.0**-10


def packet_lost(seed, episode, r, hold):
    return bool(uniform(PC.words(seed, int(episode), int(r), PLANE_HOLD, 1)[0]) < F(hold))


def oracle(seed, skip, bs, ns, episode, r0, acts, noise=0.0, bias=0.0, delay=0, hold=0.0, z32=None,
           normals="f32", fill=RING_FILL):
    """The rule, row by row, step by step, element by element.  acts f64 [T, n, A]; row i is at step
    r0[i] + t of episode[i] at step t.  normals: "f32" (f64 Box-Muller rounded to f32) or "f64"; z32
    f32 [T, n, A] overrides them.  Returns (out f64 [T, n, A], NaN where nothing arrives, mask u8
    [T, n]); a command made before the case began arrives as `fill`."""
    steps, n, A = acts.shape
    out = np.full((steps, n, A), np.nan)
    mask = np.zeros((steps, n), dtype=np.uint8)
    B, S, P, D = F(bias), F(noise), F(hold), int(delay)
    for i in range(n):
        ep = int(episode[i])
        made = {}  # step -> the command made at it
        wb = PC.words(seed, ep, 0, PLANE_BIAS, A)
        for t in range(steps):
            r = int(r0[i]) + t
            v = np.empty(A)
            zrow = None
            if S != 0 and z32 is None:
                zrow = PC.normals(seed, ep, r - r % skip, PLANE_NOISE, A)
                if normals == "f32":
                    zrow = zrow.astype(F)
            for k in range(A):
                x = np.float64(acts[t, i, k])
                if B != 0:
                    x = x + np.float64(bs[k]) * np.float64(F(2.0) * uniform(wb[k]) - F(1.0))
                if S != 0:
                    z = z32[t, i, k] if z32 is not None else zrow[k]
                    x = x + np.float64(ns[k]) * np.float64(z)
                v[k] = x
            made[r] = v
            if r < D:
                continue
            if P != 0 and packet_lost(seed, ep, r, P):
                continue
            out[t, i] = made[r - D] if (r - D) in made else fill
            mask[t, i] = 1
    return out, mask


def tolerance(acts, bs, ns):
    """f64 [A]: how far the device may lie from the f64-normal oracle: the device normal's error
    (NORMAL_BAR) scaled by ns_k, plus the f64 roundings of the three terms (|z| <= 5.78)."""
    big = np.abs(acts).max() + np.abs(bs) + 5.78 * np.abs(ns)
    return np.abs(ns) * NORMAL_BAR + 8 * np.finfo(np.float64).eps * big
