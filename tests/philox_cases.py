"""The per-episode sampler-noise rule of include/rmbx.h (rmbx_philox_normal), restated in numpy.

An independent oracle for tests/test_sampler_noise.py and tests/test_sampler_noise_gpu.py; the
package does not import it.  Philox4x32-10 follows Random123 (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC'11); the normals are the f64 Box-Muller values of the same words.
"""

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of uint32 values, key: two.  Returns the four output words as
    uint64 arrays holding uint32 values."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    sh = np.uint64(32)
    m = np.uint64(MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # < 2^64: both factors < 2^32
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> sh, p0 & m
        hi1, lo1 = p1 >> sh, p1 & m
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def words(seed, episode, draw, plane, L):
    """The raw words of one row: uint32 [4 * ceil(L / 4)].  episode / draw are int32 values whose
    bit patterns enter the counter."""
    nb = (int(L) + 3) // 4
    seed = int(seed)
    assert 0 <= seed < 2**64
    j = np.arange(nb, dtype=np.uint64)
    w = philox4x32_10((j, int(plane) & MASK, int(draw) & MASK, int(episode) & MASK), (seed & MASK, seed >> 32))
    return np.stack(w, axis=1).reshape(-1).astype(np.uint32)


def words_batch(seed, episode, draw, plane0, nplane, L):
    """uint32 [nplane, n, 4 * ceil(L / 4)] for the i32 arrays episode / draw [n]."""
    nb = (int(L) + 3) // 4
    seed = int(seed)
    ep = (np.asarray(episode, dtype=np.int64) & MASK).astype(np.uint64)[None, :, None]
    dr = (np.asarray(draw, dtype=np.int64) & MASK).astype(np.uint64)[None, :, None]
    pl = (int(plane0) + np.arange(nplane, dtype=np.uint64))[:, None, None]
    j = np.arange(nb, dtype=np.uint64)[None, None, :]
    w = philox4x32_10((j, pl, dr, ep), (seed & MASK, seed >> 32))
    return np.stack(w, axis=-1).reshape(nplane, len(np.asarray(episode)), 4 * nb).astype(np.uint32)


def normals_from_words(w, L=None):
    """f64 Box-Muller normals of uint32 words [..., 4 * nb] -> [..., L] (L defaults to all)."""
    w = np.asarray(w, dtype=np.uint32)
    wa, wb = w[..., 0::2], w[..., 1::2]
    u1 = ((wa >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0**-23
    u2 = ((wb >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0**-23
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(w.shape, dtype=np.float64)
    z[..., 0::2] = r * np.cos(2.0 * np.pi * u2)
    z[..., 1::2] = r * np.sin(2.0 * np.pi * u2)
    return z if L is None else z[..., :L]


def normals(seed, episode, draw, plane, L):
    """f64 [L]: the normals of one row."""
    return normals_from_words(words(seed, episode, draw, plane, L), L)
