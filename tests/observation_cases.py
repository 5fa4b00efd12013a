"""Inputs of the observation-kernel edge tests (tests/test_observation_cases.py on the host,
tests/test_pointcloud_edges_gpu.py, tests/test_image_edges_gpu.py and tests/test_sarnn_edges_gpu.py
on the device): the frames, clouds and recurrences at which index arithmetic, reductions and
tie-breaks go wrong, each with its oracle result computed once and shared.

Nothing here touches a device.  The oracles are oracle/pointcloud.py, oracle/image.py and the f64
recomputations of tests/test_sarnn_gpu.py.
"""

import functools

import numpy as np
import torch

from oracle import image as OI
from oracle import pointcloud as OP
from test_pointcloud_gpu import HI, LO, STATS

FOVY = 45.0

# ------------------------------------------------------------------------------------------
# Point cloud / FPS
# ------------------------------------------------------------------------------------------
# 32x32: exactly one pixel slot per lane; 64x128: all eight slots of every lane (the kernel's limit);
# 90x91: 8190 pixels, a ragged last slot; 17x23: fewer pixels than lanes
FPS_SIZES = [(32, 32, 64), (64, 128, 256), (90, 91, 128), (17, 23, 64)]
TIE_SCENES = ("constant", "checker", "late_start")
MIN_TIE_STEPS = 20
FLAT_COLOUR = (120, 80, 200)


def late_start_rows(H):
    """Invalid leading rows of the late_start scene: 20, or 5 where the frame has fewer than 21 rows
    (17x23: the first kept pixel is then pixel 115, a later lane of the only slot)."""
    return 20 if H > 20 else 5


def tie_scene(name, H, W):
    """(depth f32 [H, W], rgb u8 [H, W, 3]) of a frame as the substitute renderer draws them: flat
    depth, flat colours, so that farthest-point distances tie."""
    d = np.full((H, W), 0.5, dtype=np.float32)
    rgb = np.empty((H, W, 3), dtype=np.uint8)
    rgb[:] = FLAT_COLOUR
    if name == "checker":
        cell = (np.arange(H)[:, None] // 8 + np.arange(W)[None, :] // 8) % 2
        d[cell == 0] = 0.75  # the far level in the top left cell
        rgb[:, 0::2] = 0
        rgb[:, 1::2] = 255
    elif name == "late_start":
        d[:late_start_rows(H)] = 0.0
    elif name != "constant":
        raise ValueError(name)
    return d, rgb


def cropped_cloud(depth, rgb, lo=LO, hi=HI):
    """f64 [P, 6] cloud of the oracle after the crop (what oracle.pointcloud.observation samples)."""
    xyz, col = OP.glue.depth_to_pointcloud(depth, FOVY, rgb)
    return OP.glue.crop_bb(np.concatenate((xyz, col), axis=1), None if lo is None else np.asarray(lo),
                           None if hi is None else np.asarray(hi))


def kept_pixels(depth, rgb, lo=LO, hi=HI):
    """Flat pixel index of every point of cropped_cloud, in its order (the crop keeps pixel order)."""
    d = depth.reshape(-1)
    valid = np.flatnonzero((0.0 < d) & (d < np.inf))
    xyz = OP.glue.depth_to_pointcloud(depth, FOVY, rgb)[0]
    m = np.ones(len(valid), dtype=bool)
    if lo is not None:
        m &= np.all(xyz > np.asarray(lo), axis=1)
    if hi is not None:
        m &= np.all(xyz < np.asarray(hi), axis=1)
    return valid[m]


def fps_trace(points, K):
    """The loop of oracle.pointcloud.fps_indices with its intermediate state kept: (indices int64 [K],
    per step the indices of the points that attain the running-minimum maximum, none where that
    maximum is 0).  The host test holds the indices equal to fps_indices', so this is the oracle, not
    a second one."""
    pts = np.asarray(points, dtype=np.float32)
    P = pts.shape[0]
    idx = np.full(K, -1, dtype=np.int64)
    dists = np.full(P, np.finfo(np.float32).max, dtype=np.float32)
    sel, ties = 0, []
    for k in range(min(K, P)):
        idx[k] = sel
        diff = pts[sel][None, :] - pts
        d2 = np.zeros(P, dtype=np.float32)
        for d in range(pts.shape[1]):
            d2 = d2 + diff[:, d] * diff[:, d]
        dists = np.minimum(d2, dists)
        m = dists.max()
        ties.append(np.flatnonzero(dists == m) if m > 0 else np.empty(0, dtype=np.int64))
        sel = int(np.argmax(dists)) if m > 0 else 0
    return idx, ties


def _sparse_frame(H, W, pixels, seed, depth=None):
    """A frame invalid (depth 0) everywhere but at the flat pixel indices `pixels`; their depths are below
    0.45, where no pixel of a 64x128 frame leaves the box LO..HI."""
    rng = np.random.default_rng(seed)
    d = np.zeros(H * W, dtype=np.float32)
    d[pixels] = rng.uniform(0.2, 0.45, len(pixels)).astype(np.float32) if depth is None else depth
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return d.reshape(H, W), rgb


def _random_frame(H, W, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.2, 1.3, (H, W)).astype(np.float32)  # z above 1.0 is cropped by the max bound
    d[:3] = 0.0
    d[-2:, :5] = np.inf
    return d, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _scattered(H, W, count, seed):
    return np.sort(np.random.default_rng(seed).choice(H * W, size=count, replace=False))


def count_cases():
    """name -> (depth, rgb, K, expected kept count): kept counts around K on a 64x128 frame that is
    invalid elsewhere."""
    H, W = 64, 128
    one = _sparse_frame(H, W, np.array([H * W - 1]), 1)  # lane 1023, slot 7
    sparse = _sparse_frame(H, W, _scattered(H, W, 100, 4), 4)
    # five pixels so close to the camera that every squared f32 distance underflows to 0: each round is
    # all-zero and re-selects point 0 while K is not yet reached
    near = _sparse_frame(H, W, np.array([700, 1500, 2600, 5000, 8000]), 6, depth=np.float32(1e-30))
    near[1][:] = FLAT_COLOUR
    return {
        "one_kept_last_pixel": (*one, 64, 1),
        "exactly_K": (*_sparse_frame(H, W, _scattered(H, W, 64, 2), 2), 64, 64),
        "K_plus_1": (*_sparse_frame(H, W, _scattered(H, W, 65, 3), 3), 64, 65),
        "K_is_1": (*sparse, 1, 100),
        "K_9000_tail": (*sparse, 9000, 100),  # 8900 trailing slots: the tail loop strides nine times
        "two_kept_K_8": (*_sparse_frame(H, W, np.array([3000, 8191]), 5), 8, 2),
        "zero_rounds": (*near, 8, 5),
    }


def bound_cases():
    """name -> (min_bound, max_bound): the wrapper passes NULL for a missing one."""
    return {"min_only": (LO, None), "max_only": (None, HI), "neither": (None, None)}


def bounds_frame():
    """48x64 random frame with a fifth of its pixels far (5.0: kept only without a max bound).  The min
    bound binds on x and y at the frame's left and top (z > 0 > -0.4 always), the max bound on z."""
    d, rgb = _random_frame(48, 64, 11)
    rng = np.random.default_rng(12)
    d[rng.uniform(size=d.shape) < 0.2] = 5.0
    return d, rgb


Z_LO = [-0.4, -0.4, 0.25]
_ONE, _QUARTER = np.float32(1.0), np.float32(0.25)
STRICT_DEPTHS = np.array([_ONE, np.nextafter(_ONE, np.float32(0)), _QUARTER, np.nextafter(_QUARTER, _ONE),
                          0.5, 0.75], dtype=np.float32)
STRICT_KEPT = 4  # all but the depths exactly on the max z bound 1.0 and the min z bound 0.25


def strict_frame():
    """17x23 frame, six valid pixels around the centre: z exactly on a bound is dropped (strict
    comparisons), its neighbour inside the bound is kept."""
    H, W = 17, 23
    pix = np.array([(H // 2) * W + W // 2 + k for k in range(-3, 3)])
    return _sparse_frame(H, W, pix, 13, depth=STRICT_DEPTHS)


SUBNORMAL = np.float32(1e-40)
ODD_DEPTHS = np.array([np.nan, -0.0, -0.7, np.inf, SUBNORMAL, -np.inf], dtype=np.float32)


def odd_depth_frame():
    """(depth, rgb, number of ordinary valid pixels): 32x32, 40 valid pixels with NaN, -0.0, a negative,
    +inf, -inf and a positive subnormal scattered among them; of those six only the subnormal is kept."""
    H, W = 32, 32
    pix = _scattered(H, W, 46, 14)
    d, rgb = _sparse_frame(H, W, pix, 14)
    flat = d.reshape(-1)
    flat[pix[3::8][:6]] = ODD_DEPTHS
    return d, rgb, 40


def mixed_batch():
    """(depth [4, 32, 32], rgb, K): a tie scene, a random scene, an empty frame and a one-point frame."""
    H, W = 32, 32
    none = np.array([], dtype=np.int64)
    frames = [tie_scene("checker", H, W), _random_frame(H, W, 21), _sparse_frame(H, W, none, 22),
              _sparse_frame(H, W, np.array([517]), 23)]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), 64


_OBSERVATIONS = {}


def observation(key, depth, rgb, K, lo=LO, hi=HI):
    """oracle.pointcloud.observation of a frame (normalised f32 [K, 6], raw f64 [K, 6], count), computed
    once per `key` (which names the frame) and shared between the tests; the arrays are read-only."""
    full = (key, K, None if lo is None else tuple(lo), None if hi is None else tuple(hi))
    if full not in _OBSERVATIONS:
        norm, raw, count = OP.observation(depth, rgb, FOVY, lo, hi, K, STATS)
        norm.setflags(write=False)
        raw.setflags(write=False)
        _OBSERVATIONS[full] = (norm, raw, count)
    return _OBSERVATIONS[full]


# ------------------------------------------------------------------------------------------
# Image resize
# ------------------------------------------------------------------------------------------
# (H, W, C) -> (rw, rh)
RESIZE_GEOMETRY = {
    "up": ((24, 32, 3), (84, 84)),              # both border clamps of every row and column
    "up_tiny": ((5, 7, 3), (84, 84)),           # most output pixels sit in a clamp
    "identity_c1": ((37, 53, 1), (53, 37)),
    "shrink_x_grow_y_c4": ((37, 53, 4), (20, 50)),
    "one_row": ((1, 9, 3), (5, 3)),             # s0 = s1 = 0 on every row
    "area": ((96, 128, 3), (64, 48)),           # exact 2x in both axes: the 2x2 mean
    "half_x_only": ((96, 128, 3), (64, 50)),    # exact 2x in x alone: bilinear
    "one_pixel": ((48, 64, 3), (1, 1)),
}
RESIZE_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}
AFFINE = (2.0, -1.0)
# the f32 resize has no area path for one axis alone either; "area" and "half_x_only" are its 2x cases
GRID_CAP = 16384 * 256
BIG = (600, 100, 100, (84, 84))  # 600 * 84 * 84 = 4 233 600 output pixels: a second grid-stride pass


def crops(rw, rh):
    """(y0, x0, ch, cw): full, one pixel at the far corner, a ragged interior window (deduplicated)."""
    out = [(0, 0, rh, rw), (rh - 1, rw - 1, 1, 1), (rh // 3, rw // 4, max(1, rh // 2), max(1, (rw * 3) // 5 - 1))]
    for y0, x0, ch, cw in out:
        assert 0 <= y0 and 0 <= x0 and y0 + ch <= rh and x0 + cw <= rw
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def u8_sources(name, n=2):
    (H, W, C), _ = RESIZE_GEOMETRY[name]
    src = np.random.default_rng(sum(map(ord, name))).integers(0, 256, (n, H, W, C), dtype=np.uint8)
    src.setflags(write=False)
    return src


@functools.lru_cache(maxsize=None)
def resized_u8(name):
    """oracle.image.resize_u8 of every source of a geometry, u8 [n, rh, rw, C]."""
    out = np.stack([OI.resize_u8(s, RESIZE_GEOMETRY[name][1]) for s in u8_sources(name)])
    out.setflags(write=False)
    return out


def policy_u8(name, crop):
    """oracle.image.policy_image of every source: f32 [n, C, ch, cw]."""
    return np.stack([OI.policy_image(s, RESIZE_GEOMETRY[name][1], crop, *AFFINE) for s in u8_sources(name)])


@functools.lru_cache(maxsize=None)
def depth_sources(name, special, n=2):
    """f32 [n, H, W] depth frames of a geometry; special: a patch of +inf (the renderer's misses), two
    leading rows of 0 (invalid) and one NaN."""
    (H, W, _), _ = RESIZE_GEOMETRY[name]
    src = np.random.default_rng(1 + sum(map(ord, name))).uniform(0.1, 3.0, (n, H, W)).astype(np.float32)
    if special:
        src[:, :min(2, H - 1)] = 0.0
        src[:, H // 2:H // 2 + max(1, H // 4), W // 3:W // 3 + max(1, W // 4)] = np.inf
        src[:, H - 1, W - 1] = np.nan
    src.setflags(write=False)
    return src


@functools.lru_cache(maxsize=None)
def resized_depth(name, special):
    with np.errstate(invalid="ignore"):  # inf * 0 next to the patch is NaN, in OpenCV as here
        out = np.stack([OI.resize_f32(s, RESIZE_GEOMETRY[name][1]) for s in depth_sources(name, special)])
    out.setflags(write=False)
    return out


def same_bits(got, want):
    """NaN at the same positions, every other f32 element equal bit for bit (so +inf, -0.0 and
    subnormals count)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan)
                and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


@functools.lru_cache(maxsize=None)
def big_u8():
    """(src u8 [600, 100, 100, 3], policy f32 [600, 3, 84, 84]) past the grid cap."""
    n, H, W, size = BIG
    src = np.random.default_rng(31).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return src, np.stack([OI.policy_image(s, size, (0, 0, size[1], size[0]), *AFFINE) for s in src])


@functools.lru_cache(maxsize=None)
def big_depth():
    n, H, W, size = BIG
    src = np.random.default_rng(32).uniform(0.1, 3.0, (n, H, W)).astype(np.float32)
    return src, np.stack([OI.resize_f32(s, size) for s in src])


# ------------------------------------------------------------------------------------------
# SARNN
# ------------------------------------------------------------------------------------------
# (S, K, ncam).  att_ocg3(K) = 4: K 3, 4; 8: K 7, 8, 13..16 (two groups from 13); K % 8 == 0 takes the other
# branch of sarnn_conv_groups.  S = 8: a 2x2 map, one band of two rows; 9, 23: odd maps; 128: 4-row bands
ATTENTION_CASES = [(8, 3, 1), (9, 8, 3), (23, 4, 2), (20, 7, 2), (20, 13, 2), (20, 16, 4), (64, 16, 2), (128, 16, 1)]
KNOWN_ANSWER_CASES = [(20, 5), (64, 5)]
KNOWN_ANSWER_BAR = 2.0 ** -18



@functools.lru_cache(maxsize=None)
def constant_image_case(S, K, ncam=2, n=3):
    """(model, images f32 [n, ncam, 3, S, S]): every (env, camera, channel) plane a constant of its own, so
    the logits of a camera are the same at every pixel."""
    from robomanipbaselines_amd.policy.sarnn.sarnn_model import SarnnModel

    torch.manual_seed(300 + S + K)
    model = SarnnModel(7, ncam, [S, S], K, 50).eval().requires_grad_(False)
    levels = torch.rand(n, ncam, 3, 1, 1, generator=torch.Generator().manual_seed(S))
    return model, levels.expand(n, ncam, 3, S, S).contiguous()


# (hidden, state_dim, key_dim): a full block; the wave boundary from both sides; one unit and no keys;
# input and decoder loops that wrap the 128 threads; the input limit of 256
LSTM_CASES = [(128, 7, 20), (64, 7, 20), (65, 7, 20), (1, 1, 0), (50, 130, 120), (128, 1, 255)]
LSTM_ENVS, LSTM_STEPS = 5, 4


@functools.lru_cache(maxsize=None)
def lstm_case(hd, sd, kd):
    """(lstm, dec, xs, want, ref_err): LSTMCell + decoder of that size, LSTM_STEPS inputs [n, sd + kd], per
    step the f64 (pred, h, c) of the recurrence fed its own state back, and the measured max
    |torch-CPU fp32 - f64| of the reference route over all steps and outputs."""
    from test_sarnn_gpu import _lstm_f64, _lstm_modules

    n = LSTM_ENVS
    lstm, dec = _lstm_modules(sd + kd, hd, sd, 40 + hd + sd + kd)
    g = torch.Generator().manual_seed(41 + hd)
    xs = [torch.rand(n, sd + kd, generator=g) for _ in range(LSTM_STEPS)]
    h32, c32 = torch.zeros(n, hd), torch.zeros(n, hd)
    h64, c64 = torch.zeros(n, hd, dtype=torch.float64), torch.zeros(n, hd, dtype=torch.float64)
    want, ref_err = [], 0.0
    for x in xs:
        h32, c32 = lstm(x, (h32, c32))
        p32 = dec(h32)
        p64, h64, c64 = _lstm_f64(x, h64, c64, lstm, dec)
        want.append((p64, h64, c64))
        ref_err = max(ref_err, *(float((a.double() - b).abs().max()) for a, b in ((p32, p64), (h32, h64), (c32, c64))))
    return lstm, dec, xs, want, ref_err
