"""rmbx_pointcloud_fps at its edges, bitwise against oracle/pointcloud.py (kept count, raw f64 points,
normalised f32 cloud) on the frames of tests/observation_cases.py; tests/test_observation_cases.py
shows on the oracle alone that each frame reaches the edge it names.

  * tie scenes: flat depth and flat colours, as the substitute renderer draws them, tie the running
    maximum in 20 to 135 of the FPS steps, in all three stages of the kernel's argmax (a lane's slots,
    the wave shuffle, the 16 waves through LDS); at 1024 pixels (one slot per lane), 8192 (all eight
    slots, the limit), 8190 (a ragged last slot) and 391 (fewer pixels than lanes)
  * kept counts 1 (the last pixel: slot 7 of lane 1023), K, K + 1, 2 with K = 8, K = 1, K = 9000 (the
    trailing slots through nine passes of the strided tail loop), and a cloud whose every round is
    all-zero
  * a missing min / max bound (NULL), strict comparisons at both z bounds, and NaN, -0.0, negative,
    +-inf and subnormal depths
  * each env of a mixed batch equals the same env alone; n = 0; rejections before any launch
"""

import numpy as np
import pytest
import torch

import observation_cases as C
from test_pointcloud_gpu import HI, LO, STATS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(d, rgb, K, lo=LO, hi=HI):
    from robomanipbaselines_amd import kernels as K_

    if d.ndim == 2:
        d, rgb = d[None], rgb[None]
    out, cnt, raw = K_.pointcloud_fps(torch.from_numpy(np.ascontiguousarray(d)).to(DEV),
                                      torch.from_numpy(np.ascontiguousarray(rgb)).to(DEV), C.FOVY, K, STATS, lo, hi,
                                      raw=True)
    return out.cpu().numpy(), cnt.cpu().numpy(), raw.cpu().numpy()


def _constant(n, H, W):
    """Device (depth, rgb) of n flat frames at depth 0.5."""
    return torch.full((n, H, W), 0.5, device=DEV), torch.zeros((n, H, W, 3), dtype=torch.uint8, device=DEV)


def _check(got, e, want, what):
    out, cnt, raw = got
    norm_ref, raw_ref, count_ref = want
    assert cnt[e] == count_ref, what
    bad = np.flatnonzero((raw[e] != raw_ref).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(raw_ref)} points differ, first at slot {bad[0]}"
    assert np.array_equal(out[e], norm_ref), what


@pytest.mark.parametrize("H,W,K", C.FPS_SIZES)
def test_fps_tie_scenes(H, W, K):
    frames = [C.tie_scene(name, H, W) for name in C.TIE_SCENES]
    got = _run(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), K)
    for e, name in enumerate(C.TIE_SCENES):
        _check(got, e, C.observation(("tie", name, H, W), *frames[e], K), f"{name} {H}x{W}")


@pytest.mark.parametrize("name", list(C.count_cases()))
def test_fps_counts_around_k(name):
    d, rgb, K, kept = C.count_cases()[name]
    got = _run(d, rgb, K)
    assert got[1][0] == kept
    _check(got, 0, C.observation(name, d, rgb, K), name)


@pytest.mark.parametrize("name", list(C.bound_cases()))
def test_fps_missing_bounds(name):
    lo, hi = C.bound_cases()[name]
    d, rgb = C.bounds_frame()
    _check(_run(d, rgb, 128, lo, hi), 0, C.observation("bounds", d, rgb, 128, lo, hi), name)


def test_fps_bounds_are_strict():
    d, rgb = C.strict_frame()
    got = _run(d, rgb, 8, C.Z_LO, HI)
    assert got[1][0] == C.STRICT_KEPT
    _check(got, 0, C.observation("strict", d, rgb, 8, C.Z_LO, HI), "strict bounds")


def test_fps_odd_depth_values():
    d, rgb, ordinary = C.odd_depth_frame()
    got = _run(d, rgb, 64)
    assert got[1][0] == ordinary + 1  # of NaN, -0.0, negative, +inf, -inf, subnormal: the subnormal
    _check(got, 0, C.observation("odd", d, rgb, 64), "odd depth values")


def test_fps_envs_are_independent_and_empty_batch():
    from robomanipbaselines_amd import kernels as K_

    d, rgb, K = C.mixed_batch()
    batch = _run(d, rgb, K)
    assert batch[1].tolist()[2:] == [0, 1] and not batch[0][2].any() and not batch[2][2].any()
    for e in range(4):
        alone = _run(d[e], rgb[e], K)
        for b, a in zip(batch, alone):
            assert np.array_equal(b[e], a[0]), e
        if e != 2:  # the reference raises on an empty cloud; the kernel emits zeros
            _check(batch, e, C.observation(("mixed", e), d[e], rgb[e], K), f"mixed batch env {e}")
    out, cnt, raw = K_.pointcloud_fps(*_constant(0, 32, 32), C.FOVY, K, STATS, LO, HI, raw=True)
    assert out.shape == raw.shape == (0, K, 6) and cnt.shape == (0,)


def test_fps_rejections():
    from robomanipbaselines_amd import kernels as K_

    def call(H, W, K, n=1):
        return K_.pointcloud_fps(*_constant(n, H, W), C.FOVY, K, STATS, LO, HI)

    with pytest.raises(ValueError, match="exceeds 8192 pixels"):
        call(91, 91, 64)
    with pytest.raises(ValueError, match="K must be positive"):
        call(32, 32, 0)
    with pytest.raises(ValueError, match="exceeds 8192 pixels"):  # an empty batch is checked all the same
        call(91, 91, 64, n=0)
    torch.cuda.synchronize()
    assert call(90, 91, 64)[1].item() == 8190  # nothing was launched: the device still serves the next call
