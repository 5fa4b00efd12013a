"""--perturb on the host: the spec parser, the episode constants of common/perturb.py against the
independent restatement (tests/perturb_cases.py), their properties, the oracle's own noise moments,
the flag and its pass-through.  No device."""

import importlib.util
import os

import numpy as np
import pytest
from conftest import ROOT

import perturb_cases as PT
from robomanipbaselines_amd.common import perturb as P


# -- parse_spec -------------------------------------------------------------------------------------
def test_parse_spec_every_key_and_the_defaults():
    s = P.parse_spec(["brightness=20", "contrast=0.25", "gain=0.5", "noise=4", "occluder=0.3", "state_noise=0.125"])
    assert (s.brightness, s.contrast, s.gain, s.noise, s.occluder, s.state_noise) == (20.0, 0.25, 0.5, 4.0, 0.3, 0.125)
    assert s.touches_images and s.occ_size(480, 640) == (144, 192)
    d = P.parse_spec([])
    assert d == P.PerturbSpec() and d.as_dict() == dict.fromkeys(
        ("brightness", "contrast", "gain", "noise", "occluder", "state_noise"), 0.0)
    assert not d.touches_images and d.occ_size(480, 640) == (0, 0)
    assert not P.parse_spec(["state_noise=1"]).touches_images
    one = P.parse_spec(["noise=0.1"])
    assert one.noise == float(np.float32(0.1)) and one.brightness == 0.0  # the f32 value the kernel reads
    with pytest.raises(Exception):  # frozen
        s.noise = 1.0
    # the edges of the ranges
    assert P.parse_spec(["brightness=255"]).brightness == 255.0 and P.parse_spec(["occluder=1"]).occ_size(6, 10) == (6, 10)
    assert P.parse_spec(["occluder=1.0"]).occluder == 1.0 and P.parse_spec(["contrast=0"]).contrast == 0.0
    # the spec survives its own dict (result file, trace header) and names every key when printed
    assert P.spec_from_dict(s.as_dict()) == s and P.spec_from_dict(one.as_dict()) == one
    assert str(s) == "brightness=20 contrast=0.25 gain=0.5 noise=4 occluder=0.3 state_noise=0.125"


@pytest.mark.parametrize("items,what", [
    (["blur=1"], "unknown key"), (["noise=1", "noise=2"], "twice"), (["noise"], "KEY=VALUE"), (["=3"], "KEY=VALUE"),
    (["noise="], "KEY=VALUE"), (["noise=abc"], "not a number"), (["noise=nan"], "outside"), (["noise=inf"], "outside"),
    (["noise=-1"], "outside"), (["brightness=256"], "outside"), (["brightness=-0.5"], "outside"),
    (["contrast=1"], "outside"), (["contrast=-0.1"], "outside"), (["gain=1.0"], "outside"), (["gain=-1"], "outside"),
    (["occluder=1.01"], "outside"), (["occluder=-0.1"], "outside"), (["state_noise=-2"], "outside"),
])
def test_parse_spec_errors(items, what):
    with pytest.raises(ValueError, match=what):
        P.parse_spec(items)


# -- episode_params ---------------------------------------------------------------------------------
SPEC = P.parse_spec(["brightness=30", "contrast=0.4", "gain=0.2", "occluder=0.3"])
EPISODES = np.array([0, 1, 2, 77, 4117, 2**31 - 1, -1, -2**31], dtype=np.int32)  # negative bit patterns too


@pytest.mark.parametrize("seed", [0, 3, 2**40 + 7, 2**64 - 1])
@pytest.mark.parametrize("camera", [0, 2, 255])
def test_episode_params_equal_the_restatement(seed, camera):
    H, W = 48, 64
    got = P.episode_params(seed, EPISODES, SPEC, camera, H, W)
    occ_h, occ_w = SPEC.occ_size(H, W)
    assert (got["occ_h"], got["occ_w"]) == (occ_h, occ_w) == (14, 19)
    for r, e in enumerate(EPISODES):
        want = PT.constants(seed, int(e), camera, H, W, SPEC.brightness, SPEC.contrast, SPEC.gain, occ_h, occ_w)
        assert got["b"][r].tobytes() == np.float32(want["b"]).tobytes(), (seed, e)
        assert got["c"][r].tobytes() == np.float32(want["c"]).tobytes(), (seed, e)
        assert got["g"][r].tobytes() == want["g"].astype(np.float32).tobytes(), (seed, e)
        assert (int(got["y0"][r]), int(got["x0"][r])) == (want["y0"], want["x0"]), (seed, e)
        assert got["colour"][r].tobytes() == want["colour"].tobytes(), (seed, e)
    assert got["b"].dtype == got["c"].dtype == got["g"].dtype == got["colour"].dtype == np.float32


def test_episode_params_properties():
    H, W, seed = 6, 10, 5
    ep = np.arange(-50, 350, dtype=np.int32)
    per_cam = [P.episode_params(seed, ep, SPEC, cam, H, W) for cam in (0, 1, 2)]
    a = per_cam[0]
    # lighting: one per episode, shared by the cameras, different between episodes
    for other in per_cam[1:]:
        for k in ("b", "c", "g"):
            assert other[k].tobytes() == a[k].tobytes(), k
        assert (other["y0"] != a["y0"]).any() or (other["x0"] != a["x0"]).any()  # the occluders are per camera
    assert len(np.unique(a["b"])) > 390 and len(np.unique(a["c"])) > 390 and len(np.unique(a["g"])) > 1100
    # ranges
    assert (np.abs(a["b"]) <= SPEC.brightness).all() and (np.abs(a["c"] - 1) <= SPEC.contrast + 1e-7).all()
    assert (np.abs(a["g"] - 1) <= SPEC.gain + 1e-7).all() and (a["c"] > 0).all() and (a["g"] > 0).all()
    assert ((a["colour"] >= 0) & (a["colour"] <= 255) & (a["colour"] == np.floor(a["colour"]))).all()
    # the rectangle lies inside the image, and moves
    for f in (0.1, 0.3, 0.5, 0.99, 1.0):
        spec = P.parse_spec([f"occluder={f}"])
        for (h, w) in ((6, 10), (5, 7), (480, 640)):
            p = P.episode_params(seed, ep, spec, 1, h, w)
            oh, ow = spec.occ_size(h, w)
            if oh == 0:
                assert (p["y0"] == 0).all() and (p["x0"] == 0).all() and not p["colour"].any()
                continue
            assert (p["y0"] >= 0).all() and (p["y0"] + oh <= h).all(), (f, h, w)
            assert (p["x0"] >= 0).all() and (p["x0"] + ow <= w).all(), (f, h, w)
            if f == 1.0:
                assert (oh, ow) == (h, w) and not p["y0"].any() and not p["x0"].any()
            elif h - oh >= 2:
                assert len(np.unique(p["y0"])) > 1
    # without the components: the neutral constants
    z = P.episode_params(seed, ep, P.PerturbSpec(), 0, H, W)
    assert not z["b"].any() and (z["c"] == 1).all() and (z["g"] == 1).all()
    with pytest.raises(ValueError, match="camera"):
        P.episode_params(seed, ep, SPEC, 256, H, W)


def test_uniform_is_exact_and_open():
    w = np.array([0, 1, 511, 512, 2**31, 2**32 - 1], dtype=np.uint32)
    u = PT.uniform(w)
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
    want = ((w >> 9).astype(np.float64) + 0.5) * 2.0**-23
    assert (u.astype(np.float64) == want).all()


# -- the oracle's own noise ---------------------------------------------------------------------------
def test_oracle_noise_moments():
    """A constant frame of 128 with noise=8: 8 rows of 64 x 64 x 3, N = 98,304 elements.  The mean of
    out - 128 within 5 standard errors (5 * 8 / sqrt(N) = 0.13); the standard deviation within 0.1 of
    sqrt(64 + 1/12) = 8.005 (rounding adds the 1/12), 5 relative standard errors of 1 / sqrt(2 N)."""
    n, H, W = 8, 64, 64
    rgb = np.full((n, H, W, 3), 128, np.uint8)
    ep, dr = np.arange(10, 10 + n, dtype=np.int32), np.arange(n, dtype=np.int32) * 3
    out, pre = PT.apply_oracle(rgb, 11, ep, dr, 1, noise=8.0)
    d = out.astype(np.float64) - 128.0
    N = d.size
    assert N == 98304 and out.min() > 0 and out.max() < 255  # 128 +- 5.77 sigma stays inside: no clamping
    assert abs(d.mean()) <= 5 * 8 / np.sqrt(N), d.mean()
    assert abs(d.std() - np.sqrt(64 + 1 / 12)) <= 0.1, d.std()
    assert np.abs(pre - 128.0).max() <= 8 * 5.78
    # rows are different streams; the same (episode, draw, camera) is the same stream
    assert not (out[0] == out[1]).all()
    again, _ = PT.apply_oracle(rgb[:1], 11, ep[3:4], dr[3:4], 1, noise=8.0)
    assert again.tobytes() == out[3:4].tobytes()


def test_oracle_identity_and_forms():
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8)
    ep = dr = np.zeros(2, np.int32)
    out, pre = PT.apply_oracle(rgb, 1, ep, dr, 0)
    assert out.tobytes() == rgb.tobytes() and (pre == rgb).all()
    s = PT.policy_form(rgb, 4)
    assert s.shape == (2, 2, 3, 16) and not s[..., 12:].any()
    assert s[1, 1, 2, 7] == rgb[1, 3, 4, 1]  # (dy, dx, k) = (1, 0, 1) of cell (1, 2): pixel (3, 4)
    f = PT.policy_form(rgb, 0, (0.5, 0.4, 0.3), (0.2, 0.25, 0.5))
    assert f.shape == (2, 3, 4, 6) and f.dtype == np.float32
    assert f[0, 2, 1, 5] == (np.float32(rgb[0, 1, 5, 2]) / np.float32(255) - np.float32(0.3)) / np.float32(0.5)
    assert PT.bf16_bits(np.array([1.0, 1.00390625, 1.01171875, -2.0], np.float32)).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC000]


# -- the flag ---------------------------------------------------------------------------------------
def test_the_flag_is_parsed_and_refuses_a_bad_spec():
    from robomanipbaselines_amd.policy.mlp.rollout_mlp import RolloutMlp

    ro = RolloutMlp.__new__(RolloutMlp)  # the parser alone: no env, no device
    ro.setup_args(argv=[])
    assert ro.args.perturb is None
    ro.setup_args(argv=["--perturb", "noise=4", "occluder=0.25"])
    assert ro.args.perturb == ["noise=4", "occluder=0.25"]
    with pytest.raises(ValueError, match="unknown key"):
        ro.setup_args(argv=["--perturb", "fog=1"])
    with pytest.raises(ValueError, match="outside"):
        ro.setup_args(argv=["--perturb", "contrast=1.5"])


def test_bench_policy_passes_the_flag_through(monkeypatch):
    spec = importlib.util.spec_from_file_location("bench_policy_perturb_under_test",
                                                  os.path.join(ROOT, "scripts", "bench_policy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    on = mod.rollout_argv(mod.parse_args(["Act", "--perturb", "noise=4", "gain=0.1"]))
    i = on.index("--perturb")
    assert on[i + 1:i + 3] == ["noise=4", "gain=0.1"]
    assert "--perturb" not in mod.rollout_argv(mod.parse_args(["Act"]))


def test_kernel_wrapper_rejections_before_the_device():
    """kernels.image_perturb checks shapes, dtypes and devices itself, so a wrong call fails the same
    way with or without a GPU."""
    import torch

    from robomanipbaselines_amd import kernels as K

    rgb = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    ep = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        K.image_perturb(rgb, 0, ep, ep, 0, rgb_out=rgb)
    with pytest.raises(ValueError, match="seed"):
        K.image_perturb(rgb, -1, ep, ep, 0, rgb_out=rgb)
