"""The per-episode observation perturbation on the device (include/rmbx.h, rmbx_image_perturb):
the kernel against the numpy restatement fed with the device's own normals (bitwise) and against the
independent f64-normal oracle (tests/perturb_cases.py), its layout independence, masks, aliasing and
argument errors; then --perturb in the rollouts, the streaming loop and bin/Replay.py --as_seen."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import perturb_cases as PT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, CAM = 2**40 + 7, 2
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
NORMAL_BAR = 4e-6  # the bar tests/test_sampler_noise_gpu.py holds the device normals to
# n, H, W, policy forms: L = 105 (Philox tail block, rows off a 4-byte boundary); W % 4 != 0, even; the
# wide path; 7.4 M elements: past the grid cap, so the stride loop runs
SHAPES = {"5x7": (2, 5, 7, (0, 1)), "6x10": (3, 6, 10, (0, 1, 2, 3, 4)), "48x64": (5, 48, 64, (0, 1, 2, 3, 4)),
          "480x640": (8, 480, 640, (0, 1, 2, 3, 4))}
# strengths: brightness <= 64 and noise <= 32 keep |v| below 1024 (the oracle allowance relies on it)
COMPONENTS = {"brightness": dict(brightness=40.0), "contrast": dict(contrast=0.5), "gain": dict(gain=0.3),
              "occluder": dict(occluder=0.4), "noise": dict(noise=8.0),
              "all": dict(brightness=64.0, contrast=0.5, gain=0.3, occluder=0.4, noise=32.0)}
FORM_DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.bfloat16, 3: torch.float32, 4: torch.uint8}
EPISODES = np.array([4117, -1, 0, 5, 2**31 - 1, 77, 6, 1], dtype=np.int32)
DRAWS = np.array([0, 3, 0, 250, 7, 1, 2**20, 9], dtype=np.int32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _kw(comp, H, W):
    """Kernel / restatement keywords of a component set (occluder fraction -> pixels)."""
    kw = dict(comp)
    f = kw.pop("occluder", 0.0)
    kw["occ_h"], kw["occ_w"] = int(np.floor(f * H)), int(np.floor(f * W))
    return kw


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The fixed inputs of a shape and, computed once, the device's normals of its rows."""
    from robomanipbaselines_amd import kernels as K

    n, H, W, forms = SHAPES[shape]
    rgb = np.random.default_rng(1234).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    ep, dr = EPISODES[:n].copy(), DRAWS[:n].copy()
    z = torch.empty((1, n, H * W * 3), dtype=torch.float32, device=DEV)
    K.philox_normal(SEED, _t(ep), _t(dr), z, plane0=PT.PLANE_NOISE + CAM)
    return rgb, ep, dr, z[0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _z64(shape):
    rgb, ep, dr, _ = _case(shape)
    return PT.normals64(SEED, ep, dr, CAM, rgb[0].size)


def _new_policy(form, n, H, W, fill=None):
    shape = (n, 3, H, W) if form < 2 else (n, H // 2, W // 2, 16)
    if fill is None:
        return torch.empty(shape, dtype=FORM_DTYPE[form], device=DEV)
    return torch.full(shape, fill, dtype=FORM_DTYPE[form], device=DEV)


def _bits(policy):
    """numpy view of a policy tensor that compares bitwise (bf16 as uint16)."""
    if policy.dtype == torch.bfloat16:
        return policy.view(torch.int16).cpu().numpy().view(np.uint16)
    return policy.cpu().numpy()


def _run(rgb, ep, dr, forms, kw, camera=CAM, seed=SEED, active=None, in_place=False):
    """The kernel's outputs: (rgb_out u8, {form: bits}).  rgb_out and the first form leave in one call,
    the other forms in calls of their own."""
    from robomanipbaselines_amd import kernels as K

    n, H, W, _ = rgb.shape
    src, e, d = _t(rgb), _t(ep), _t(dr)
    out = src if in_place else torch.empty_like(src)
    got = {}
    for i, form in enumerate(forms):
        pol = _new_policy(form, n, H, W)
        K.image_perturb(src, seed, e, d, camera, rgb_out=out if i == 0 else None, policy=pol, mean=MEAN, std=STD,
                        active=active, **kw)
        got[form] = _bits(pol)
    if not forms:
        K.image_perturb(src, seed, e, d, camera, rgb_out=out, active=active, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), got


def _forms_equal(got, u8, what):
    for form, bits in got.items():
        want = PT.policy_form(u8, form, MEAN, STD)
        assert bits.dtype == want.dtype and bits.shape == want.shape, (what, form)
        assert bits.tobytes() == want.tobytes(), (what, form, int((bits != want).sum()))


# -- 1. identity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_zero_spec_is_the_identity(shape):
    rgb, ep, dr, _ = _case(shape)
    out, got = _run(rgb, ep, dr, SHAPES[shape][3], {})
    assert out.tobytes() == rgb.tobytes()
    _forms_equal(got, rgb, shape)
    for form in (2, 3, 4):
        if form in got:
            assert not got[form][..., 12:].any()


@torch.no_grad()
def test_zero_spec_forms_equal_the_renderers():
    """One small rendered Cable frame: each of the five forms is bitwise what Renderer.render(policy=)
    writes for the same frame, mean and std."""
    import render_cases as RC
    from robomanipbaselines_amd import kernels as K
    from robomanipbaselines_amd.render import Renderer

    W, H = 104, 72  # the frame of tests/test_render_full_gpu.py
    arrays, eng = RC.asset_engine("ur5e_cable", DEV)
    rnd = Renderer(arrays, DEV, width=W, height=H)
    n = eng.n_env
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=DEV)
    rnd.render(eng, "front", rgb=rgb)
    assert len(torch.unique(rgb)) > 20
    ep = dr = torch.zeros(n, dtype=torch.int32, device=DEV)
    for form in range(5):
        want, got = _new_policy(form, n, H, W), _new_policy(form, n, H, W)
        rnd.render(eng, "front", policy=want, mean=MEAN, std=STD)
        K.image_perturb(rgb, 3, ep, dr, 0, policy=got, mean=MEAN, std=STD)
        assert _bits(got).tobytes() == _bits(want).tobytes(), form


# -- 2. exact against the device's normals ----------------------------------------------------------
@pytest.mark.parametrize("comp", list(COMPONENTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exact_against_the_restatement_with_device_normals(shape, comp):
    rgb, ep, dr, z32 = _case(shape)
    n, H, W, forms = SHAPES[shape]
    kw = _kw(COMPONENTS[comp], H, W)
    want = PT.apply_exact(rgb, SEED, ep, dr, CAM, z32=z32, **kw)
    out, got = _run(rgb, ep, dr, forms, kw)
    diff = out != want
    assert not diff.any(), (shape, comp, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert (out != rgb).mean() > 0.05, (shape, comp)  # the component does something
    _forms_equal(got, want, (shape, comp))


# -- 3. against the independent oracle --------------------------------------------------------------
@pytest.mark.parametrize("comp", list(COMPONENTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_independent_oracle(shape, comp):
    """An element may differ from the f64-normal oracle, by one level, only where the oracle's
    pre-rounding value lies within tau = sigma * NORMAL_BAR + 5 * 2^-14 of a half-integer (the device
    normal's error scaled by sigma, plus five f32 roundings of values below 1024); such elements are
    at most 0.5 % (expected: about 2 tau), asserted from the oracle alone."""
    rgb, ep, dr, _ = _case(shape)
    n, H, W, forms = SHAPES[shape]
    kw = _kw(COMPONENTS[comp], H, W)
    sigma = kw.get("noise", 0.0)
    want, pre = PT.apply_oracle(rgb, SEED, ep, dr, CAM, z64=_z64(shape) if sigma > 0 else None, **kw)
    assert np.abs(pre).max() < 1024
    tau = sigma * NORMAL_BAR + 5 * 2.0**-14
    near = PT.near_tie(pre, tau)
    print(f"\n{shape} {comp}: near-tie share {near.mean():.2e} (tau {tau:.2e})")
    assert near.mean() <= 0.005, (shape, comp, near.mean())
    out, got = _run(rgb, ep, dr, forms, kw)
    d = out.astype(np.int32) - want.astype(np.int32)
    print(f"{shape} {comp}: differing elements {int((d != 0).sum())} of {d.size}")
    assert not d[~near].any(), (shape, comp, int((d[~near] != 0).sum()))
    assert np.abs(d).max() <= 1, (shape, comp)
    for form, bits in got.items():
        exp, free = PT.policy_form(want, form, MEAN, STD), ~PT.layout(near, form)
        assert (bits[free] == exp[free]).all(), (shape, comp, form)


# -- 4. saturation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 255])
@pytest.mark.parametrize("shape", ["5x7", "48x64"])
def test_saturation_clamps(shape, level):
    _, ep, dr, z32 = _case(shape)
    n, H, W, forms = SHAPES[shape]
    rgb = np.full((n, H, W, 3), level, np.uint8)
    kw = dict(noise=32.0, brightness=64.0)
    want = PT.apply_exact(rgb, SEED, ep, dr, CAM, z32=z32, **kw)
    _, pre = PT.apply_oracle(rgb, SEED, ep, dr, CAM, **kw)
    out, got = _run(rgb, ep, dr, forms, kw)
    assert out.tobytes() == want.tobytes()
    _forms_equal(got, want, (shape, level))
    over, under = pre > 256, pre < -1
    assert (over if level else under).sum() > 10  # the frame does leave the range
    assert (out[over] == 255).all() and (out[under] == 0).all()  # clamped, never wrapped


# -- 5. layout independence ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x7", "6x10", "48x64"])
def test_a_row_does_not_depend_on_the_layout(shape):
    n0, H, W, forms = SHAPES[shape]
    n = 5
    rgb = np.random.default_rng(7).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    ep, dr = EPISODES[:n], DRAWS[:n]
    kw = _kw(COMPONENTS["all"], H, W)
    full, full_forms = _run(rgb, ep, dr, forms, kw)
    perm = np.array([3, 0, 4, 2, 1])
    shuffled, shuffled_forms = _run(rgb[perm], ep[perm], dr[perm], forms, kw)
    assert shuffled.tobytes() == full[perm].tobytes()
    for f in forms:
        assert shuffled_forms[f].tobytes() == full_forms[f][perm].tobytes(), f
    for r in (0, 3):
        alone, alone_forms = _run(rgb[r:r + 1], ep[r:r + 1], dr[r:r + 1], forms, kw)
        assert alone.tobytes() == full[r:r + 1].tobytes(), r
        for f in forms:
            assert alone_forms[f].tobytes() == full_forms[f][r:r + 1].tobytes(), (r, f)
    pair, _ = _run(rgb[1:3], ep[1:3], dr[1:3], (), kw)
    assert pair.tobytes() == full[1:3].tobytes()
    # another camera, draw, episode or seed: another noise (and another occluder per camera / episode)
    noise = dict(noise=8.0)
    base, _ = _run(rgb, ep, dr, (), noise)
    assert _run(rgb, ep, dr, (), noise, camera=CAM + 1)[0].tobytes() != base.tobytes()
    other_draw = _run(rgb, ep, dr + 1, (), noise)[0]
    assert all(other_draw[r].tobytes() != base[r].tobytes() for r in range(n))
    assert _run(rgb, ep + 1, dr, (), noise)[0].tobytes() != base.tobytes()
    assert _run(rgb, ep, dr, (), noise, seed=SEED + 1)[0].tobytes() != base.tobytes()
    # the draw does not move the episode constants
    const = _kw(dict(brightness=40.0, contrast=0.5, gain=0.3, occluder=0.4), H, W)
    assert _run(rgb, ep, dr + 5, (), const)[0].tobytes() == _run(rgb, ep, dr, (), const)[0].tobytes()


def test_the_cameras_of_an_episode_share_the_lighting():
    """b, c and g recovered from noise-free runs on constant frames are those of common/perturb.py's
    episode_params, the same for two cameras and different between episodes."""
    from robomanipbaselines_amd.common import perturb as P

    n, H, W = 5, 6, 10
    ep, dr = EPISODES[:n], DRAWS[:n]
    spec = P.parse_spec(["brightness=60", "contrast=0.5", "gain=0.4"])
    k = P.episode_params(SEED, ep, spec, 0, H, W)
    f32 = np.float32

    def const(level, **kw):
        rgb = np.full((n, H, W, 3), level, np.uint8)
        a, b = _run(rgb, ep, dr, (), kw, camera=0)[0], _run(rgb, ep, dr, (), kw, camera=1)[0]
        assert a.tobytes() == b.tobytes()
        assert (a == a[:, :1, :1, :]).all()  # constant per row and channel
        return a[:, 0, 0, :].astype(np.float64)

    got_b = const(128, brightness=60.0)
    assert (got_b == np.rint(f32(128) + k["b"])[:, None]).all() and len(np.unique(got_b)) > 2
    got_c = const(255, contrast=0.5)
    assert (got_c == np.clip(np.rint(f32(127.5) * k["c"] + f32(127.5)), 0, 255)[:, None]).all()
    got_g = const(150, gain=0.4)
    assert (got_g == np.rint(f32(150) * k["g"])).all() and len(np.unique(got_g)) > 4


# -- 6. active, aliasing, errors -------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x7", "6x10", "48x64"])
def test_inactive_rows_are_not_written_and_in_place_equals_out_of_place(shape):
    from robomanipbaselines_amd import kernels as K

    n0, H, W, forms = SHAPES[shape]
    n = 4
    rgb = np.random.default_rng(9).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    ep, dr = EPISODES[:n], DRAWS[:n]
    kw = _kw(COMPONENTS["all"], H, W)
    full, full_forms = _run(rgb, ep, dr, forms, kw)
    active = torch.tensor([1, 0, 0, 1], dtype=torch.uint8, device=DEV)
    src, e, d = _t(rgb), _t(ep), _t(dr)
    out = torch.full_like(src, 9)
    for i, form in enumerate(forms):
        fill = 7 if form == 4 else -3.0
        pol = _new_policy(form, n, H, W, fill=fill)
        K.image_perturb(src, SEED, e, d, CAM, rgb_out=out if i == 0 else None, policy=pol, mean=MEAN, std=STD,
                        active=active, **kw)
        bits = _bits(pol)
        assert bits[[0, 3]].tobytes() == full_forms[form][[0, 3]].tobytes(), form
        assert bool((pol[1:3] == fill).all()), form
    got = out.cpu().numpy()
    assert got[[0, 3]].tobytes() == full[[0, 3]].tobytes() and (got[1:3] == 9).all()
    # in place
    same, _ = _run(rgb, ep, dr, forms[:1], kw, in_place=True)
    assert same.tobytes() == full.tobytes()


def test_argument_errors_launch_nothing():
    from robomanipbaselines_amd import _native as N
    from robomanipbaselines_amd import kernels as K

    n, H, W = 3, 6, 8
    rgb = torch.full((n + 1, H, W, 3), 5, dtype=torch.uint8, device=DEV)
    out = torch.full((n + 1, H, W, 3), 9, dtype=torch.uint8, device=DEV)
    pol = torch.full((n, 3, H, W), -3.0, dtype=torch.float32, device=DEV)
    s2d = torch.full((n, H // 2, W // 2, 16), 7, dtype=torch.uint8, device=DEV)
    ep = torch.arange(n, dtype=torch.int32, device=DEV)
    dr = torch.zeros(n, dtype=torch.int32, device=DEV)
    lib = N.load()

    def params(**over):
        v = dict(brightness=10.0, contrast=0.2, gain=0.2, noise_sigma=4.0, occ_h=2, occ_w=3)
        v.update(over)
        return N.PerturbParams(v["brightness"], v["contrast"], v["gain"], v["noise_sigma"], v["occ_h"], v["occ_w"],
                               (ctypes.c_float * 3)(*v.get("mean", MEAN)), (ctypes.c_float * 3)(*v.get("std", STD)))

    ok = dict(rgb=rgb.data_ptr(), rgb_out=out.data_ptr(), policy=pol.data_ptr(), dtype=0, p=params(), episode=ep.data_ptr(),
              draw=dr.data_ptr(), camera=1, n=n, H=H, W=W)
    elems = n * H * W * 3
    bad = [dict(rgb=None), dict(p=None), dict(episode=None), dict(draw=None), dict(rgb_out=None, policy=None),
           dict(n=0), dict(H=0), dict(W=-1), dict(H=8193), dict(n=2**20, H=1024, W=1024), dict(dtype=5), dict(dtype=-1),
           dict(camera=-1), dict(camera=256), dict(p=params(brightness=-1.0)), dict(p=params(brightness=256.0)),
           dict(p=params(contrast=1.0)), dict(p=params(contrast=-0.5)), dict(p=params(gain=1.0)),
           dict(p=params(noise_sigma=-1.0)), dict(p=params(noise_sigma=float("inf"))), dict(p=params(noise_sigma=float("nan"))),
           dict(p=params(occ_h=H + 1)), dict(p=params(occ_w=W + 1)), dict(p=params(occ_h=-1)),
           dict(p=params(std=(0.2, 0.0, 0.2))), dict(p=params(mean=(float("nan"), 0.0, 0.0))),
           dict(policy=s2d.data_ptr(), dtype=4, H=5, rgb_out=None), dict(policy=s2d.data_ptr(), dtype=2, W=7, rgb_out=None),
           dict(rgb_out=rgb.data_ptr() + 3 * W), dict(rgb_out=rgb.data_ptr() + elems - 1),  # overlaps, not equal
           dict(policy=rgb.data_ptr() + 4), dict(policy=out.data_ptr()), dict(policy=pol.data_ptr() + 2)]
    for over in bad:
        a = dict(ok)
        a.update(over)
        st = lib.rmbx_image_perturb(a["rgb"], a["rgb_out"], a["policy"], a["dtype"],
                                    None if a["p"] is None else ctypes.byref(a["p"]), ctypes.c_uint64(3), a["episode"],
                                    a["draw"], a["camera"], None, a["n"], a["H"], a["W"], N.stream_ptr())
        assert st == -1, {k: v for k, v in over.items() if k != "p"}
        with pytest.raises(ValueError, match="rmbx_image_perturb"):
            N.check(st)
    good = rgb[:n]
    for kw in (dict(seed=-1), dict(rgb=good.float()), dict(rgb=good[..., :2].contiguous()), dict(episode=ep[:2]),
               dict(draw=dr.long()), dict(rgb_out=out[:2]), dict(rgb_out=None, policy=None), dict(policy=pol[:, :2].contiguous()),
               dict(policy=pol.double()), dict(policy=s2d[:, :2].contiguous()), dict(active=torch.ones(n, device=DEV)),
               dict(episode=ep.cpu()), dict(rgb=good.permute(0, 2, 1, 3)), dict(camera=300), dict(mean=(0.0, 0.0))):
        a = dict(rgb=good, seed=3, episode=ep, draw=dr, camera=1, rgb_out=out[:n], policy=pol, noise=4.0)
        a.update(kw)
        with pytest.raises(ValueError):
            K.image_perturb(**a)
    torch.cuda.synchronize()
    assert (out == 9).all() and (pol == -3.0).all() and (s2d == 7).all() and (rgb == 5).all()
    K.image_perturb(good, 3, ep, dr, 1, rgb_out=out[:n], policy=pol, noise=4.0)
    assert (out[:n] != 9).any() and (pol != -3.0).all() and (out[n] == 9).all()


# -- rollouts ---------------------------------------------------------------------------------------
SPEC = ["brightness=20", "contrast=0.3", "gain=0.2", "noise=6", "occluder=0.25", "state_noise=0.05"]
BASE = ["--device", DEV, "--world_random_scale", "0.01", "0.01", "0.0", "--seed", "3", "--precision", "fp32"]


def _compose(policy):
    from test_stream_gpu import _compose as compose

    return compose(policy)


def _spec_kw(ro):
    s = ro.perturb_spec
    H, W = ro.env.renderer.height, ro.env.renderer.width
    occ_h, occ_w = s.occ_size(H, W)
    return dict(brightness=s.brightness, contrast=s.contrast, gain=s.gain, noise=s.noise, occ_h=occ_h, occ_w=occ_w)


def _expected_frame(ro, clean, episodes, draw, cam="front"):
    """The restatement (with the device's normals) of the frame the policy must read: u8 numpy."""
    from robomanipbaselines_amd import kernels as K

    n = clean.shape[0]
    ci = ro.env.camera_names.index(cam)
    seed = int(ro.args.seed)
    ep = np.asarray(episodes, np.int32)
    dr = np.full(n, draw, np.int32)
    z = torch.empty((1, n, clean[0].numel()), dtype=torch.float32, device=DEV)
    K.philox_normal(seed, _t(ep), _t(dr), z, plane0=PT.PLANE_NOISE + ci)
    return PT.apply_exact(clean.cpu().numpy(), seed, ep, dr, ci, z32=z[0].cpu().numpy(), **_spec_kw(ro))


def _capture_policy_rgb(ro, log):
    """Log (rollout_time_idx, clean frame, returned frame) of every policy_rgb call."""
    inner = ro.policy_rgb

    def spy(cam):
        frame = inner(cam)
        clean = ro.info["rgb_images"][cam]
        # info["rgb_images"] stays clean: it is the frame a plain render of this state gives
        plain = torch.empty_like(clean)
        ro.env.render_images(cam, rgb=plain)
        assert torch.equal(clean, plain) and frame.data_ptr() != clean.data_ptr()
        log.append((int(ro.rollout_time_idx), clean.clone(), frame.clone()))
        return frame

    ro.policy_rgb = spy


def _step_until(ro, log, count, limit=400):
    ro.reset()
    for _ in range(limit):
        ro.step_once()
        if len(log) >= count:
            return
    raise AssertionError("the rollout never reached its inferences")


# -- 7. state noise ---------------------------------------------------------------------------------
def test_state_noise():
    from robomanipbaselines_amd import kernels as K
    from robomanipbaselines_amd.common.perturb import parse_spec
    from robomanipbaselines_amd.common.rollout_base import BatchedRolloutBase

    ro = _compose("Sarnn")(argv=BASE + ["--num_envs", "3", "--world_idx_list", "0", "1", "2", "--env_offset", "4",
                                        "--perturb", "state_noise=0.05", "noise=2"])
    ro.reset()
    ro.rollout_time_idx = 12
    clean = ro.normalize_state(ro.get_raw_state())
    assert clean.dtype == torch.float32 and clean.shape == (3, ro.state_dim) and ro.state_dim > 0
    got = BatchedRolloutBase.get_state(ro)
    ep, dr = _t(np.arange(4, 7, dtype=np.int32)), _t(np.full(3, 12, np.int32))
    z = torch.empty((1, 3, ro.state_dim), dtype=torch.float32, device=DEV)
    K.philox_normal(3, ep, dr, z, plane0=PT.PLANE_STATE)
    want = PT.state_noise(clean.cpu().numpy(), 3, None, None, np.float32(0.05), z[0].cpu().numpy())
    assert got.cpu().numpy().tobytes() == want.tobytes() and not torch.equal(got, clean)
    # another observation of the episode: another noise
    ro.rollout_time_idx = 15
    assert not torch.equal(BatchedRolloutBase.get_state(ro), got)
    # state_noise 0 with the flag on: the unperturbed state
    ro.perturb_spec = parse_spec(["noise=2"])
    ro._perturb_begin()
    assert torch.equal(BatchedRolloutBase.get_state(ro), clean)


# -- 8. rollout level -------------------------------------------------------------------------------
def test_flag_off_launches_nothing_and_keeps_the_fused_path(monkeypatch):
    """Without --perturb the kernel is never called (it is replaced by one that raises), and the tensor
    ACT reads at its first inference is bitwise the direct fused render: the default path is unchanged."""
    from robomanipbaselines_amd import kernels as K

    def refuse(*a, **k):
        raise AssertionError("image_perturb was called without --perturb")

    monkeypatch.setattr(K, "image_perturb", refuse)
    for policy in ("Act", "Sarnn"):
        ro = _compose(policy)(argv=BASE + ["--num_envs", "2", "--world_idx_list", "0", "1"])
        assert ro.perturb_spec is None
        seen, inner = [], ro.get_images

        def spy(*a, **k):
            img = inner(*a, **k)
            mean, std = ro.image_norm
            direct = None
            if policy == "Act":
                direct = torch.empty(img[:, 0].shape, dtype=img.dtype, device=img.device)
                ro.env.render_images("front", policy=direct, mean=mean, std=std)
            seen.append((img.clone(), direct))
            return img

        ro.get_images = spy
        _step_until(ro, seen, 1)
        assert ro._perturb is None
        if policy == "Act":
            img, direct = seen[0]
            assert img.shape[1] == 1 and _bits(img[:, 0].contiguous()).tobytes() == _bits(direct).tobytes()
        assert ro.policy_rgb("front") is ro.info["rgb_images"]["front"]


def test_act_reads_the_perturbed_policy_form():
    """The fused-form path: the tensor ACT's get_images returns at the first two inferences is the
    policy form of the restated perturbation of the clean info["rgb_images"] frame."""
    ro = _compose("Act")(argv=BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--env_offset", "3", "--perturb", *SPEC])
    log, inner = [], ro.get_images

    def spy(*a, **k):
        img = inner(*a, **k)
        clean = ro.info["rgb_images"]["front"]
        # info["rgb_images"] stays clean: it is the frame a plain render of this state gives
        plain = torch.empty_like(clean)
        ro.env.render_images("front", rgb=plain)
        assert torch.equal(clean, plain)
        log.append((int(ro.rollout_time_idx), clean.clone(), img.clone()))
        return img

    ro.get_images = spy
    _step_until(ro, log, 2)
    assert log[0][0] == 0 and log[1][0] == ro.args.skip
    mean, std = ro.image_norm
    H, W = ro.env.renderer.height, ro.env.renderer.width
    for t, clean, img in log[:2]:
        want_u8 = _expected_frame(ro, clean, [3, 4], t)
        assert (want_u8 != clean.cpu().numpy()).mean() > 0.5
        assert img.shape[1] == 1
        got = img[:, 0].contiguous()
        if tuple(got.shape) == (2, H // 2, W // 2, 16):
            form = {torch.bfloat16: 2, torch.float32: 3, torch.uint8: 4}[got.dtype]
        else:
            form = 1 if got.dtype == torch.bfloat16 else 0
        want = PT.policy_form(want_u8, form, mean, std)
        assert _bits(got).tobytes() == want.tobytes(), (t, form)


def test_sarnn_reads_the_perturbed_frame():
    """The policy_rgb path: the frame SARNN's get_images crops at the first two inferences."""
    ro = _compose("Sarnn")(argv=BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--env_offset", "3", "--perturb", *SPEC])
    log = []
    _capture_policy_rgb(ro, log)
    _step_until(ro, log, 2)
    assert log[0][0] == 0 and log[1][0] == ro.args.skip
    for t, clean, frame in log[:2]:
        want = _expected_frame(ro, clean, [3, 4], t)
        assert frame.cpu().numpy().tobytes() == want.tobytes(), t
        assert not torch.equal(frame, clean)
    assert not torch.equal(log[0][2], log[1][2])


def test_shards_read_the_same_perturbed_rows():
    """One lockstep run of 4 envs against two of 2 at --env_offset 0 and 2: the first inference reads
    the same perturbed rows, bit for bit."""
    argv = BASE + ["--world_idx_list", "0", "1", "2", "3", "--perturb", *SPEC]
    whole, wlog = _compose("Sarnn")(argv=argv + ["--num_envs", "4"]), []
    _capture_policy_rgb(whole, wlog)
    _step_until(whole, wlog, 1)
    half = _compose("Sarnn")(argv=argv + ["--num_envs", "2"])
    for off in (0, 2):
        half.args.env_offset = half.env.env_offset = off
        hlog = []
        half.__dict__.pop("policy_rgb", None)
        _capture_policy_rgb(half, hlog)
        _step_until(half, hlog, 1)
        assert hlog[0][0] == wlog[0][0] == 0
        assert torch.equal(hlog[0][1], wlog[0][1][off:off + 2]), f"offset {off}: the clean frames differ"
        assert torch.equal(hlog[0][2], wlog[0][2][off:off + 2]), f"offset {off}: the perturbed rows differ"
    assert not torch.equal(wlog[0][2][0], wlog[0][2][1])


def _hash_frames(frame):
    """i64 [n]: a hash of every row's bytes, on the device."""
    bits = frame.reshape(frame.shape[0], -1).to(torch.int64)
    k = torch.arange(bits.shape[1], dtype=torch.int64, device=bits.device)
    weight = (k * 0x1E3779B97F4A7C15 + 0x632BE59BD9B4E019) | 1  # wraps mod 2^64: fixed odd weights
    return ((bits + 0x1234567) * weight).sum(dim=1)


def test_streamed_episodes_read_the_lockstep_frames():
    """6 episodes streamed through 2 slots, then the same episodes as three lockstep runs at
    --env_offset 0, 2, 4 (same object): per (episode, rollout_time_idx) the policy read the same
    perturbed frame -- the first frame of every episode and every later one both runs made."""
    n, M = 2, 6
    ro = _compose("Sarnn")(argv=BASE + ["--num_envs", str(n), "--num_episodes", str(M), "--max_duration", "0.3",
                                        "--world_idx_list", "0", "1", "2", "--perturb", *SPEC])
    n_pre = len(ro.pre_durations)
    log, inner = [], ro.policy_rgb

    def spy(cam):
        frame = inner(cam)
        if ro.args.num_episodes is not None:
            episode, live = ro.stream.slot_episode.clone(), ro.stream.phase == n_pre
            draw = ro.sched.view(torch.int32)[:, 1].clone()
        else:
            episode = ro.args.env_offset + torch.arange(n, dtype=torch.int32, device=DEV)
            live = torch.ones(n, dtype=torch.bool, device=DEV)
            draw = torch.full((n,), int(ro.rollout_time_idx), dtype=torch.int32, device=DEV)
        log.append((episode, draw, live.clone(), _hash_frames(frame)))
        return frame

    ro.policy_rgb = spy

    def by_key():
        out = {}
        for episode, draw, live, h in log:
            episode, draw, live, h = (t.cpu().numpy() for t in (episode, draw, live, h))
            for r in range(n):
                if live[r]:
                    out[(int(episode[r]), int(draw[r]))] = int(h[r])
        return out

    ro.run()
    assert ro.episode_records["episode"].tolist() == list(range(M)) and len(set(ro.episode_records["slot"].tolist())) > 1
    streamed = by_key()
    assert sorted({e for e, _ in streamed}) == list(range(M)) and all((e, 0) in streamed for e in range(M))
    assert len(set(streamed.values())) == len(streamed)  # every (episode, draw) its own frame
    ro.args.num_episodes = None
    lock = {}
    for off in (0, 2, 4):
        ro.args.env_offset = ro.env.env_offset = off
        log.clear()
        ro.run()
        lock.update(by_key())
    common = sorted(set(streamed) & set(lock))
    assert all((e, 0) in common for e in range(M)) and len(common) >= 2 * M
    differ = [k for k in common if streamed[k] != lock[k]]
    assert not differ, differ[:8]


def test_line_result_and_header_exactly_with_the_flag(tmp_path, capsys):
    import json

    argv = BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--max_duration", "0.1", "--trace_stride", "6"]
    off = _compose("Mlp")(argv=argv + ["--trace_dir", str(tmp_path / "off")])
    off.run()
    assert "Perturb:" not in capsys.readouterr().out and "perturb" not in off.result
    with open(tmp_path / "off" / "header.json") as f:
        assert "perturb" not in json.load(f)
    on = _compose("Mlp")(argv=argv + ["--trace_dir", str(tmp_path / "on"), "--perturb", *SPEC])
    on.run()
    text = capsys.readouterr().out
    line = "[Rollout] Perturb: brightness=20 contrast=0.3 gain=0.2 noise=6 occluder=0.25 state_noise=0.05"
    assert text.count(line) == 1 and text.count("Perturb:") == 1
    want = on.perturb_spec.as_dict()
    assert on.result["perturb"] == want and set(want) == {"brightness", "contrast", "gain", "noise", "occluder", "state_noise"}
    with open(tmp_path / "on" / "header.json") as f:
        assert json.load(f)["perturb"] == want
    assert len(on.result["success"]) == 2


# -- 9. Replay --as_seen ----------------------------------------------------------------------------
def test_replay_as_seen_is_the_frame_the_policy_read(tmp_path):
    from robomanipbaselines_amd.bin import Replay
    from robomanipbaselines_amd.common import episode_trace as ET
    from robomanipbaselines_amd.common.image_io import decode_png

    trace = str(tmp_path / "trace")
    ro = _compose("Sarnn")(argv=BASE + ["--num_envs", "2", "--world_idx_list", "1", "4", "--env_offset", "5", "--max_steps", "100",
                                        "--trace_dir", trace, "--perturb", *SPEC])
    log, inner, steps = [], ro.policy_rgb, [0]
    step_once = ro.step_once

    def counted():
        steps[0] += 1
        step_once()

    def spy(cam):
        frame = inner(cam)
        # called inside step_once number steps[0]: the state is the row of step steps[0] - 1
        log.append((steps[0] - 1, int(ro.rollout_time_idx), ro.info["rgb_images"][cam].cpu().numpy(), frame.cpu().numpy()))
        return frame

    ro.step_once, ro.policy_rgb = counted, spy
    assert ro.run() == 100 and len(log) >= 3
    reader = ET.TraceReader(trace)
    assert reader.header["perturb"] == ro.perturb_spec.as_dict()
    renderer = Replay.make_renderer(reader.header, DEV)
    seen = Replay.as_seen_of(reader.header)
    for step, t, clean, frame in (log[0], log[2]):
        for e in range(2):
            rows = reader.episode(5 + e)
            idx = Replay.select_rows(rows, [str(step)])
            assert int(rows["rollout_time_idx"][idx[0]]) == t
            got = Replay.render_rows(renderer, rows, idx, ["front"], DEV, as_seen=seen)
            assert got[0].tobytes() == frame[e].tobytes(), (step, e)
            plain = Replay.render_rows(renderer, rows, idx, ["front"], DEV)
            assert plain[0].tobytes() == clean[e].tobytes() and plain[0].tobytes() != got[0].tobytes(), (step, e)
    # the command line: one PNG, the frame episode 6 read at its second inference
    step, t, clean, frame = log[1]
    (path,) = Replay.main([trace, "--episode", "6", "--steps", str(step), "--cameras", "front", "--as_seen",
                           "--output_image_dir", str(tmp_path / "png")])
    with open(path, "rb") as f:
        assert decode_png(f.read()).tobytes() == frame[1].tobytes()
    (path,) = Replay.main([trace, "--episode", "6", "--steps", str(step), "--cameras", "front",
                           "--output_image_dir", str(tmp_path / "png0")])
    with open(path, "rb") as f:
        assert decode_png(f.read()).tobytes() == clean[1].tobytes()
    # a trace without the key is refused before anything is drawn
    header = dict(reader.header)
    del header["perturb"]
    with pytest.raises(ValueError, match="perturb"):
        Replay.as_seen_of(header)
