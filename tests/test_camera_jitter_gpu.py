"""The per-episode camera jitter on the device (include/rmbx.h, rmbx_camera_jitter_draw and
rmbx_scene_tables.cam_rows): the draw kernel against the numpy restatement (bitwise); the renderer with
rows bound against an unbound renderer handed the composed camera, env by env (bitwise, every output,
with meshes, shadows, four samples and the static-background cache); known answers of a pinhole and
the brute-force oracle, both built without the restated quaternion product; then --camera_jitter in the
lockstep rollouts, shards, the streaming loop and Replay.

Measured on the MI355X: see BASELINE.md, the --camera_jitter section."""

import ctypes
import json
import math

import numpy as np
import pytest
import torch
import yaml

import camera_jitter_cases as CC
import render_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1234.5  # what rows hold where the kernel must not write
W, H = CC.W, CC.H


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _spec(**over):
    from robomanipbaselines_amd.common.camera_jitter import CameraJitterSpec

    v = dict(CC.STRENGTHS)
    v.update(over)
    return CameraJitterSpec(**{k: CC.f32(x) for k, x in v.items()})


def _kw(spec):
    P, T, F = spec.strengths()
    return dict(pos=float(P), tan_half_rot=float(T), fovy=float(F))


# -- 1. the draw kernel ---------------------------------------------------------------------------------
def _draw(spec, episodes, ncam, active=None, seed=CC.SEED):
    """rows f64 [ncam, n, 8] as the kernel leaves them over a SENTINEL fill, with a guard row past the end."""
    from robomanipbaselines_amd import kernels as K

    n = len(episodes)
    buf = torch.full((ncam * n * 8 + 8,), SENTINEL, dtype=torch.float64, device=DEV)
    rows = buf[:ncam * n * 8].view(ncam, n, 8)
    K.camera_jitter_draw(seed, _t(np.asarray(episodes, np.int32)), rows, active=None if active is None else _t(active),
                         **_kw(spec))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[ncam * n * 8:] == SENTINEL).all()
    return out[:ncam * n * 8].reshape(ncam, n, 8)


@pytest.mark.parametrize("ncam", [1, 3])
@pytest.mark.parametrize("seed", [0, CC.SEED, 2**64 - 1])
def test_draw_is_bitwise_the_restatement(seed, ncam):
    from robomanipbaselines_amd.common import camera_jitter as CJ

    assert len(CC.EPISODES) == 7 and {0, -1, 2**31 - 1} <= set(CC.EPISODES.tolist())
    spec = _spec()
    got = _draw(spec, CC.EPISODES, ncam, seed=seed)
    assert got.tobytes() == CJ.rows(seed, CC.EPISODES, spec, ncam).tobytes()
    # the independent scalar restatement too
    P, T, F = spec.strengths()
    want = np.array([[CC.jitter_row(seed, e, c, P, T, F) for e in CC.EPISODES] for c in range(ncam)])
    assert got.tobytes() == want.tobytes()
    # a row depends on its episode and camera alone: other batch, other position; more rows than one block
    assert _draw(spec, CC.EPISODES[::-1].copy(), ncam, seed=seed).tobytes() == got[:, ::-1].tobytes()
    many = np.arange(-3, 600, dtype=np.int32)
    assert len(many) == 603
    assert _draw(spec, many, ncam, seed=seed).tobytes() == CJ.rows(seed, many, spec, ncam).tobytes()


def test_drawn_rows_keep_their_ranges():
    spec = _spec(pos=0.5, rot=30.0, fovy=0.4999)
    P, T, F = (float(x) for x in spec.strengths())
    got = _draw(spec, np.arange(-3, 600, dtype=np.int32), 3)
    d, q, s = got[..., :3], got[..., 3:7], got[..., 7]
    assert (np.abs(d) < P).all() and np.abs(d).max() > 0.99 * P
    assert (q[..., 0] > 0).all()
    r = q[..., 1:] / q[..., :1]
    assert (np.abs(r) < T).all() and np.abs(r).max() > 0.99 * T
    assert (s > 1 - F).all() and (s < 1 + F).all() and s.min() < 1 - 0.99 * F and s.max() > 1 + 0.99 * F
    # the cameras of one episode differ, in every component
    for c, c2 in ((0, 1), (0, 2), (1, 2)):
        assert (got[c][:, [0, 1, 2, 4, 5, 6, 7]] != got[c2][:, [0, 1, 2, 4, 5, 6, 7]]).all()


def test_drawn_quaternions_are_unit_to_one_ulp():
    """|q| == 1 to 1 ulp (of 1.0: 2^-52) on the rows of the draw cases, the norm measured exactly (a
    rational sum of squares: an f64 norm has roundings of the size it would measure).

    The rule sums |r|^2 before it adds the 1 for this: adding the squares to 1 one by one rounds three
    times at the size of 1 and left 1.22 / 1.25 / 1.32 ulp on the 603-episode batches (about 1 % of the
    rows above 1).  With the one rounding that remains the batches measure 0.90 / 0.88 / 0.93 ulp, the
    7-episode cases 0.69 / 0.85 / 0.66, and 1.8 million rows at rot=3 and rot=30 at most 0.99."""
    from robomanipbaselines_amd.common import camera_jitter as CJ

    spec = _spec()
    worst = {}
    for seed in (0, CC.SEED, 2**64 - 1):
        for name, episodes in (("7 episodes", CC.EPISODES), ("603 episodes", np.arange(-3, 600, dtype=np.int32))):
            got = _draw(spec, episodes, 3, seed=seed)
            assert got.tobytes() == CJ.rows(seed, episodes, spec, 3).tobytes()
            worst[(seed, name)] = CC.norm_deviation_ulps(got[..., 3:7])
    print("\nmax | |q| - 1 | in ulps of 1.0:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_draw_skips_inactive_rows_and_zero_strengths():
    from robomanipbaselines_amd.common import camera_jitter as CJ
    from robomanipbaselines_amd.common.camera_jitter import CameraJitterSpec

    spec = _spec()
    active = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)
    got = _draw(spec, CC.EPISODES, 3, active=active)
    want = CJ.rows(CC.SEED, CC.EPISODES, spec, 3)
    assert got[:, active != 0].tobytes() == want[:, active != 0].tobytes() and (got[:, active == 0] == SENTINEL).all()
    assert (_draw(spec, CC.EPISODES, 3, active=np.zeros(7, np.uint8)) == SENTINEL).all()
    # zero strengths: the identity components exactly, key by key
    assert _draw(CameraJitterSpec(), CC.EPISODES, 2).tobytes() == np.tile(CC.IDENTITY, (2, 7, 1)).tobytes()
    for key, cols in (("pos", [0, 1, 2]), ("rot", [3, 4, 5, 6]), ("fovy", [7])):
        one = _draw(_spec(**{key: 0.0}), CC.EPISODES, 3)
        assert one[..., cols].tobytes() == np.tile(CC.IDENTITY[cols], (3, 7, 1)).tobytes(), key
        assert np.delete(one, cols, -1).tobytes() == np.delete(want, cols, -1).tobytes(), key


def test_draw_argument_errors_launch_nothing():
    from robomanipbaselines_amd import _native as NA
    from robomanipbaselines_amd import kernels as K

    n, ncam = 5, 2
    buf = torch.full((ncam * n * 8 + 8,), SENTINEL, dtype=torch.float64, device=DEV)
    rows = buf[:ncam * n * 8].view(ncam, n, 8)
    ep = torch.arange(n, dtype=torch.int32, device=DEV)
    act = torch.ones(n, dtype=torch.uint8, device=DEV)
    lib = NA.load()
    tmax = float(CC.T_MAX)

    def params(**over):
        v = dict(pos=0.1, tan_half_rot=0.05, fovy=0.1)
        v.update(over)
        return NA.CameraJitterParams(v["pos"], v["tan_half_rot"], v["fovy"])

    ok = dict(episode=ep.data_ptr(), p=params(), rows=rows.data_ptr(), n=n, ncam=ncam)
    inf, nan = float("inf"), float("nan")
    bad = [dict(episode=None), dict(p=None), dict(rows=None), dict(n=0), dict(n=-1), dict(ncam=0), dict(ncam=-2),
           dict(ncam=65), dict(rows=rows.data_ptr() + 4), dict(episode=ep.data_ptr() + 2)]
    above = dict(pos=float(np.nextafter(np.float32(0.5), np.float32(1))), tan_half_rot=float(np.nextafter(CC.T_MAX, np.float32(1))),
                 fovy=0.5)
    for key in ("pos", "tan_half_rot", "fovy"):
        bad += [dict(p=params(**{key: v})) for v in (above[key], 1.5, -0.1, inf, -inf, nan)]
    for over in bad:
        a = dict(ok)
        a.update(over)
        st = lib.rmbx_camera_jitter_draw(ctypes.c_uint64(3), a["episode"], None if a["p"] is None else ctypes.byref(a["p"]),
                                         a["ncam"], a["rows"], act.data_ptr(), a["n"], NA.stream_ptr())
        assert st == -1, {k: v for k, v in over.items() if k != "p"}
        with pytest.raises(ValueError, match="rmbx_camera_jitter_draw"):
            NA.check(st)
    for kw in (dict(seed=-1), dict(seed=2**64), dict(episode=ep.long()), dict(episode=ep[:0]), dict(episode=ep.cpu()),
               dict(episode=ep.view(n, 1)), dict(rows=rows[:, :n - 1].contiguous()), dict(rows=rows.float()),
               dict(rows=rows[..., :7].contiguous()), dict(rows=rows.transpose(0, 1)), dict(rows=rows.cpu()),
               dict(rows=rows[0]), dict(rows=rows[:0]), dict(active=act[:2]), dict(active=act.bool()), dict(active=act.cpu()),
               dict(pos=0.6), dict(fovy=-0.5), dict(tan_half_rot=nan)):
        a = dict(seed=3, episode=ep, rows=rows, pos=0.1, tan_half_rot=0.05, fovy=0.1, active=act)
        a.update(kw)
        with pytest.raises(ValueError):
            K.camera_jitter_draw(**a)
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()
    # the bounds themselves are accepted (pos and rot are closed ranges)
    K.camera_jitter_draw(3, ep, rows, pos=0.5, tan_half_rot=tmax, fovy=0.1, active=act)
    torch.cuda.synchronize()
    assert (rows != SENTINEL).all() and (buf[ncam * n * 8:] == SENTINEL).all()


# -- 2. the renderer with rows bound ---------------------------------------------------------------------
FORMS = {0: torch.float32, 1: torch.bfloat16, 2: torch.bfloat16, 3: torch.float32, 4: torch.uint8}
FILL = 77  # what the outputs hold where the renderer must not write


def _frames(rnd, eng, cam, active=None):
    """Every output of one camera: rgb, depth, hit_geom and the five policy forms (byte views)."""
    n, h, w = eng.n_env, rnd.height, rnd.width
    out = {"rgb": torch.full((n, h, w, 3), FILL, dtype=torch.uint8, device=DEV),
           "depth": torch.full((n, h, w), float(FILL), dtype=torch.float32, device=DEV),
           "hit": torch.full((n, h, w), FILL, dtype=torch.int32, device=DEV)}
    rnd.render(eng, cam, rgb=out["rgb"], depth=out["depth"], hit_geom=out["hit"], active=active)
    for form, dt in FORMS.items():
        shape = (n, 3, h, w) if form < 2 else (n, h // 2, w // 2, 16)
        p = torch.full(shape, FILL, dtype=dt, device=DEV)
        rnd.render(eng, cam, policy=p, active=active)
        out[f"policy{form}"] = p.view(torch.uint8)
    torch.cuda.synchronize()
    return out


def _bind(rnd, cam, rows):
    """Bind `rows` [n, 8] to camera `cam`, identity rows to the scene's other cameras; returns the tensor."""
    c, ncam = rnd.cam_names.index(cam), len(rnd.cam_names)
    full = np.tile(CC.IDENTITY, (ncam, len(rows), 1))
    full[c] = rows
    t = _t(full)
    rnd.bind_camera_rows(t)
    return t


def _assert_each_env_is_its_unbound_camera(arrays, eng, cam, rows, w, h, got, **kw):
    """The property: env e of `got` (rendered with rows bound) is bit for bit env e of an unbound
    renderer on jittered_arrays(arrays, c, rows[e]), in every output."""
    from robomanipbaselines_amd.common import camera_jitter as CJ
    from robomanipbaselines_amd.render import Renderer

    ref = Renderer(arrays, DEV, width=w, height=h, **kw)
    c = ref.cam_names.index(cam)
    nominal = _frames(ref, eng, cam)
    moved = 0
    for e, r in enumerate(rows):
        ref.arrays = CJ.jittered_arrays(arrays, c, r)
        ref.bind_camera_rows(None)  # (drops the static caches: they were built for another camera)
        want = _frames(ref, eng, cam)
        for k in got:
            assert torch.equal(got[k][e], want[k][e]), (cam, e, k)
        if not np.array_equal(np.asarray(r), CC.IDENTITY):
            assert not torch.equal(got["hit"][e], nominal["hit"][e]) or not torch.equal(got["rgb"][e], nominal["rgb"][e]), (cam, e)
            moved += 1
    return moved


def _synthetic_engine(n=7):
    a, gx, gm = CC.synthetic(n)
    return a, RC.SceneEngine(gx, gm, n, DEV)


def _drawn(ncam=1, c=0):
    from robomanipbaselines_amd.common import camera_jitter as CJ

    return CJ.rows(CC.SEED, [5], _spec(pos=0.1, rot=10.0, fovy=0.2), ncam)[c, 0]


@torch.no_grad()
@pytest.mark.parametrize("samples", [1, 4])
def test_synthetic_scene_each_env_is_its_unbound_camera(samples, monkeypatch):
    """A sphere, a box, a cylinder and a textured plane; identity rows among a pure displacement, a pure
    rotation, a pure fovy scale, the spec's extremes and a drawn row; the world camera's static cache in
    use (1 sample) and bypassed (4 samples, and RMBX_RENDER_CACHE=0)."""
    from robomanipbaselines_amd.render import Renderer

    a, eng = _synthetic_engine()
    rows = CC.rows_for_the_renderer(_drawn())
    rnd = Renderer(a, DEV, width=W, height=H, samples=samples)
    _bind(rnd, "cam", rows)
    got = _frames(rnd, eng, "cam")
    assert ("cam" in rnd._caches) == (samples == 1)
    assert _assert_each_env_is_its_unbound_camera(a, eng, "cam", rows, W, H, got, samples=samples) == 5
    # every primitive type is in the nominal frame, and the identity envs see it
    assert set(np.unique(got["hit"][0].cpu().numpy()).tolist()) >= {0, 1, 2, 3}
    if samples == 1:
        monkeypatch.setenv("RMBX_RENDER_CACHE", "0")
        full = Renderer(a, DEV, width=W, height=H)
        _bind(full, "cam", rows)
        uncached = _frames(full, eng, "cam")
        assert "cam" not in full._caches
        for k in got:
            assert torch.equal(got[k], uncached[k]), k


def _cable_engine(n=4):
    from robomanipbaselines_amd import model as MD
    from robomanipbaselines_amd.engine import PhysicsEngine

    arrays = MD.load("ur5e_cable")
    eng = PhysicsEngine(arrays, n, DEV)
    q = np.tile(RC.asset_qpos(arrays), (n // 2, 1))  # even envs at INIT, odd envs displaced by DISPLACED
    eng.qpos.copy_(torch.from_numpy(q))
    eng.forward()
    torch.cuda.synchronize()
    return arrays, eng


def _cable_rows(cam):
    c = list(RC.CAMERAS).index(cam)
    t = float(CC.T_MAX) * 0.999
    return np.stack([CC.row(d=(0.03, -0.02, 0.015), r=(0.02, -0.015, 0.01), s=1.04), _drawn(3, c), CC.IDENTITY,
                     CC.row(d=(0.499, -0.499, 0.499), r=(-t, t, t), s=1.4999)])


@torch.no_grad()
@pytest.mark.parametrize("cam", RC.CAMERAS)
def test_cable_scene_each_env_is_its_unbound_camera(cam):
    """The shipped Cable scene with its meshes at 160 x 120: the world cameras (cached) and the hand
    camera (on the moving wrist: the row acts in that body's frame), env 1 and 3 with the arm displaced."""
    from robomanipbaselines_amd.render import Renderer

    arrays, eng = _cable_engine()
    assert [str(x) for x in arrays["names_cam"]] == list(RC.CAMERAS)
    rows = _cable_rows(cam)
    rnd = Renderer(arrays, DEV, width=160, height=120)
    assert rnd.mesh_tri is not None
    _bind(rnd, cam, rows)
    got = _frames(rnd, eng, cam)
    assert (cam in rnd._caches) == (cam != "hand")
    assert _assert_each_env_is_its_unbound_camera(arrays, eng, cam, rows, 160, 120, got) == 3
    mesh = torch.tensor([int(g) for g in arrays["rmesh_geoms"]], device=DEV)
    assert torch.isin(got["hit"][0], mesh).float().mean() > 0.01  # the jittered env sees the arm's meshes
    # the cached path a second time (nothing dirty): the same frames
    again = _frames(rnd, eng, cam)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@torch.no_grad()
@pytest.mark.parametrize("samples", [1, 4])
def test_cable_scene_with_shadows_each_env_is_its_unbound_camera(samples):
    from robomanipbaselines_amd.render import Renderer

    arrays, eng = _cable_engine(2)
    rows = _cable_rows("front")[:2]
    rnd = Renderer(arrays, DEV, width=160, height=120, shadows=True, samples=samples)
    _bind(rnd, "front", rows)
    got = _frames(rnd, eng, "front")
    assert _assert_each_env_is_its_unbound_camera(arrays, eng, "front", rows, 160, 120, got, shadows=True, samples=samples) == 2
    plain = Renderer(arrays, DEV, width=160, height=120, samples=samples)
    _bind(plain, "front", rows)
    lit = _frames(plain, eng, "front")
    assert not torch.equal(lit["rgb"], got["rgb"]) and torch.equal(lit["hit"], got["hit"])  # the shadows are drawn


@torch.no_grad()
def test_identity_rows_are_no_rows_bound_bit_for_bit():
    from robomanipbaselines_amd.render import Renderer

    a, eng = _synthetic_engine()
    cases = [(a, eng, "cam", W, H, {}), (a, eng, "cam", W, H, dict(samples=4))]
    arrays, ceng = _cable_engine(2)
    cases += [(arrays, ceng, "front", 160, 120, {}), (arrays, ceng, "hand", 160, 120, {}),
              (arrays, ceng, "front", 160, 120, dict(shadows=True))]
    for ar, en, cam, w, h, kw in cases:
        want = _frames(Renderer(ar, DEV, width=w, height=h, **kw), en, cam)
        rnd = Renderer(ar, DEV, width=w, height=h, **kw)
        _bind(rnd, cam, np.tile(CC.IDENTITY, (en.n_env, 1)))
        got = _frames(rnd, en, cam)
        for k in want:
            assert torch.equal(got[k], want[k]), (cam, kw, k)
        # and after unbinding a renderer that had jittered rows bound is the unbound one again
        _bind(rnd, cam, np.tile(CC.row(d=(0.1, 0, 0), s=1.2), (en.n_env, 1)))
        assert not torch.equal(_frames(rnd, en, cam)["rgb"], want["rgb"])
        rnd.bind_camera_rows(None)
        got = _frames(rnd, en, cam)
        for k in want:
            assert torch.equal(got[k], want[k]), (cam, kw, k, "unbound")


@torch.no_grad()
def test_static_cache_follows_the_rows(monkeypatch):
    """The world camera of the synthetic scene (three static primitives).  The same rows twice: the
    second call finds no env dirty and gives the same frame.  One env's row rewritten in the bound
    tensor: that env alone is dirty, and its frame is the full uncached render's; a row rewritten with
    the same values dirties nothing."""
    from robomanipbaselines_amd.common import camera_jitter as CJ
    from robomanipbaselines_amd.render import Renderer

    a, eng = _synthetic_engine()
    rows = CC.rows_for_the_renderer(_drawn())
    rnd = Renderer(a, DEV, width=W, height=H)
    assert int(rnd.static_prims.numel()) == 3
    bound = _bind(rnd, "cam", rows)
    rgb = torch.empty((7, H, W, 3), dtype=torch.uint8, device=DEV)

    def render():
        rnd.render(eng, "cam", rgb=rgb)
        torch.cuda.synchronize()
        return rnd._caches["cam"][4].cpu().numpy().tolist(), rgb.clone()

    dirty, first = render()
    assert dirty == [1] * 7
    dirty, second = render()
    assert dirty == [0] * 7 and torch.equal(first, second)
    new = CC.row(d=(-0.2, 0.1, 0.05), r=(0.05, 0.1, -0.02), s=0.8)
    bound[0, 3].copy_(_t(new))
    dirty, third = render()
    assert dirty == [0, 0, 0, 1, 0, 0, 0]
    want = torch.empty((7, H, W, 3), dtype=torch.uint8, device=DEV)
    Renderer(CJ.jittered_arrays(a, 0, new), DEV, width=W, height=H).render(eng, "cam", rgb=want)
    assert torch.equal(third[3], want[3]) and not torch.equal(third[3], second[3])
    keep = [0, 1, 2, 4, 5, 6]
    assert torch.equal(third[keep], second[keep])
    bound[0, 3].copy_(_t(new.copy()))
    assert render()[0] == [0] * 7
    # the moving sphere alone does not dirty the cache, with rows bound as without
    eng.gxpos[:, 0, 1] += 0.1
    dirty, moved = render()
    assert dirty == [0] * 7 and not torch.equal(moved, third)
    monkeypatch.setenv("RMBX_RENDER_CACHE", "0")  # the call without a cache: rmbx_render_scene's path
    full = Renderer(a, DEV, width=W, height=H)
    full.bind_camera_rows(bound)
    full.render(eng, "cam", rgb=want)
    assert "cam" not in full._caches and torch.equal(moved, want)


@torch.no_grad()
def test_active_mask_leaves_inactive_envs_untouched():
    from robomanipbaselines_amd.render import Renderer

    a, eng = _synthetic_engine()
    rows = CC.rows_for_the_renderer(_drawn())
    active = torch.tensor([1, 0, 1, 1, 0, 1, 0], dtype=torch.uint8, device=DEV)
    on = active.bool()
    for kw in ({}, dict(samples=4)):
        rnd = Renderer(a, DEV, width=W, height=H, **kw)
        _bind(rnd, "cam", rows)
        want = _frames(rnd, eng, "cam")
        rnd2 = Renderer(a, DEV, width=W, height=H, **kw)
        _bind(rnd2, "cam", rows)
        got = _frames(rnd2, eng, "cam", active=active)
        for k in want:
            assert torch.equal(got[k][on], want[k][on]), (kw, k)
            off = got[k][~on]
            if k == "depth":
                assert (off == float(FILL)).all(), (kw, k)
            elif k in ("rgb", "hit"):
                assert (off == FILL).all(), (kw, k)
            else:  # a policy form's bytes: those of its FILL-filled tensor
                form = int(k[-1])
                ref = torch.full((1,), FILL, dtype=FORMS[form], device=DEV).view(torch.uint8)
                assert torch.equal(off.reshape(-1, ref.numel()), ref.expand(off.numel() // ref.numel(), -1)), (kw, k)


def test_bind_camera_rows_checks_its_arguments():
    from robomanipbaselines_amd.render import Renderer

    a, eng = _synthetic_engine()
    rnd = Renderer(a, DEV, width=W, height=H)
    good = _t(np.tile(CC.IDENTITY, (1, 7, 1)))
    for bad in (good.float(), good.cpu(), good[0], good.repeat(2, 1, 1), good[..., :7].contiguous(), good.transpose(0, 1),
                np.tile(CC.IDENTITY, (1, 7, 1)), good[:, :0]):
        with pytest.raises(ValueError):
            rnd.bind_camera_rows(bad)
    rnd.bind_camera_rows(good[:, :5].contiguous())
    with pytest.raises(ValueError, match="5 envs"):
        rnd.render(eng, "cam", rgb=torch.empty((7, H, W, 3), dtype=torch.uint8, device=DEV))
    rnd.bind_camera_rows(None)  # unbinding, also what was never bound, is fine
    rnd.bind_camera_rows(None)


# -- 3. independent of the restated composition ------------------------------------------------------------
def _centroid(mask):
    ys, xs = np.nonzero(mask)
    return np.array([xs.mean() + 0.5, ys.mean() + 0.5]), len(xs)


@torch.no_grad()
def test_pinhole_known_answers():
    """One small sphere at a known point in front of a world camera that is offset and rolled by 90
    degrees (so the mount's frame is not the camera's).  The centroid of its hit_geom mask, against
    the pinhole f = (H / 2) / tan(fovy / 2): a displacement d along the camera's x and y moves it by
    -d f / z pixels (image y pointing down: +d_y f / z); a fovy scale scales its offset from the image
    centre by tan(fovy / 2) / tan(fovy' / 2); a rotation about the camera's y puts it at the projection
    of the counter-rotated point.  Each within half a pixel, the discretisation of a mask of about 100
    pixels."""
    from robomanipbaselines_amd.render import Renderer

    c = math.sqrt(0.5)
    cam_pos, cam_quat, fovy = np.array([0.3, -0.2, 0.5]), (c, 0.0, 0.0, c), 45.0
    Rc = CC.quat2mat(cam_quat)  # camera axes in the world: x -> world y, y -> world -x
    assert np.allclose(Rc @ [1, 0, 0], [0, 1, 0]) and np.allclose(Rc @ [0, 1, 0], [-1, 0, 0])
    P = np.array([0.25, 0.12, -2.0])  # the sphere's centre in the camera frame
    z = -P[2]
    f = (H / 2) / math.tan(math.radians(fovy) / 2)
    a, pos, gm = RC.scene([(2, (0.13, 0, 0), tuple(cam_pos + Rc @ P), (1, 0, 0))], cam_pos=tuple(cam_pos), cam_quat=cam_quat,
                          fovy=fovy)
    d_cam = np.array([0.15, -0.1, 0.0])
    th = math.radians(6.0)
    s = 1.3
    rows = np.stack([CC.IDENTITY, CC.row(d=Rc @ d_cam), CC.row(s=s), CC.row(r=(0, math.tan(th / 2), 0))])
    eng = RC.SceneEngine(pos, gm, 4, DEV)
    rnd = Renderer(a, DEV, width=W, height=H)
    _bind(rnd, "cam", rows)
    hit = torch.empty((4, H, W), dtype=torch.int32, device=DEV)
    rnd.render(eng, "cam", hit_geom=hit)
    hit = hit.cpu().numpy()
    cen, area = zip(*(_centroid(hit[e] == 0) for e in range(4)))
    print(f"\ncentroids {[c.round(3).tolist() for c in cen]} areas {area}; f = {f:.3f} px, z = {z}")
    assert 80 <= area[0] <= 130
    centre = np.array([W / 2, H / 2])
    assert np.abs(cen[0] - CC.project(P, fovy)).max() < 0.5
    # displacement: -d f / z in x, +d f / z in the image's downward y
    shift = cen[1] - cen[0]
    assert abs(shift[0] - (-d_cam[0] * f / z)) < 0.5 and abs(shift[1] - (d_cam[1] * f / z)) < 0.5, shift
    assert np.abs(shift).min() > 3
    # fovy: the offset from the image centre scales by tan(fovy / 2) / tan(fovy' / 2)
    k = math.tan(math.radians(fovy) / 2) / math.tan(math.radians(fovy * s) / 2)
    assert np.abs((cen[2] - centre) - k * (cen[0] - centre)).max() < 0.5 and k < 0.8
    assert abs(area[2] / area[0] - k * k) < 0.1
    # rotation about the camera's y by th: the point counter-rotated into the turned camera's frame
    Pr = CC.rodrigues((0, 1, 0), th).T @ P
    assert np.abs(cen[3] - CC.project(Pr, fovy)).max() < 0.5
    assert abs((cen[3] - cen[0])[0]) > 5  # turning left moves the image right by about f tan(th)


@torch.no_grad()
def test_a_jittered_env_against_the_brute_force_oracle():
    """Env ORACLE_ENV of the synthetic scene with ORACLE_ROW bound, every pixel, against
    oracle/render_oracle.c handed a camera composed from rotation matrices
    (camera_jitter_cases.camera_by_matrices): zero unexplained pixels at render_cases' tolerances, the
    excused share under its cap (tests/test_camera_jitter.py holds the oracle alone under it)."""
    from oracle import render as OR
    from robomanipbaselines_amd.render import Renderer

    a, eng = _synthetic_engine()
    e = CC.ORACLE_ENV
    rows = np.tile(CC.IDENTITY, (7, 1))
    rows[e] = CC.ORACLE_ROW
    rnd = Renderer(a, DEV, width=W, height=H)
    _bind(rnd, "cam", rows)
    f = _frames(rnd, eng, "cam")
    hit, depth, rgb = (f[k][e].cpu().numpy() for k in ("hit", "depth", "rgb"))
    aj = CC.camera_by_matrices(a, 0, CC.ORACLE_ROW)
    xs, ys = RC.all_pixels(W, H)
    res = RC.compare_frame(aj, OR.scene_prims(aj), eng.pose(e), "cam", W, H, xs, ys, hit, depth, rgb)
    print(f"\njittered env vs the oracle: {len(xs)} pixels, differing {res.differing}, ambiguous {res.ambiguous}, "
          f"unexplained {len(res.unexplained)}")
    assert len(res.unexplained) == 0, res.detail
    assert res.ambiguous < RC.AMBIGUOUS_CAP * len(xs)
    # and against the nominal camera the same frame is wrong: the comparison can see the jitter
    nominal = RC.compare_frame(a, OR.scene_prims(a), eng.pose(e), "cam", W, H, xs, ys, hit, depth, rgb)
    assert len(nominal.unexplained) > 0.02 * len(xs)


# -- 4. rollouts -----------------------------------------------------------------------------------------------
from test_actuation_gpu import BASE, _compose, _rows_now  # noqa: E402
from test_perturb_gpu import _hash_frames  # noqa: E402

ON = ["pos=0.02", "rot=3", "fovy=0.05"]


def _spy(ro, log, checked=None):
    """Log, per policy inference, (episode, r, live, a hash of the frame each row read, the action each
    row got).  checked (a list): at every row's first inference its frame must be the one an unbound
    Renderer draws of the same state with the camera composed from rows(seed, episode) on the host; the
    episode is appended."""
    check_rows = checked is not None
    from robomanipbaselines_amd.common import camera_jitter as CJ
    from robomanipbaselines_amd.render import Renderer

    inner_rgb, inner_infer, seen = ro.policy_rgb, ro.infer_policy, {}
    ref = [None]

    def rgb(cam):
        frame = inner_rgb(cam)
        if cam == "front":
            seen["frame"] = frame
        return frame

    def infer():
        seen.pop("frame", None)
        inner_infer()
        episode, r, live = _rows_now(ro)
        frame = seen["frame"]
        log.append((episode, r, live, _hash_frames(frame).cpu().numpy(), ro.policy_action.cpu().numpy().copy()))
        if check_rows:
            rnd = ro.env.renderer
            if ref[0] is None:
                ref[0] = Renderer(ro.env.arrays, DEV, width=rnd.width, height=rnd.height)
            c = rnd.cam_names.index("front")
            want = torch.empty_like(frame)
            for i in range(ro.n):
                if live[i] and int(r[i]) == 0:
                    row = CJ.rows(int(ro.args.seed), [int(episode[i])], ro.camera_jitter_spec, len(rnd.cam_names))[c, 0]
                    assert ro._camera_jitter.rows[c, i].cpu().numpy().tobytes() == row.tobytes(), (i, int(episode[i]))
                    ref[0].arrays = CJ.jittered_arrays(ro.env.arrays, c, row)
                    ref[0].bind_camera_rows(None)
                    ref[0].render(ro.env.engine, "front", rgb=want)
                    assert torch.equal(frame[i], want[i]), (i, int(episode[i]))
                    checked.append(int(episode[i]))

    ro.policy_rgb, ro.infer_policy = rgb, infer


def _by_key(log):
    out = {}
    for entry in log:
        episode, r, live, h, action = entry[:5]
        for i in range(len(episode)):
            if live[i]:
                out[(int(episode[i]), int(r[i]))] = (int(h[i]), action[i].tobytes())
    return out


def test_slots_shards_and_the_streaming_loop_see_the_same_episodes():
    """Episodes 0..3 with --camera_jitter: streamed through 2 slots (episodes 2 and 3 in recycled slots),
    in lockstep with 4 envs, and as two lockstep shards of 2 at --env_offset 0 and 2.  Per (episode,
    rollout_time_idx) the policy read the same frame and made the same action, bit for bit; every
    episode's first frame, a recycled slot's included, is the unbound render of the camera composed
    from rows(seed, episode)."""
    tail = ["--world_idx_list", "0", "1", "2", "--max_duration", "0.3", "--camera_jitter", *ON]
    st = _compose("Sarnn")(argv=BASE + ["--num_envs", "2", "--num_episodes", "4", *tail])
    slog, schecked = [], []
    _spy(st, slog, checked=schecked)
    st.run()
    assert st.episode_records["episode"].tolist() == [0, 1, 2, 3] and len(set(st.episode_records["slot"].tolist())) == 2
    assert sorted(schecked) == [0, 1, 2, 3]  # every episode's first frame was checked, the recycled slots' too
    streamed = _by_key(slog)
    lk = _compose("Sarnn")(argv=BASE + ["--num_envs", "4", *tail])
    llog, lchecked = [], []
    _spy(lk, llog, checked=lchecked)
    lk.run()
    assert sorted(lchecked) == [0, 1, 2, 3]
    lock4 = _by_key(llog)
    half = _compose("Sarnn")(argv=BASE + ["--num_envs", "2", *tail])
    hlog = []
    _spy(half, hlog)
    lock2 = {}
    for off in (0, 2):
        half.args.env_offset = half.env.env_offset = off
        hlog.clear()
        half.run()
        lock2.update(_by_key(hlog))
    assert all((e, 0) in d for e in range(4) for d in (streamed, lock4, lock2))
    assert len({v[0] for k, v in lock4.items() if k[1] == 0}) == 4  # four episodes, four different first frames
    for name, other in (("4 lockstep envs vs 2-env shards", lock2), ("4 lockstep envs vs 2 streaming slots", streamed)):
        common = sorted(set(lock4) & set(other))
        assert len(common) >= 8, (name, len(common))
        frames = [k for k in common if lock4[k][0] != other[k][0]]
        actions = [k for k in common if lock4[k][1] != other[k][1]]
        print(f"\n{name}: {len(common)} common (episode, step) keys, differing frames {frames[:6]}, actions {actions[:6]}")
        assert not frames and not actions, name


def test_line_result_yaml_and_header_exactly_with_the_flag(tmp_path, capsys):
    argv = BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--max_duration", "0.1", "--trace_stride", "6"]
    off = _compose("Mlp")(argv=argv + ["--trace_dir", str(tmp_path / "off"), "--result_filename", str(tmp_path / "off.yaml")])
    off.run()
    assert "Camera jitter:" not in capsys.readouterr().out and "camera_jitter" not in off.result
    with open(tmp_path / "off" / "header.json") as f:
        assert "camera_jitter" not in json.load(f)
    with open(tmp_path / "off.yaml") as f:
        assert "camera_jitter" not in yaml.safe_load(f)
    on = _compose("Mlp")(argv=argv + ["--trace_dir", str(tmp_path / "on"), "--result_filename", str(tmp_path / "on.yaml"),
                                      "--camera_jitter", *ON])
    on.run()
    text = capsys.readouterr().out
    assert text.count("[Rollout] Camera jitter: pos=0.02 rot=3 fovy=0.05") == 1 and text.count("Camera jitter:") == 1
    want = on.camera_jitter_spec.as_dict()
    assert list(want) == ["pos", "rot", "fovy"] and want == {"pos": CC.f32(0.02), "rot": 3.0, "fovy": CC.f32(0.05)}
    assert on.result["camera_jitter"] == want and "dynamics" not in on.result and "perturb" not in on.result
    with open(tmp_path / "on" / "header.json") as f:
        assert json.load(f)["camera_jitter"] == want
    with open(tmp_path / "on.yaml") as f:
        assert yaml.safe_load(f)["camera_jitter"] == want
    assert len(on.result["success"]) == 2
    with pytest.raises(ValueError, match="--camera_jitter"):
        _compose("Mlp")(argv=argv + ["--camera_jitter", "rot=45"])
    # the point cloud's intrinsics stay the nominal ones
    assert on.env.get_camera_fovy("front") == float(on.env.arrays["cam_fovy"][0])


def test_flag_off_is_the_unbound_renderer(monkeypatch):
    """Without --camera_jitter neither the draw wrapper nor bind_camera_rows is called (both are replaced
    by ones that raise), nothing is bound, and the frames the policy reads are bitwise those of a fresh
    Renderer that never had rows bound."""
    from robomanipbaselines_amd import kernels as K
    from robomanipbaselines_amd.render import Renderer

    def refuse(*a, **k):
        raise AssertionError("camera_jitter_draw was called without --camera_jitter")

    def refuse_bind(*a, **k):
        raise AssertionError("bind_camera_rows was called without --camera_jitter")

    monkeypatch.setattr(K, "camera_jitter_draw", refuse)
    argv = BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--max_duration", "0.2"]
    with monkeypatch.context() as m:
        m.setattr(Renderer, "bind_camera_rows", refuse_bind)
        for extra in ([], ["--num_episodes", "3"]):
            ro = _compose("Sarnn")(argv=argv + extra)
            assert ro.camera_jitter_spec is None
            rnd = ro.env.renderer
            fresh = Renderer(ro.env.arrays, DEV, width=rnd.width, height=rnd.height)
            inner, frames = ro.policy_rgb, []

            def spy(cam, inner=inner, ro=ro, fresh=fresh, frames=frames):
                frame = inner(cam)
                want = torch.empty_like(frame)
                fresh.render(ro.env.engine, cam, rgb=want)
                assert torch.equal(frame, want)
                frames.append(cam)
                return frame

            ro.policy_rgb = spy
            ro.run()
            assert len(frames) >= 2 and ro._camera_jitter is None and rnd._cam_rows is None and rnd._scene.cam_rows is None
            assert "camera_jitter" not in ro.result
    on = _compose("Sarnn")(argv=argv + ["--camera_jitter", "rot=1"])
    with pytest.raises(AssertionError, match="camera_jitter_draw was called"):
        on.run()


def test_replay_draws_the_recorded_episodes_rows(tmp_path):
    """A run recorded with --camera_jitter and --perturb: Replay of a recorded step is bitwise the clean
    jittered frame of the live step, with --as_seen the frame the policy read; a header without the key
    replays the nominal cameras, as before."""
    import types

    from robomanipbaselines_amd.bin import Replay
    from robomanipbaselines_amd.common import episode_trace as ET
    from robomanipbaselines_amd.common.image_io import decode_png
    from robomanipbaselines_amd.render import Renderer

    trace = str(tmp_path / "trace")
    ro = _compose("Sarnn")(argv=BASE + ["--num_envs", "2", "--world_idx_list", "1", "4", "--env_offset", "5", "--max_steps", "100",
                                        "--trace_dir", trace, "--camera_jitter", *ON, "--perturb", "brightness=20", "noise=4"])
    log, inner, steps = [], ro.policy_rgb, [0]
    step_once = ro.step_once

    def counted():
        steps[0] += 1
        step_once()

    def spy(cam):
        frame = inner(cam)
        log.append((steps[0] - 1, int(ro.rollout_time_idx), ro.info["rgb_images"][cam].cpu().numpy(), frame.cpu().numpy()))
        return frame

    ro.step_once, ro.policy_rgb = counted, spy
    assert ro.run() == 100 and len(log) >= 3
    reader = ET.TraceReader(trace)
    assert reader.header["camera_jitter"] == ro.camera_jitter_spec.as_dict()
    renderer = Replay.make_renderer(reader.header, DEV)
    seen, jit = Replay.as_seen_of(reader.header), Replay.camera_jitter_of(reader.header)
    bare = dict(reader.header)
    del bare["camera_jitter"]
    assert jit is not None and Replay.camera_jitter_of(bare) is None
    plain_renderer = Renderer(ro.env.arrays, DEV, width=renderer.width, height=renderer.height)
    for step, t, clean, frame in (log[0], log[2]):
        for e in range(2):
            rows = reader.episode(5 + e)
            idx = Replay.select_rows(rows, [str(step)])
            assert int(rows["rollout_time_idx"][idx[0]]) == t
            got = Replay.render_rows(renderer, rows, idx, ["front"], DEV, camera_jitter=jit)
            assert got[0].tobytes() == clean[e].tobytes(), (step, e)
            got = Replay.render_rows(renderer, rows, idx, ["front"], DEV, as_seen=seen, camera_jitter=jit)
            assert got[0].tobytes() == frame[e].tobytes() and frame[e].tobytes() != clean[e].tobytes(), (step, e)
            # without the key: the nominal cameras, what a renderer that never had rows bound draws of the row
            nominal = Replay.render_rows(renderer, rows, idx, ["front"], DEV, camera_jitter=Replay.camera_jitter_of(bare))
            dev = {k: _t(rows[k][idx]) for k in ("gxpos", "gxmat", "xpos", "xquat")}
            eng = types.SimpleNamespace(n_env=1, ngeom=rows["gxpos"].shape[1], nbody=rows["xpos"].shape[1], **dev)
            want = torch.empty((1, renderer.height, renderer.width, 3), dtype=torch.uint8, device=DEV)
            plain_renderer.render(eng, "front", rgb=want)
            assert nominal[0].tobytes() == want[0].cpu().numpy().tobytes() and nominal[0].tobytes() != clean[e].tobytes()
    # the command line: one PNG per call, episode 6's second inference, clean and as seen
    step, t, clean, frame = log[1]
    (path,) = Replay.main([trace, "--episode", "6", "--steps", str(step), "--cameras", "front", "--device", DEV,
                           "--output_image_dir", str(tmp_path / "png0")])
    with open(path, "rb") as f:
        assert decode_png(f.read()).tobytes() == clean[1].tobytes()
    (path,) = Replay.main([trace, "--episode", "6", "--steps", str(step), "--cameras", "front", "--as_seen", "--device", DEV,
                           "--output_image_dir", str(tmp_path / "png")])
    with open(path, "rb") as f:
        assert decode_png(f.read()).tobytes() == frame[1].tobytes()
