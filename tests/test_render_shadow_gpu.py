"""The renderer's hard shadows (Renderer(shadows=True): render_kernel<*, 0, true> of
csrc/rmbx_render.hip) held to the composed oracle of tests/shadow_cases.py on every pixel, with
render_cases.compare_frame's rule: geom, depth and 8-bit colour of every pixel, zero unexplained
pixels, at most 2 % excused where the oracle itself is ambiguous under the jitter.  The shadow changes
3.4 % / 5.2 % of Cable front's pixels (test_render_shadow_oracle.py), so a renderer without it fails.

Synthetic scenes reach what the shipped ones do not: every occluder type, a mesh as receiver and as
its own occluder, an occluder outside the view frustum, MAX_PRIM primitives across tile borders.
Everything else is bitwise: shadows off for a scene whose light casts none, the static-background
cache (a shadowed render bypasses it), the active mask, tile groups, the policy forms, the order of
the envs in the batch.

Measured on an MI355X (differing / ambiguous / unexplained pixels per env; pixels the shadow changes
against the same Renderer's shadows-off frame): Cable front 0/0/0 and 0/0/0 of 7,488 (252, 402),
side 0/0/0 twice (110, 135), hand at 52 x 36 0/0/0 twice of 1,872 (635, 521), Ring front 1/1/0 twice
(314, 492), Pick front 0/0/0 twice (298, 463); every synthetic case 0/0/0 but the 128 primitives'
1/1/0 of 6,144.  About 2 s per shipped-scene case (the oracle on the CPU), the file 15 s."""

import functools

import numpy as np
import pytest
import torch

import render_cases as RC
import shadow_cases as SC

gpu = pytest.mark.gpu
DEV = "cuda:0"
W, H = 104, 72
PLANE = (0, (0, 0, 0.1), (0, 0, 0), (0.8, 0.7, 0.6))


def _buffers(n, h, w):
    return (torch.full((n, h, w, 3), 9, dtype=torch.uint8, device=DEV),
            torch.full((n, h, w), -5.0, dtype=torch.float32, device=DEV),
            torch.full((n, h, w), -7, dtype=torch.int32, device=DEV))


def _frame(rnd, eng, cam, **kw):
    out = _buffers(eng.n_env, rnd.height, rnd.width)  # (sentinels: an unwritten pixel shows)
    rnd.render(eng, cam, rgb=out[0], depth=out[1], hit_geom=out[2], **kw)
    torch.cuda.synchronize()
    return out


def _np(frame):
    return tuple(t.cpu().numpy() for t in frame)


def _changed(on, off):
    """Pixels whose colour the shadow changes by more than RGB_TOL, per env."""
    return (np.abs(on.astype(int) - off.astype(int)).max(-1) > RC.RGB_TOL).reshape(len(on), -1).sum(1)


def _cube(c, s):
    """A cube's 12 triangles, wound outwards (one-sided triangles: seen from outside, and its
    underside faces the shadow rays from below)."""
    v = np.array([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)]) + np.asarray(c, np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([[v[q[0]], v[q[i]], v[q[i + 1]]] for q in quads for i in (1, 2)])


def _synthetic(objects, w, h, tris=None, n_env=1, edit=None, **kw):
    """Render a synthetic scene from the oblique camera with shadows on and off: (arrays, engine,
    frame with shadows, frame without)."""
    from robomanipbaselines_amd.render import Renderer

    a, pos, gm = RC.scene(objects, cam_pos=SC.CAM_POS, cam_quat=SC.CAM_QUAT, tris=tris, **kw)
    if edit is not None:
        edit(a, pos, gm)
    eng = RC.SceneEngine(pos, gm, n_env, DEV)
    on = _frame(Renderer(a, DEV, width=w, height=h, shadows=True), eng, "cam")
    off = _frame(Renderer(a, DEV, width=w, height=h), eng, "cam")
    assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])  # depth and hit_geom never change
    return a, eng, _np(on), _np(off)


# ---- synthetic occluders, every pixel -------------------------------------------------------------
def _rot_x(a, pos, gm):
    gm[1] = RC.rot((1, 0.3, 0), 70)  # the occluder tilted: its shadow is not its upright outline


OCCLUDERS = {
    "sphere": dict(objects=[PLANE, (2, (0.15, 0, 0), (0.1, 0.1, 0.4), (0.9, 0.2, 0.2))]),
    "capsule": dict(objects=[PLANE, (3, (0.06, 0.2, 0), (-0.1, 0.0, 0.4), (0.2, 0.9, 0.2))], edit=_rot_x),
    "cylinder": dict(objects=[PLANE, (5, (0.1, 0.15, 0), (0.0, 0.2, 0.45), (0.2, 0.2, 0.9))], edit=_rot_x),
    "box": dict(objects=[PLANE, (6, (0.2, 0.1, 0.05), (0.1, -0.1, 0.35), (0.9, 0.9, 0.2))], edit=_rot_x),
    "mesh": dict(objects=[PLANE], tris=_cube((0.05, 0.1, 0.4), 0.12)),
}


@gpu
@torch.no_grad()
@pytest.mark.parametrize("kind", sorted(OCCLUDERS))
def test_each_occluder_type_casts_onto_a_plane(kind):
    w, h = 64, 48
    a, eng, on, off = _synthetic(w=w, h=h, **OCCLUDERS[kind])
    res = SC.check(kind, a, [eng.pose(0)], "cam", w, h, on)
    plane = on[2][0] == 0
    dark = (np.abs(on[0][0].astype(int) - off[0][0].astype(int)).max(-1) > RC.RGB_TOL)
    print(f"{kind}: shadow-changed pixels {int(dark.sum())}, on the plane {int((dark & plane).sum())}")
    assert (dark & plane).sum() > 30 and res[0].occluded.sum() > 30


@gpu
@torch.no_grad()
def test_missing_mesh_bounding_box_casts():
    """A mesh geom whose file is missing is drawn, and casts, as its bounding box."""
    w, h = 64, 48

    def edit(a, pos, gm):
        a["geom_csize"][1] = (0.15, 0.1, 0.05)

    a, eng, on, off = _synthetic([PLANE, (7, (0, 0, 0), (0.0, 0.1, 0.4), (0.3, 0.8, 0.8))], w, h, edit=edit)
    assert (on[2][0] == 1).sum() > 40  # the box is drawn
    SC.check("missing mesh box", a, [eng.pose(0)], "cam", w, h, on)
    assert _changed(on[0], off[0])[0] > 30


@gpu
@torch.no_grad()
def test_mesh_receiver_under_a_primitive_and_a_mesh_shadowing_itself():
    w, h = 64, 48
    # a cube mesh whose top a sphere shadows; beside it two stacked triangles of the same mesh: the
    # lower faces up (seen), the upper faces down (culled for the camera above, but it faces the
    # shadow rays from below: it casts)
    lower = [[-0.7, -0.2, 0.2], [-0.2, -0.2, 0.2], [-0.45, 0.4, 0.2]]
    upper = [[-0.55, -0.1, 0.5], [-0.45, 0.2, 0.5], [-0.35, -0.1, 0.5]]
    tris = np.concatenate([_cube((0.3, 0.1, 0.2), 0.2), np.array([lower, upper])])
    a, eng, on, off = _synthetic([PLANE, (2, (0.12, 0, 0), (0.3, 0.1, 0.7), (0.9, 0.2, 0.2))], w, h, tris=tris)
    SC.check("mesh receiver", a, [eng.pose(0)], "cam", w, h, on)
    mesh = on[2][0] == 2
    dark = np.abs(on[0][0].astype(int) - off[0][0].astype(int)).max(-1) > RC.RGB_TOL
    xs = np.arange(w)[None, :].repeat(h, 0)
    left, right = dark & mesh & (xs < w // 2 - 4), dark & mesh & (xs >= w // 2)
    print(f"mesh pixels {int(mesh.sum())}, shadowed on the cube's top {int(right.sum())}, on the lower triangle {int(left.sum())}")
    assert right.sum() >= 8 and left.sum() >= 8


@gpu
@torch.no_grad()
def test_occluder_outside_the_view_frustum():
    """A sphere 3 m up, above and behind the camera's view (over 90 degrees off its axis), shadows the ground at
    the image centre: the query must test the block's primitives, not the tile's culled list."""
    w, h = 64, 48
    a, eng, on, off = _synthetic([PLANE, (2, (0.3, 0, 0), (0.0, 0.0, 3.0), (0.9, 0.2, 0.2))], w, h)
    assert (on[2][0] == 0).all()  # the sphere is not in the frame
    SC.check("occluder outside the frustum", a, [eng.pose(0)], "cam", w, h, on)
    assert _changed(on[0], off[0])[0] > 100
    assert np.abs(on[0][0, h // 2, w // 2].astype(int) - off[0][0, h // 2, w // 2].astype(int)).max() > RC.RGB_TOL


@gpu
@torch.no_grad()
def test_128_primitives_shadow_across_tile_borders():
    w, h = 96, 64
    objs = [PLANE]
    for k in range(127):  # MAX_PRIM in all: a grid of small spheres over the ground the frame shows
        i, j = k % 13, k // 13
        objs.append((2, (0.03 + 0.004 * (k % 4), 0, 0), (-0.9 + 0.15 * i, -0.6 + 0.17 * j, 0.15 + 0.02 * (k % 5)),
                     (0.2 + 0.06 * (k % 13), 0.9 - 0.08 * (k // 13), 0.5)))
    a, eng, on, off = _synthetic(objs, w, h)
    SC.check("128 primitives", a, [eng.pose(0)], "cam", w, h, on)
    dark = np.abs(on[0][0].astype(int) - off[0][0].astype(int)).max(-1) > RC.RGB_TOL
    tiles = {(int(y) // 16, int(x) // 16) for y, x in np.argwhere(dark)}
    print(f"128 primitives: shadow-changed pixels {int(dark.sum())} in {len(tiles)} of 24 tiles")
    assert dark.sum() > 200 and len(tiles) >= 12


@gpu
@torch.no_grad()
def test_a_convex_primitive_does_not_shadow_itself():
    """The lit top of a sphere and of a box keep the light (the ray from 1 mm above the surface
    leaves its own primitive), the ground under them loses it."""
    w, h = 64, 48
    a, eng, on, off = _synthetic([PLANE, (2, (0.2, 0, 0), (-0.3, 0.1, 0.2), (0.9, 0.2, 0.2)),
                                  (6, (0.15, 0.15, 0.1), (0.3, 0.1, 0.1), (0.2, 0.9, 0.2))], w, h)
    SC.check("self shadow", a, [eng.pose(0)], "cam", w, h, on)
    for g in (1, 2):
        px = on[2][0] == g
        assert px.sum() > 50 and np.array_equal(on[0][0][px], off[0][0][px]), g
    assert _changed(on[0], off[0])[0] > 20


# ---- the shipped scenes -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _asset(name):
    arrays, eng = RC.asset_engine(name, DEV)
    return arrays, eng, [RC.engine_pose(eng, e) for e in range(eng.n_env)]


@gpu
@torch.no_grad()
@pytest.mark.parametrize("name,cam,w,h", [("ur5e_cable", "front", W, H), ("ur5e_cable", "side", W, H),
                                          ("ur5e_cable", "hand", W // 2, H // 2), ("ur5e_ring", "front", W, H),
                                          ("ur5e_pick", "front", W, H)])
def test_every_pixel_of_the_shadowed_scenes(name, cam, w, h):
    from robomanipbaselines_amd.render import Renderer, scene_casts_shadows

    arrays, eng, poses = _asset(name)
    assert scene_casts_shadows(arrays)
    rnd = Renderer(arrays, DEV, width=w, height=h, shadows=True)
    on = _frame(rnd, eng, cam)
    assert bool((rnd._vis == -1).all()) and bool((rnd._tflag == 0).all())  # the workspaces are empty again
    off = _frame(Renderer(arrays, DEV, width=w, height=h), eng, cam)
    assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    changed = _changed(_np(on)[0], _np(off)[0])
    print(f"{name} {cam} {w}x{h}: pixels the shadow changes vs the same Renderer's shadows-off frame {changed.tolist()}")
    SC.check(f"{name} {cam}", arrays, poses, cam, w, h, _np(on))
    if (name, cam) == ("ur5e_cable", "front"):
        assert (changed >= 200).all(), changed  # the case cannot pass vacuously


@gpu
@torch.no_grad()
def test_scene_whose_light_casts_no_shadow_is_bitwise_the_plain_render():
    """`--shadows scene` follows the compiled light_castshadow: Insert's light has castshadow="false"."""
    from robomanipbaselines_amd.render import Renderer, scene_casts_shadows

    arrays, eng, _ = _asset("ur5e_insert")
    assert not scene_casts_shadows(arrays)
    rnd = Renderer(arrays, DEV, width=W, height=H, shadows=scene_casts_shadows(arrays))
    for x, y in zip(_frame(rnd, eng, "front"), _frame(Renderer(arrays, DEV, width=W, height=H), eng, "front")):
        assert torch.equal(x, y)


@gpu
@torch.no_grad()
def test_other_light_directions_are_refused():
    from robomanipbaselines_amd import _native as N
    from robomanipbaselines_amd.render import Renderer

    arrays, eng, _ = _asset("ur5e_cable")
    b = dict(arrays)
    b["light_dir"] = np.array([[0.0, 0.6, -0.8]])
    with pytest.raises(ValueError, match="shadows"):
        Renderer(b, DEV, width=W, height=H, shadows=True)
    Renderer(b, DEV, width=W, height=H)  # without shadows the light arrays are not consulted
    rnd = Renderer(arrays, DEV, width=W, height=H, shadows=True)
    rnd._scene.light_dir[1] = 0.5  # the C ABI refuses it too, before any launch
    rgb, depth, hit = _buffers(2, H, W)
    with pytest.raises(ValueError, match="light_dir"):
        rnd.render(eng, "front", rgb=rgb, depth=depth, hit_geom=hit)
    torch.cuda.synchronize()
    assert bool((rgb == 9).all()) and bool((hit == -7).all()) and N is not None


# ---- the static-background cache ---------------------------------------------------------------------
def _everything(rnd, eng, cam):
    n, h, w = eng.n_env, rnd.height, rnd.width
    out = _frame(rnd, eng, cam)
    s2d = torch.full((n, h // 2, w // 2, 16), 77, dtype=torch.uint8, device=DEV)
    rnd.render(eng, cam, policy=s2d)
    torch.cuda.synchronize()
    return out + (s2d,)


@gpu
@torch.no_grad()
def test_shadowed_render_through_the_cache_equals_the_uncached_one(monkeypatch):
    """Welded receivers (the ground, a box) and a moving box over them, a world camera: with the cache
    enabled and disabled the shadowed frames are bitwise equal, on the first frame (where an unshadowed
    render rebuilds its cache) and after the box moved (where it would reuse it) -- and the moving
    box's shadow moves with it over the welded receivers."""
    from robomanipbaselines_amd.render import Renderer

    w, h = 96, 64
    objs = [PLANE, (6, (0.3, 0.2, 0.05), (0.2, 0.2, 0.05), (0.2, 0.9, 0.2)), (6, (0.1, 0.1, 0.03), (0.0, 0.0, 0.5), (0.9, 0.2, 0.2))]
    a, pos, gm = RC.scene(objs, cam_pos=SC.CAM_POS, cam_quat=SC.CAM_QUAT, welded=[1, 1, 0])
    pos2 = np.stack([pos, pos])
    pos2[1, 2] += (0.1, 0.05, 0.1)
    eng = RC.SceneEngine(pos2, gm, 2, DEV)
    monkeypatch.setenv("RMBX_RENDER_CACHE", "1")
    cached = Renderer(a, DEV, width=w, height=h, shadows=True)
    assert cached.prim_static.tolist() == [1, 1, 0]
    plain = Renderer(a, DEV, width=w, height=h)
    frames = []
    for step in range(3):
        monkeypatch.setenv("RMBX_RENDER_CACHE", "1")
        got = _everything(cached, eng, "cam")
        off = _everything(plain, eng, "cam")  # (the unshadowed render does use its cache)
        assert "cam" in plain._caches and "cam" not in cached._caches
        monkeypatch.setenv("RMBX_RENDER_CACHE", "0")
        want = _everything(Renderer(a, DEV, width=w, height=h, shadows=True), eng, "cam")
        for name, x, y in zip(("rgb", "depth", "hit", "s2d"), got, want):
            assert torch.equal(x, y), (step, name, int((x != y).sum()))
        assert (_changed(_np(got)[0], _np(off)[0]) > 15).all()
        if step == 0:
            SC.check("welded receivers", a, [eng.pose(0), eng.pose(1)], "cam", w, h, _np(got)[:3])
        frames.append(got[0].clone())
        eng.gxpos[:, 2, 0] += 0.15  # the moving box moves; the welded receivers stay
    assert not torch.equal(frames[0], frames[1]) and not torch.equal(frames[1], frames[2])


@gpu
@torch.no_grad()
def test_cable_front_across_a_pose_change_with_and_without_the_cache(monkeypatch):
    from robomanipbaselines_amd import model as MD
    from robomanipbaselines_amd.engine import PhysicsEngine
    from robomanipbaselines_amd.render import Renderer

    arrays = MD.load("ur5e_cable")
    eng = PhysicsEngine(arrays, 2, DEV)
    q = torch.from_numpy(RC.asset_qpos(arrays)).to(DEV)
    monkeypatch.setenv("RMBX_RENDER_CACHE", "1")
    cached = Renderer(arrays, DEV, width=W, height=H, shadows=True)
    last = None
    for step in range(2):
        eng.qpos.copy_(q)
        eng.forward()
        monkeypatch.setenv("RMBX_RENDER_CACHE", "1")
        got = _everything(cached, eng, "front")
        monkeypatch.setenv("RMBX_RENDER_CACHE", "0")
        want = _everything(Renderer(arrays, DEV, width=W, height=H, shadows=True), eng, "front")
        for name, x, y in zip(("rgb", "depth", "hit", "s2d"), got, want):
            assert torch.equal(x, y), (step, name, int((x != y).sum()))
        assert last is None or not torch.equal(last, got[0])
        last = got[0].clone()
        q[:, :6] += torch.tensor([0.3, 0.2, -0.25, 0.4, -0.3, 0.5], dtype=torch.float64, device=DEV)


# ---- active mask, tile groups, policy forms, batch order ---------------------------------------------
def _cable3():
    from robomanipbaselines_amd import model as MD
    from robomanipbaselines_amd.engine import PhysicsEngine

    arrays = MD.load("ur5e_cable")
    eng = PhysicsEngine(arrays, 3, DEV)
    q = np.tile(np.asarray(arrays["qpos0"], np.float64), (3, 1))
    q[:, :6] = RC.INIT
    q[1, :6] += RC.DISPLACED
    q[2, :6] -= 0.5 * np.asarray(RC.DISPLACED)
    eng.qpos.copy_(torch.from_numpy(q))
    eng.forward()
    torch.cuda.synchronize()
    return arrays, eng, q


@gpu
@torch.no_grad()
@pytest.mark.parametrize("cam", ["front", "hand"])
def test_active_mask_groups_forms_and_batch_order(cam, monkeypatch):
    from robomanipbaselines_amd.engine import PhysicsEngine
    from robomanipbaselines_amd.render import IMAGENET_MEAN, IMAGENET_STD, Renderer

    arrays, eng, q = _cable3()
    n = 3
    rnd = Renderer(arrays, DEV, width=W, height=H, shadows=True)
    monkeypatch.delenv("RMBX_RENDER_GROUPS", raising=False)
    want = _frame(rnd, eng, cam)
    again = _frame(rnd, eng, cam)  # two renders of the same state
    for x, y in zip(want, again):
        assert torch.equal(x, y)
    assert (_changed(_np(want)[0], _np(_frame(Renderer(arrays, DEV, width=W, height=H), eng, cam))[0]) > 50).all()
    # the active mask: env 1 keeps its sentinels, the others are the unmasked frames; workspaces empty
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV)
    got = _frame(rnd, eng, cam, active=active)
    for g, w_, s in zip(got, want, (9, -5.0, -7)):
        assert bool((g[1] == s).all()) and torch.equal(g[0], w_[0]) and torch.equal(g[2], w_[2])
    assert bool((rnd._vis == -1).all()) and bool((rnd._tflag == 0).all())
    # tile groups
    for g in ("1", "7", "35"):
        monkeypatch.setenv("RMBX_RENDER_GROUPS", g)
        for name, x, y in zip(("rgb", "depth", "hit"), _frame(rnd, eng, cam), want):
            assert torch.equal(x, y), (g, name)
    monkeypatch.delenv("RMBX_RENDER_GROUPS", raising=False)
    # the policy forms carry the shadow: each is the u8 frame's pixels, as the unshadowed forms are
    u8 = want[0]
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=DEV)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=DEV)
    norm = (u8.float() / 255.0 - mean) / std  # [n, H, W, 3], the kernel's f32 expression
    chw = torch.empty((n, 3, H, W), dtype=torch.float32, device=DEV)
    chw16 = torch.empty((n, 3, H, W), dtype=torch.bfloat16, device=DEV)
    s2d8 = torch.empty((n, H // 2, W // 2, 16), dtype=torch.uint8, device=DEV)
    s2d32 = torch.empty((n, H // 2, W // 2, 16), dtype=torch.float32, device=DEV)
    s2d16 = torch.empty((n, H // 2, W // 2, 16), dtype=torch.bfloat16, device=DEV)
    for p in (chw, chw16, s2d8, s2d32, s2d16):
        rnd.render(eng, cam, policy=p)
    torch.cuda.synchronize()
    torch.testing.assert_close(chw, norm.permute(0, 3, 1, 2), rtol=0, atol=1e-6)
    assert torch.equal(chw16, chw.to(torch.bfloat16))

    def s2d(x):  # [n, H, W, 3] -> [n, H/2, W/2, 16], channel (dy * 2 + dx) * 3 + c, 12..15 zero
        x = x.reshape(n, H // 2, 2, W // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, H // 2, W // 2, 12)
        return torch.cat([x, torch.zeros_like(x[..., :4])], -1)

    assert torch.equal(s2d8, s2d(u8))
    assert torch.equal(s2d32, s2d(chw.permute(0, 2, 3, 1).contiguous()))
    assert torch.equal(s2d16, s2d32.to(torch.bfloat16))
    # batch order: the same states in another env order give the same frames, permuted
    perm = [2, 0, 1]
    eng2 = PhysicsEngine(arrays, 3, DEV)
    eng2.qpos.copy_(torch.from_numpy(q[perm]))
    eng2.forward()
    torch.cuda.synchronize()
    for name, x, y in zip(("rgb", "depth", "hit"), _frame(rnd, eng2, cam), want):
        assert torch.equal(x, y[perm]), name
