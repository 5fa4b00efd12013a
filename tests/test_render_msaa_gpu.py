"""The renderer's 4-samples-per-pixel mode (Renderer(samples=4): four raster_kernel<true> +
render_kernel<*, 0, *, true> passes and resolve_kernel of csrc/rmbx_render.hip) held to the frame
tests/msaa_cases.py composes from the unchanged oracle: every compared pixel within RGB_TOL of
(s0 + s1 + s2 + s3 + 2) // 4 of the oracle's four 8-bit samples, zero unexplained pixels, at most 5 %
excused where one of the samples is ambiguous under the jitter.  The mode moves 6-10 % of a frame's
pixels by more than RGB_TOL (test_render_msaa_oracle.py), so a renderer without it fails.

Known answers on synthetic scenes pin the sample pattern (a red box around one sample position, its
mirror image, a strip only the centre ray sees, edges at a quarter, a half and three quarters of a
pixel, a mesh triangle's edge, a shadow edge); everything else is bitwise: samples=1 against the
default, depth and hit_geom against the single-sample render, the cache, the tile groups, the active
mask, the policy forms.

Measured on an MI355X (differing / excused / unexplained pixels per env; pixels the mode moves by more
than RGB_TOL against the same Renderer's single-sample frame): Cable front 0/0/0 twice of 7,488 (628,
734 moved), Insert front 0/0/0 twice (533, 675), Cable hand 0/0/0 twice of 1,872 (540, 504 of the whole
frame), Pick hand 0/0/0 twice (481, 368), Cable front with shadows 0/0/0 twice (693, 830); every
known answer equal to the composed value to the level.  The oracle on the CPU is the time: 2.5-4 s per
scene case, 7 s with shadows (four composed shadow casts per pixel), the file 24 s."""

import functools
import glob
import os

import numpy as np
import pytest
import torch

import msaa_cases as MC
import render_cases as RC
import shadow_cases as SC
from oracle import render as OR

gpu = pytest.mark.gpu
DEV = "cuda:0"
W, H = 104, 72
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BLUE, RED = (0.1, 0.2, 0.9), (0.9, 0.15, 0.1)
T45 = float(np.tan(np.deg2rad(22.5)))


def _buffers(n, h, w):
    return (torch.full((n, h, w, 3), 9, dtype=torch.uint8, device=DEV),
            torch.full((n, h, w), -5.0, dtype=torch.float32, device=DEV),
            torch.full((n, h, w), -7, dtype=torch.int32, device=DEV))


def _frame(rnd, eng, cam, **kw):
    out = _buffers(eng.n_env, rnd.height, rnd.width)  # (sentinels: an unwritten pixel shows)
    rnd.render(eng, cam, rgb=out[0], depth=out[1], hit_geom=out[2], **kw)
    torch.cuda.synchronize()
    return out


def _empty(rnd):
    return bool((rnd._vis == -1).all()) and bool((rnd._tflag == 0).all())


@functools.lru_cache(maxsize=None)
def _asset(name):
    arrays, eng = RC.asset_engine(name, DEV)
    return arrays, eng, [RC.engine_pose(eng, e) for e in range(eng.n_env)]


# ---- 1. every pixel of real scenes -------------------------------------------------------------------
@gpu
@torch.no_grad()
@pytest.mark.parametrize("name,cam,subset,shadows", [("ur5e_cable", "front", False, False),
                                                     ("ur5e_insert", "front", False, False),
                                                     ("ur5e_cable", "hand", True, False),
                                                     ("ur5e_pick", "hand", True, False),
                                                     ("ur5e_cable", "front", False, True)])
def test_every_pixel_of_the_4_sample_scenes(name, cam, subset, shadows):
    from robomanipbaselines_amd.render import Renderer

    arrays, eng, poses = _asset(name)
    rnd = Renderer(arrays, DEV, width=W, height=H, samples=4, shadows=shadows)
    got = _frame(rnd, eng, cam)
    assert _empty(rnd)
    one = _frame(Renderer(arrays, DEV, width=W, height=H, shadows=shadows), eng, cam)
    assert torch.equal(got[1], one[1]) and torch.equal(got[2], one[2])  # depth and hit_geom: the centre ray's
    moved = (np.abs(got[0].cpu().numpy().astype(int) - one[0].cpu().numpy().astype(int)).max(-1) > RC.RGB_TOL)
    print(f"{name} {cam}: pixels the 4 samples move vs the same Renderer's single-sample frame "
          f"{moved.reshape(2, -1).sum(1).tolist()} of {W * H}")
    xs, ys = MC.every_fourth(W, H) if subset else RC.all_pixels(W, H)
    MC.check(f"{name} {cam}{' shadows' if shadows else ''}", arrays, poses, cam, W, H, xs, ys, got[0].cpu().numpy(),
             shadows=shadows)
    if cam == "front":  # the case cannot pass vacuously: more pixels move than may be excused
        assert (moved.reshape(2, -1).sum(1) > MC.EXCUSED_CAP * W * H).all()


# ---- 3. known answers that pin the pattern -----------------------------------------------------------
def _box(x0, x1, y0, y1, zf=1.0, hz=1e-3, rgb=RED):
    """A thin box whose front face, at camera depth zf, covers the pixel-coordinate rectangle
    [x0, x1] x [y0, y1] of the W x H frame of a fovy-45 camera at the origin looking along -z."""
    X = [(2 * x / W - 1) * T45 * W / H * zf for x in (x0, x1)]
    Y = [(1 - 2 * y / H) * T45 * zf for y in (y0, y1)]
    return (6, ((X[1] - X[0]) / 2, (Y[0] - Y[1]) / 2, hz), ((X[0] + X[1]) / 2, (Y[0] + Y[1]) / 2, -(zf + hz)), rgb)


PLANE_BEHIND = (0, (0, 0, 0.1), (0, 0, -2.0), BLUE)


def _known(objects, tris=None, shadows=False, cam_pos=(0.0, 0.0, 0.0), cam_quat=(1.0, 0.0, 0.0, 0.0)):
    """Render a synthetic scene with samples=4 and samples=1: (arrays, pose, prims, 4-sample frame,
    single-sample frame) as numpy."""
    from robomanipbaselines_amd.render import Renderer

    a, pos, gm = RC.scene(objects, tris=tris, cam_pos=cam_pos, cam_quat=cam_quat)
    eng = RC.SceneEngine(pos, gm, 1, DEV)
    four = _frame(Renderer(a, DEV, width=W, height=H, samples=4, shadows=shadows), eng, "cam")
    one = _frame(Renderer(a, DEV, width=W, height=H, shadows=shadows), eng, "cam")
    assert torch.equal(four[1], one[1]) and torch.equal(four[2], one[2])
    return a, eng.pose(0), OR.scene_prims(a), [t[0].cpu().numpy() for t in four], [t[0].cpu().numpy() for t in one]


def _pixel(a, prims, pose, px, py, shadows=False):
    return MC.cast4(a, prims, pose, "cam", W, H, np.array([px]), np.array([py]), shadows)


def _close(got, want):
    return np.abs(np.asarray(got).astype(int) - np.asarray(want).astype(int)).max() <= RC.RGB_TOL


PIXELS = ((37, 29), (101, 67), (16, 47), (63, 0))  # inside a tile, in the ragged corner tile, on tile borders


@gpu
@torch.no_grad()
@pytest.mark.parametrize("k", range(4))
def test_a_box_around_one_sample_position(k):
    """The box covers +-0.1 pixel around sample k of one pixel: exactly that sample sees it, the pixel
    is (A + 3 B + 2) // 4; around the mirrored position (1 - sx, sy) no sample sees it."""
    px, py = PIXELS[k]
    sx, sy = MC.PATTERN[k]
    a, pose, prims, four, one = _known([PLANE_BEHIND, _box(px + sx - 0.1, px + sx + 0.1, py + sy - 0.1, py + sy + 0.1)])
    s = _pixel(a, prims, pose, px, py)
    assert s.geom[0].tolist() == [1 if j == k else 0 for j in range(4)]
    A, B = s.s8[0, k], s.s8[0, (k + 1) % 4]
    want = (A + 3 * B + 2) // 4
    # (the three plane samples differ by a level at most; one wrong sample is worth >= 20 levels)
    assert np.abs(want - s.resolved[0]).max() <= 1 and np.abs(want - B).max() >= 20
    print(f"sample {k} pixel {(px, py)}: box {A.tolist()} plane {B.tolist()} expected {want.tolist()} gpu {four[0][py, px].tolist()}")
    assert _close(four[0][py, px], want)
    assert _close(one[0][py, px], B) and one[2][py, px] == 0  # the centre ray misses it
    for (qx, qy) in ((px - 1, py), (px + 1, py), (px, py - 1), (px, py + 1)):
        if 0 <= qx < W and 0 <= qy < H:
            assert _close(four[0][qy, qx], B), (qx, qy)
    # mirrored
    mx = 1.0 - sx
    a, pose, prims, four, one = _known([PLANE_BEHIND, _box(px + mx - 0.1, px + mx + 0.1, py + sy - 0.1, py + sy + 0.1)])
    s = _pixel(a, prims, pose, px, py)
    assert s.geom[0].tolist() == [0, 0, 0, 0]
    assert _close(four[0][py, px], s.resolved[0]) and _close(four[0][py, px], B)
    assert four[2][py, px] == 0 and four[1][py, px] == one[1][py, px]  # what the centre ray sees: the plane


@gpu
@torch.no_grad()
def test_a_strip_only_the_centre_ray_sees():
    px, py = 37, 29
    a, pose, prims, four, one = _known([PLANE_BEHIND, _box(px + 0.45, px + 0.55, py - 3, py + 4)])
    s = _pixel(a, prims, pose, px, py)
    assert s.geom[0].tolist() == [0, 0, 0, 0]
    cg, cd, _ = OR.cast(a, prims, pose.gxpos, pose.gxmat, pose.xpos, pose.xquat, "cam", W, H, np.array([[px + 0.5, py + 0.5]]))
    assert cg[0] == 1
    # hit_geom and depth are the centre ray's (the box), bitwise the single-sample render's (_known)
    assert four[2][py, px] == 1 and abs(four[1][py, px] - cd[0]) <= RC.DEPTH_RTOL * cd[0] + RC.DEPTH_ATOL
    assert four[1][py, px] < 1.01
    # the colour is the plane's: no sample sees the box (the single-sample pixel is the box's red)
    assert _close(four[0][py, px], s.resolved[0]) and _close(four[0][py, px], four[0][py, px - 1])
    assert not _close(one[0][py, px], four[0][py, px])


@gpu
@torch.no_grad()
@pytest.mark.parametrize("vertical", [True, False])
@pytest.mark.parametrize("frac,covered", [(0.25, 3), (0.5, 2), (0.75, 1)])
def test_a_box_edge_through_a_pixel(vertical, frac, covered):
    """A box edge at pixel fraction 0.25 / 0.5 / 0.75 covers 3 / 2 / 1 samples, vertical or horizontal."""
    px, py = (101, 30) if vertical else (40, 67)
    box = _box(px + frac, px + frac + 9, py - 7, py + 8) if vertical else _box(px - 7, px + 8, py + frac, py + frac + 9)
    a, pose, prims, four, one = _known([PLANE_BEHIND, box])
    s = _pixel(a, prims, pose, px, py)
    axis = 0 if vertical else 1
    assert s.geom[0].tolist() == [1 if MC.PATTERN[j][axis] > frac else 0 for j in range(4)]
    assert int(s.geom[0].sum()) == covered
    print(f"{'vertical' if vertical else 'horizontal'} edge at {frac}: expected {s.resolved[0].tolist()} gpu {four[0][py, px].tolist()}")
    assert _close(four[0][py, px], s.resolved[0])
    # the neighbours across the edge are all plane / all box
    lo, hi = ((px - 1, py), (px + 1, py)) if vertical else ((px, py - 1), (px, py + 1))
    plane8, box8 = four[0][lo[1], lo[0]].astype(int), four[0][hi[1], hi[0]].astype(int)
    assert np.abs(plane8 - box8).max() >= 80
    assert _close(four[0][py, px], ((4 - covered) * plane8 + covered * box8 + 2) // 4)


@gpu
@torch.no_grad()
def test_a_mesh_triangle_edge_through_a_pixel():
    """The raster path: a triangle's edge at half a pixel covers the two samples right of it."""
    px, py = 37, 29
    xe = (2 * (px + 0.5) / W - 1) * T45 * W / H
    tri = np.array([[[xe, -0.3, -1.0], [xe + 0.3, 0.0, -1.0], [xe, 0.3, -1.0]]])  # wound towards the camera
    a, pose, prims, four, one = _known([PLANE_BEHIND], tris=tri)
    s = _pixel(a, prims, pose, px, py)
    assert s.geom[0].tolist() == [1 if MC.PATTERN[j][0] > 0.5 else 0 for j in range(4)]
    print(f"mesh edge: expected {s.resolved[0].tolist()} gpu {four[0][py, px].tolist()}")
    assert _close(four[0][py, px], s.resolved[0])
    plane8, tri8 = four[0][py, px - 1].astype(int), four[0][py, px + 1].astype(int)
    assert four[2][py, px - 1] == 0 and four[2][py, px + 1] == 1 and np.abs(plane8 - tri8).max() >= 40
    assert _close(four[0][py, px], (2 * plane8 + 2 * tri8 + 2) // 4)


@gpu
@torch.no_grad()
def test_a_shadow_edge_through_a_pixel():
    """The oblique camera over the ground; a box's shadow edge, parallel to the image rows, at half of
    pixel row 50: the two upper samples are shadowed, the two lower ones lit."""
    px, py = 52, 50
    sy = (1 - 2 * (py + 0.5) / H) * T45
    t = 0.9 / (0.6 - 0.8 * sy)
    ye = -1.2 + t * (0.6 * sy + 0.8)  # where the rays of image row py + 0.5 meet the ground
    ground = (0, (0, 0, 0.1), (0, 0, 0), (0.8, 0.7, 0.6))
    box = (6, (0.6, 0.15, 0.01), (0.0, ye + 0.15, 0.5), RED)
    a, pose, prims, four, one = _known([ground, box], shadows=True, cam_pos=SC.CAM_POS, cam_quat=SC.CAM_QUAT)
    s = _pixel(a, prims, pose, px, py, shadows=True)
    assert s.geom[0].tolist() == [0, 0, 0, 0]
    assert s.occluded[0].tolist() == [MC.PATTERN[j][1] < 0.5 for j in range(4)]
    lit, dark = s.s8[0, 3], s.s8[0, 0]
    assert np.abs(lit - dark).max() >= 20
    print(f"shadow edge: lit {lit.tolist()} shadowed {dark.tolist()} expected {s.resolved[0].tolist()} gpu {four[0][py, px].tolist()}")
    assert _close(four[0][py, px], s.resolved[0])
    assert _close(four[0][py - 1, px], dark) and _close(four[0][py + 1, px], lit)
    xs, ys = RC.all_pixels(W, H)
    band = (np.abs(xs - px) < 12) & (np.abs(ys - 44) < 12)  # the shadow's near and far edges (rows 37 and 50)
    MC.check("shadow edge", a, [pose], "cam", W, H, xs[band], ys[band], four[0][None], shadows=True)


# ---- 4. invariants, bitwise ----------------------------------------------------------------------------
def _everything(rnd, eng, cam):
    n, h, w = eng.n_env, rnd.height, rnd.width
    out = _frame(rnd, eng, cam)
    s2d = torch.full((n, h // 2, w // 2, 16), 77, dtype=torch.uint8, device=DEV)
    rnd.render(eng, cam, policy=s2d)
    torch.cuda.synchronize()
    return out + (s2d,)


@gpu
@torch.no_grad()
@pytest.mark.parametrize("cam", ["front", "hand"])
def test_samples_1_is_the_default_renderer(cam):
    from robomanipbaselines_amd.render import Renderer

    arrays, eng, _ = _asset("ur5e_cable")
    for x, y in zip(_everything(Renderer(arrays, DEV, width=W, height=H, samples=1), eng, cam),
                    _everything(Renderer(arrays, DEV, width=W, height=H), eng, cam)):
        assert torch.equal(x, y)
    four = _everything(Renderer(arrays, DEV, width=W, height=H, samples=4), eng, cam)
    one = _everything(Renderer(arrays, DEV, width=W, height=H), eng, cam)
    assert torch.equal(four[1], one[1]) and torch.equal(four[2], one[2])
    assert not torch.equal(four[0], one[0]) and not torch.equal(four[3], one[3])


@gpu
@torch.no_grad()
def test_unsupported_sample_counts_are_refused_before_any_launch():
    from robomanipbaselines_amd.render import Renderer

    arrays, eng, _ = _asset("ur5e_cable")
    with pytest.raises(ValueError, match="samples"):
        Renderer(arrays, DEV, width=W, height=H, samples=3)
    rnd = Renderer(arrays, DEV, width=W, height=H, samples=4)
    rnd._scene.samples = 2  # the C ABI refuses it too
    rgb, depth, hit = _buffers(2, H, W)
    with pytest.raises(ValueError, match="samples"):
        rnd.render(eng, "front", rgb=rgb, depth=depth, hit_geom=hit)
    torch.cuda.synchronize()
    assert bool((rgb == 9).all()) and bool((depth == -5.0).all()) and bool((hit == -7).all()) and _empty(rnd)


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
    cached = Renderer(arrays, DEV, width=W, height=H, samples=4)
    plain = Renderer(arrays, DEV, width=W, height=H)
    last = None
    for step in range(2):
        eng.qpos.copy_(q)
        eng.forward()
        monkeypatch.setenv("RMBX_RENDER_CACHE", "1")
        got = _everything(cached, eng, "front")
        one = _everything(plain, eng, "front")  # (the single-sample render does use its cache)
        assert "front" in plain._caches and "front" not in cached._caches
        monkeypatch.setenv("RMBX_RENDER_CACHE", "0")
        want = _everything(Renderer(arrays, DEV, width=W, height=H, samples=4), eng, "front")
        for name, x, y in zip(("rgb", "depth", "hit", "s2d"), got, want):
            assert torch.equal(x, y), (step, name, int((x != y).sum()))
        assert torch.equal(got[1], one[1]) and torch.equal(got[2], one[2])
        assert last is None or not torch.equal(last[1], got[0][1])
        last = got[0].clone()
        q[1, :6] += torch.tensor([0.3, 0.2, -0.25, 0.4, -0.3, 0.5], dtype=torch.float64, device=DEV)  # env 1 moves


@gpu
@torch.no_grad()
@pytest.mark.parametrize("cam", ["front", "hand"])
def test_tile_groups_active_mask_and_policy_forms(cam, monkeypatch):
    from robomanipbaselines_amd import kernels as K
    from robomanipbaselines_amd.render import Renderer

    arrays, eng, _ = _asset("ur5e_cable")
    rnd = Renderer(arrays, DEV, width=W, height=H, samples=4)
    monkeypatch.delenv("RMBX_RENDER_GROUPS", raising=False)
    want = _frame(rnd, eng, cam)
    for x, y in zip(want, _frame(rnd, eng, cam)):  # two renders of the same state
        assert torch.equal(x, y)
    # tile groups do not change the frame
    for g in ("1", "7", "35"):
        monkeypatch.setenv("RMBX_RENDER_GROUPS", g)
        for name, x, y in zip(("rgb", "depth", "hit"), _frame(rnd, eng, cam), want):
            assert torch.equal(x, y), (g, name)
    monkeypatch.delenv("RMBX_RENDER_GROUPS", raising=False)
    # an inactive env keeps its outputs (the sentinels) and its words of the workspaces; vis / tflag empty
    rnd._samp.fill_(0x3c3c3c3c)
    before = rnd._samp.clone()
    active = torch.tensor([1, 0], dtype=torch.uint8, device=DEV)
    got = _frame(rnd, eng, cam, active=active)
    for g_, w_, s in zip(got, want, (9, -5.0, -7)):
        assert bool((g_[1] == s).all()) and torch.equal(g_[0], w_[0])
    s2d = torch.full((2, H // 2, W // 2, 16), 77, dtype=torch.uint8, device=DEV)
    rnd.render(eng, cam, policy=s2d, active=active)
    torch.cuda.synchronize()
    assert bool((s2d[1] == 77).all()) and not bool((s2d[0] == 77).all())
    assert torch.equal(rnd._samp[W * H:], before[W * H:]) and not torch.equal(rnd._samp[:W * H], before[:W * H])
    assert _empty(rnd)
    # the five policy forms agree with each other and with the resolved rgb
    rgb = want[0]
    forms = {}
    for key, shape, dt in (("chw32", (2, 3, H, W), torch.float32), ("chw16", (2, 3, H, W), torch.bfloat16),
                           ("s2d32", (2, H // 2, W // 2, 16), torch.float32),
                           ("s2d16", (2, H // 2, W // 2, 16), torch.bfloat16),
                           ("s2d8", (2, H // 2, W // 2, 16), torch.uint8)):
        forms[key] = torch.full(shape, 3, dtype=dt, device=DEV)  # (a sentinel: every element must be written)
        rnd.render(eng, cam, policy=forms[key], mean=MEAN, std=STD)
    torch.cuda.synchronize()
    assert torch.equal(K.image_to_s2d(forms["chw32"]), forms["s2d32"])
    assert torch.equal(K.image_to_s2d(forms["chw16"]), forms["s2d16"])
    assert torch.equal(K.image_to_s2d(rgb.permute(0, 3, 1, 2)), forms["s2d8"])
    ref = rgb.permute(0, 3, 1, 2).double() / 255.0
    ref = (ref - torch.tensor(MEAN, dtype=torch.float64, device=DEV).view(1, 3, 1, 1)) \
        / torch.tensor(STD, dtype=torch.float64, device=DEV).view(1, 3, 1, 1)
    torch.testing.assert_close(forms["chw32"].double(), ref, rtol=0, atol=1e-6)
    assert torch.equal(forms["chw16"], forms["chw32"].to(torch.bfloat16))  # bf16 is the f32 value rounded once


# ---- 5. plumbing ---------------------------------------------------------------------------------------
@gpu
def test_rollout_command_line_with_offsamples(tmp_path):
    from robomanipbaselines_amd.bin.Rollout import main
    from robomanipbaselines_amd.common.image_io import decode_png

    imgs = {}
    for v in ("4", "1", "scene"):
        d = os.path.join(tmp_path, "img" + v)
        ro = main(["Mlp", "MujocoUR5eCable", "--auto_exit", "--no_plot", "--no_render", "--save_last_image",
                   "--output_image_dir", d, "--num_envs", "2", "--world_idx_list", "0", "3", "--max_steps", "4",
                   "--offsamples", v])
        assert ro.env.renderer.samples == (1 if v == "1" else 4) and ro.env.offsamples == ro.env.renderer.samples
        pngs = sorted(glob.glob(os.path.join(d, "*.png")))
        assert len(pngs) == 2
        with open(pngs[0], "rb") as f:
            imgs[v] = decode_png(f.read()).astype(int)
    differ = int((np.abs(imgs["4"] - imgs["1"]).max(-1) > 0).sum())
    print(f"--offsamples 4 vs 1: the saved frame differs on {differ} pixels")
    assert differ > 50
    assert np.array_equal(imgs["scene"], imgs["4"])  # the scene's value is MuJoCo's default 4
