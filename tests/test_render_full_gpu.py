"""The batched renderer (csrc/rmbx_render.hip) held to the brute-force oracle (oracle/render_oracle.c)
on every pixel, every shipped scene and every primitive type, and to the closed-form answers of
tests/test_render_oracle.py on synthetic scenes that reach the code no shipped scene does.

What the suite did not see before (census of the shipped assets, made on the CPU with the oracle at
the poses used here): test_render_gpu.py samples every 10th pixel from 5, so only odd rows and
columns, of the Cable scene alone; no shipped scene draws a sphere (primitive types over the seven
assets: plane 1 each, box 10-25, capsule 25 / 11 in Cable / Ring, cylinder 2 / 4 / 3 in Cable /
Door / Ring, sphere 0); every camera of every scene sees 0.0 % background (the floor plane fills
the frame), so the skybox, hit_geom -1 and the background depth were never produced; every scene
has meshes (22 mesh bodies and 83,838 triangles, Pick 28 and 143,296) and materials, so
render_kernel<false, *>, the flat-material path and rmbx_render never ran; Door's geom 77 is the
only box with a "2d" texture (603 / 290 / 0 pixels of the front / side / hand frame); no test
passed `active` or set RMBX_RENDER_GROUPS.

The comparison is render_cases.compare_frame: hit geom, depth (rtol 1e-4, atol 1e-5) and 8-bit
colour (+-2) of every pixel against the oracle's ray through its centre; a differing pixel is
excused only where the oracle is ambiguous (a coincident second surface, or a spread under a jitter
of 0.02 x H / 480 pixel), at most 2 % of the pixels, none unexplained.  Because the depth-spread
rule also excuses the steep limb of a round primitive (1.5-1.8 % of the synthetic frames below are
ambiguous in the oracle alone, all limb pixels), render_cases.wrong_surfaces asks in addition that
no pixel shows another surface than the oracle's unless a tie or a silhouette through the sample
explains it: measured 0 in every case.

Measured on an MI355X (differing / ambiguous / unexplained per env, of 7,488 pixels; distinct geoms
hit per env; wall time of the case, nearly all of it the oracle on the CPU):
  scene     front                      side                       hand
  cable     0/0/0  55, 56  0.9 s       0/0/0  45, 50  0.7 s       0/0/0  25, 25  2.7 s
  insert    0/0/0  34, 36  0.6 s       0/0/0  38, 43  0.7 s       0/0/0  18, 16  2.6 s
  door      0/0/0  31, 33  0.6 s       2/2/0  37, 42  0.7 s       0/0/0  15, 16  2.7 s
  cabinet   0/0/0  32, 31  0.6 s       0/0/0  43, 48  0.7 s       0/0/0  15, 16  2.6 s
  toolbox   0/0/0  34, 36  0.6 s       0/0/0  38, 43  0.7 s       0/0/0  16, 18  2.6 s
  ring      1/1/0  42, 44  0.6 s       0/0/0  46, 51  0.7 s       0/0/0  15, 16  2.6 s
  pick      0/0/0  34, 38  1.0 s       1/1/0  40, 45  1.3 s       0/0/0  16, 17  3.1 s
Cable front at 103 x 71: 0/0/0 of 7,313, 0.7 s.  Every synthetic case (centre-pixel closed forms x
10, primitives over the sky, without materials, cached x 2, spheres at tile borders, triangles,
materials, 128 spheres): 0/0/0 of 3,072 or 6,144 pixels, each under 0.05 s.  Active mask, tile
groups and policy forms: bitwise, each under 0.4 s.  CPU guard: the oracle alone calls 0.79 % of
Cable front's 104 x 72 pixels ambiguous with the scaled jitter, 1.0 s.  The whole file: 38 s.

That the cases can fail was checked once with four deliberately wrong kernels (not kept): a wrong
red value at even rows and columns fails every every-pixel case while test_render_gpu.py still
passes; one kernel with a reversed skybox gradient, a flat background of 0.92 and a 2d texture
extent of s[1] on round geoms fails the sky, no-material, material and centre-pixel cases; one with
a visibility pass that ignores `active` and a tile split that drops a tile fails the mask and group
cases; a sphere bounding radius of 0.8 r fails only test_spheres_poking_across_tile_borders, and
there only through wrong_surfaces.
"""

import functools
import time

import numpy as np
import pytest
import torch

import render_cases as RC
from oracle import render as OR

gpu = pytest.mark.gpu
DEV = "cuda:0"
W, H = 104, 72  # 6.5 x 4.5 tiles of 16 x 16: ragged tiles in both directions, both sizes even
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# the Door scene's box with a "2d" texture (geom 77, the only one in the shipped scenes) is in the
# frame of these cameras (CPU census of the oracle at the poses below)
DOOR_2D_BOX_CAMERAS = ("front", "side")


def _buffers(n, h, w, fill=None):
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=DEV)
    depth = torch.empty((n, h, w), dtype=torch.float32, device=DEV)
    hit = torch.empty((n, h, w), dtype=torch.int32, device=DEV)
    if fill is not None:
        rgb.fill_(fill[0])
        depth.fill_(fill[1])
        hit.fill_(fill[2])
    return rgb, depth, hit


def _frame(rnd, eng, cam, **kw):
    out = _buffers(eng.n_env, rnd.height, rnd.width, fill=(9, -5.0, -7))  # (sentinels: an unwritten pixel shows)
    rnd.render(eng, cam, rgb=out[0], depth=out[1], hit_geom=out[2], **kw)
    torch.cuda.synchronize()
    return out


def _check_against_oracle(what, arrays, poses, cam, w, h, frame, cap=RC.AMBIGUOUS_CAP, surfaces=False):
    """compare_frame on every pixel of every env; the counts are printed before they are asserted.
    surfaces: also no wrong surface that a tie or a silhouette does not explain
    (render_cases.wrong_surfaces)."""
    rgb, depth, hit = (t.cpu().numpy() for t in frame)
    prims = OR.scene_prims(arrays)
    xs, ys = RC.all_pixels(w, h)
    out = []
    for e, pose in enumerate(poses):
        res = RC.compare_frame(arrays, prims, pose, cam, w, h, xs, ys, hit[e], depth[e], rgb[e])
        print(f"{what} env{e}: differing {res.differing}, ambiguous {res.ambiguous}, unexplained "
              f"{len(res.unexplained)} of {len(xs)}")
        out.append(res)
        if surfaces:
            wrong = RC.wrong_surfaces(arrays, prims, pose, cam, w, h, xs, ys, hit[e], res)
            print(f"{what} env{e}: wrong surfaces {len(wrong)}")
            assert len(wrong) == 0, (what, e, [(int(xs[k]), int(ys[k]), int(hit[e][ys[k], xs[k]]), int(res.og[k]))
                                               for k in wrong[:8]])
    for e, res in enumerate(out):
        assert len(res.unexplained) == 0, (what, e, len(res.unexplained), res.detail)
        assert res.ambiguous <= cap * len(xs), (what, e, res.ambiguous)
    return out


# ---- B. every pixel of a small frame, every scene, every camera ----------------------------------
@functools.lru_cache(maxsize=None)
def _asset(name):
    arrays, eng = RC.asset_engine(name, DEV)
    return arrays, eng, [RC.engine_pose(eng, e) for e in range(eng.n_env)]


@gpu
@torch.no_grad()
@pytest.mark.parametrize("cam", RC.CAMERAS)
@pytest.mark.parametrize("name", RC.ASSETS)
def test_every_pixel_of_every_scene_and_camera(name, cam):
    from robomanipbaselines_amd.render import Renderer

    t0 = time.time()
    arrays, eng, poses = _asset(name)
    assert "rmesh_tri" in arrays and "geom_matinfo" in arrays
    rnd = Renderer(arrays, DEV, width=W, height=H)
    frame = _frame(rnd, eng, cam)
    assert bool((rnd._vis == -1).all()) and bool((rnd._tflag == 0).all())  # the workspaces are empty again
    res = _check_against_oracle(f"{name} {cam}", arrays, poses, cam, W, H, frame, surfaces=True)
    hit = frame[2].cpu().numpy()
    for e in range(2):
        assert np.unique(hit[e][hit[e] >= 0]).size >= 15, (name, cam, e)
    print(f"{name} {cam}: distinct geoms hit {[int(np.unique(h_[h_ >= 0]).size) for h_ in hit]}, "
          f"{time.time() - t0:.1f} s")
    if name == "ur5e_door" and cam in DOOR_2D_BOX_CAMERAS:
        box2d = [g for g in np.nonzero(arrays["geom_texid"] >= 0)[0]
                 if arrays["geom_type"][g] == 6 and arrays["tex_type"][arrays["geom_texid"][g]] == 0]
        assert len(box2d) == 1
        assert (hit == box2d[0]).sum() > 0 and (res[0].og == box2d[0]).sum() > 0, cam


@gpu
@torch.no_grad()
def test_odd_frame_size_and_its_space_to_depth_refusal():
    """103 x 71: no even row or column count anywhere; rgb, depth and hit against the oracle on every
    pixel.  The space-to-depth policy forms need an even size: refused, the tensor not written."""
    from robomanipbaselines_amd.render import Renderer

    arrays, eng, poses = _asset("ur5e_cable")
    w, h = 103, 71
    rnd = Renderer(arrays, DEV, width=w, height=h)
    _check_against_oracle("ur5e_cable front 103x71", arrays, poses, "front", w, h, _frame(rnd, eng, "front"))
    for dt in (torch.bfloat16, torch.float32, torch.uint8):
        pol = torch.full((2, h // 2, w // 2, 16), 7, dtype=dt, device=DEV)
        with pytest.raises(ValueError, match="even image size"):
            rnd.render(eng, "front", policy=pol)
        torch.cuda.synchronize()
        assert bool((pol == 7).all()), dt
    # and the Renderer still draws the same frame afterwards (its workspaces were left empty)
    for a, b in zip(_frame(rnd, eng, "front"), _frame(Renderer(arrays, DEV, width=w, height=h), eng, "front")):
        assert torch.equal(a, b)


@gpu
@torch.no_grad()
@pytest.mark.parametrize("cam", ["side", "hand"])
def test_policy_forms_agree_on_the_ragged_frame(cam):
    from robomanipbaselines_amd import kernels as K
    from robomanipbaselines_amd.render import Renderer

    arrays, eng, _ = _asset("ur5e_door")
    rnd = Renderer(arrays, DEV, width=W, height=H)
    rgb = _frame(rnd, eng, cam)[0]
    got = {}
    for key, shape, dt in (("chw32", (2, 3, H, W), torch.float32), ("chw16", (2, 3, H, W), torch.bfloat16),
                           ("s2d32", (2, H // 2, W // 2, 16), torch.float32),
                           ("s2d16", (2, H // 2, W // 2, 16), torch.bfloat16),
                           ("s2d8", (2, H // 2, W // 2, 16), torch.uint8)):
        got[key] = torch.full(shape, 3, dtype=dt, device=DEV)  # (a sentinel: every element must be written)
        rnd.render(eng, cam, policy=got[key], mean=MEAN, std=STD)
    torch.cuda.synchronize()
    assert torch.equal(K.image_to_s2d(got["chw32"]), got["s2d32"])
    assert torch.equal(K.image_to_s2d(got["chw16"]), got["s2d16"])
    assert torch.equal(K.image_to_s2d(rgb.permute(0, 3, 1, 2)), got["s2d8"])
    want = rgb.permute(0, 3, 1, 2).double() / 255.0
    want = (want - torch.tensor(MEAN, dtype=torch.float64, device=DEV).view(1, 3, 1, 1)) \
        / torch.tensor(STD, dtype=torch.float64, device=DEV).view(1, 3, 1, 1)
    torch.testing.assert_close(got["chw32"].double(), want, rtol=0, atol=1e-6)
    # bf16 is the f32 value rounded once
    assert torch.equal(got["chw16"], got["chw32"].to(torch.bfloat16))


# ---- C. synthetic scenes ------------------------------------------------------------------------
SKY = ((0.2, 0.4, 0.6), (0.8, 0.6, 0.4))
C70 = (np.cos(np.deg2rad(35.0)), np.sin(np.deg2rad(35.0)), 0.0, 0.0)  # the camera turned 70 degrees up about x


def _flat_materials(a, sky=SKY, spec=0.0, shin=0.5, emission=0.0):
    n = len(a["geom_type"])
    return RC.add_materials(a, [], np.full(n, -1), np.tile([spec, shin, 1.0, 1.0, 0.0, emission], (n, 1)), sky=sky)


def _in_camera_frame(a, pos, gxmat, quat):
    """Turn the scene's camera by `quat` and move the geoms with it (their camera-frame places stay)."""
    R = OR._quat2mat(np.asarray(quat, np.float64))
    a["cam_quat"] = np.array([quat], np.float64)
    return a, pos @ R.T, np.stack([(R @ m.reshape(3, 3)).reshape(9) for m in gxmat])


def _render(a, pos, gxmat, w, h, n_env=1, **eng_kw):
    from robomanipbaselines_amd.render import Renderer

    eng = RC.SceneEngine(pos, gxmat, n_env, DEV, **eng_kw)
    rnd = Renderer(a, DEV, width=w, height=h)
    return rnd, eng, _frame(rnd, eng, "cam")


def _sphere_depth(d, c, r):
    """Camera depth of the ray t d (d_z = -1) entering the sphere (c, r): the smaller root."""
    A, B, Cc = d @ d, d @ c, c @ c - r * r
    return (B - np.sqrt(B * B - A * Cc)) / A


CENTRE_CASES = {  # type, size, centre depth along the centre pixel's ray -> closed-form depth of that ray
    "sphere": (2, (0.3, 0, 0)), "box": (6, (0.2, 0.3, 0.4)), "cylinder": (5, (0.25, 0.5, 0)),
    "capsule": (3, (0.1, 0.4, 0)), "plane": (0, (0, 0, 0))}


@gpu
@torch.no_grad()
@pytest.mark.parametrize("materials", [True, False])
@pytest.mark.parametrize("kind", list(CENTRE_CASES))
def test_centre_pixel_closed_forms_of_each_primitive(kind, materials):
    """One primitive 2 m (the plane 3 m) down the view axis, axes along the camera's, as in
    test_render_oracle.py's centre-ray cases; the GPU's centre pixel (32, 24) looks half a pixel off
    the axis, through d = pixel_ray(32, 24).  Depth: the sphere's smaller root; the capsule's cap
    sphere; the flat faces of box (2 - 0.4), cylinder (2 - 0.5) and plane (3) exactly (camera depth
    of a plane z = const).  Colour of the flat faces (n = +z = towards the light): rgb (0.1 + 0.6 /
    |d| + 0.3), plus with materials the specular 0.5 x 0.3 x (h_z)^(128 x 0.7) and the emission."""
    w, h = 64, 48
    t, size = CENTRE_CASES[kind]
    z = -3.0 if kind == "plane" else -2.0
    col = np.array([0.5, 0.4, 0.2])
    a, pos, gm = RC.scene([(t, size, (0, 0, z), col)])
    if materials:
        _flat_materials(a, spec=0.5, shin=0.7, emission=0.05)
    rnd, eng, frame = _render(a, pos, gm, w, h)
    rgb, depth, hit = (x.cpu().numpy()[0] for x in frame)
    d = RC.pixel_ray(32, 24, w, h)
    c = np.array([0, 0, z])
    want = {"sphere": lambda: _sphere_depth(d, c, 0.3), "capsule": lambda: _sphere_depth(d, c + [0, 0, 0.4], 0.1),
            "box": lambda: 1.6, "cylinder": lambda: 1.5, "plane": lambda: 3.0}[kind]()
    assert hit[24, 32] == 0
    np.testing.assert_allclose(depth[24, 32], want, rtol=RC.DEPTH_RTOL, atol=RC.DEPTH_ATOL)
    if kind in ("box", "cylinder", "plane"):
        v = -d / np.linalg.norm(d)
        shade = 0.1 + 0.6 * v[2] + 0.3
        if materials:
            hv = (v + [0, 0, 1.0]) / np.linalg.norm(v + [0, 0, 1.0])
            want8 = OR.to_u8(np.minimum(col * (shade + 0.05) + 0.5 * 0.3 * hv[2] ** (128 * 0.7), 1.0))
        else:
            want8 = OR.to_u8(np.minimum(col * shade, 1.0))
        assert np.abs(rgb[24, 32].astype(int) - want8.astype(int)).max() <= 1, (rgb[24, 32], want8)
    _check_against_oracle(f"centre {kind} materials={materials}", a, [eng.pose(0)], "cam", w, h, frame, surfaces=True)


def _primitives(welded=None):
    """One of each bounded primitive type and a second, turned box and capsule, well separated in
    the camera frame, no plane: most of the frame is background."""
    objs = [(2, (0.22, 0, 0), (-0.9, 0.45, -2.6), (0.9, 0.3, 0.2)),        # sphere
            (3, (0.08, 0.3, 0), (-0.25, 0.4, -2.2), (0.2, 0.8, 0.3)),      # capsule
            (5, (0.15, 0.25, 0), (0.45, 0.45, -2.4), (0.3, 0.4, 0.9)),     # cylinder
            (6, (0.2, 0.12, 0.3), (1.0, -0.35, -2.8), (0.8, 0.8, 0.2)),    # box
            (6, (0.25, 0.1, 0.15), (-0.7, -0.4, -2.0), (0.6, 0.3, 0.7)),   # box, turned
            (3, (0.06, 0.35, 0), (0.1, -0.45, -1.8), (0.9, 0.9, 0.9)),     # capsule, turned
            (2, (0.1, 0, 0), (0.55, -0.1, -1.2), (0.2, 0.7, 0.7))]         # a small near sphere
    a, pos, gm = RC.scene(objs, welded=welded)
    gm[1] = RC.rot((1, 0, 0), 90)
    gm[2] = RC.rot((1, 0.3, 0), 55)
    gm[3] = RC.rot((0, 1, 0), 30)
    gm[4] = RC.rot((1, 1, 1), 40)
    gm[5] = RC.rot((0.2, 1, 0), 75)
    return a, pos, gm


@gpu
@torch.no_grad()
def test_primitives_over_the_gradient_skybox():
    """render_kernel<false, 0> with materials: no mesh, no plane; the background is hit_geom -1, the
    depth float32(zfar) and the skybox gradient rgb2 + (1 + w_z) / 2 (rgb1 - rgb2) of the ray's
    world z (closed form, every background pixel); every primitive type is in the frame."""
    w, h = 96, 64
    a, pos, gm = _in_camera_frame(*_primitives(), C70)
    _flat_materials(a, spec=0.4, shin=0.3)
    rnd, eng, frame = _render(a, pos, gm, w, h, n_env=2)
    assert rnd.mesh_tri is None and rnd.materials
    rgb, depth, hit = (x.cpu().numpy() for x in frame)
    res = _check_against_oracle("primitives over the sky", a, [eng.pose(0), eng.pose(1)], "cam", w, h, frame, surfaces=True)
    assert set(np.unique(hit[0]).tolist()) == {-1, 0, 1, 2, 3, 4, 5, 6}
    bg = hit[0] == -1
    assert 0.5 < bg.mean() < 0.95 and np.array_equal(bg, (res[0].og == -1).reshape(h, w))
    zfar = np.float32(float(a["_zfar"]) * float(a["_extent"]))
    assert zfar == np.float32(100.0) and (depth[0][bg] == zfar).all()
    xs, ys = RC.all_pixels(w, h)
    R = OR._quat2mat(np.asarray(C70))
    dirs = np.stack([RC.pixel_ray(x, y, w, h) for x, y in zip(xs, ys)])
    wz = (dirs @ R.T)[:, 2] / np.linalg.norm(dirs, axis=1)
    sky = np.asarray(SKY[1]) + 0.5 * (1 + wz)[:, None] * (np.asarray(SKY[0]) - np.asarray(SKY[1]))
    want8 = OR.to_u8(sky).reshape(h, w, 3).astype(int)
    assert np.abs(rgb[0].astype(int) - want8)[bg].max() <= 1
    assert len(np.unique(rgb[0][bg], axis=0)) > 20  # a gradient, not one colour
    assert torch.equal(frame[0][0], frame[0][1]) and torch.equal(frame[1][0], frame[1][1])  # equal envs


def _spheres_at_tile_borders(w, h):
    """Four spheres of about 10 pixels radius, each with its centre 0.9 radius away from the plane
    through the eye and a border between two 16-pixel tiles (x = 32 and 64, y = 16 and 48; towards
    either side): a tenth of the sphere pokes into the neighbouring tile, where a culling bound that
    is a little too tight (the bounding radius, the projected box) would drop it."""
    r, t0 = 0.26, 2.0
    objs, borders = [], []
    for axis, b, side, other in ((0, 32, -1, 0.30), (0, 64, 1, -0.25), (1, 16, 1, 0.1), (1, 48, -1, -0.3)):
        edge = RC.pixel_ray(b - 0.5, b - 0.5, w, h)[axis]  # the border's slope (pixel_ray takes the centre of px + 0.5)
        n = np.zeros(3)
        n[axis], n[2] = 1.0, edge
        n /= np.linalg.norm(n)
        on_plane = np.zeros(3)
        on_plane[axis], on_plane[1 - axis], on_plane[2] = edge * t0, other, -t0
        objs.append((2, (r, 0, 0), tuple(on_plane + side * 0.9 * r * n), (0.8, 0.5 + 0.1 * len(objs), 0.3)))
        borders.append((axis, b, side))
    return RC.scene(objs), borders


@gpu
@torch.no_grad()
def test_spheres_poking_across_tile_borders():
    w, h = 96, 64
    (a, pos, gm), borders = _spheres_at_tile_borders(w, h)
    _flat_materials(a)
    rnd, eng, frame = _render(a, pos, gm, w, h)
    res = _check_against_oracle("spheres at tile borders", a, [eng.pose(0)], "cam", w, h, frame, surfaces=True)
    og = res[0].og.reshape(h, w)
    for g, (axis, b, side) in enumerate(borders):  # the sliver beyond the border is there to be dropped
        ys, xs = np.nonzero(og == g)
        c = xs if axis == 0 else ys
        low = side > 0 if axis == 0 else side < 0  # (the image's y runs down, the camera's up)
        beyond = (c < b) if low else (c >= b)
        assert 3 <= beyond.sum() < 0.2 * len(c), (g, int(beyond.sum()), len(c))


@gpu
@torch.no_grad()
def test_primitives_without_material_arrays_and_the_entry_point_without_meshes():
    """geom_matinfo NULL: flat material colours, the background exactly (230, 255, 255) -- through
    Renderer (rmbx_render_scene_cached) and through rmbx_render, the exported entry point without
    meshes, which must give the same frame."""
    import ctypes

    from robomanipbaselines_amd import _native as N

    w, h = 96, 64
    a, pos, gm = _in_camera_frame(*_primitives(), C70)
    rnd, eng, frame = _render(a, pos, gm, w, h)
    assert rnd.mesh_tri is None and not rnd.materials
    rgb, depth, hit = (x.cpu().numpy() for x in frame)
    _check_against_oracle("primitives, no materials", a, [eng.pose(0)], "cam", w, h, frame, surfaces=True)
    bg = hit[0] == -1
    assert 0.5 < bg.mean() < 0.95
    assert (rgb[0][bg] == np.array([230, 255, 255], np.uint8)).all()
    assert (depth[0][bg] == np.float32(100.0)).all()
    rgb2, depth2, _ = _buffers(1, h, w, fill=(9, -5.0, -7))
    chw = torch.full((1, 3, h, w), -9.0, dtype=torch.float32, device=DEV)
    cam = rnd.camera("cam")
    N.call("rmbx_render", ctypes.byref(cam), N.ptr(rnd.prim_i32), N.ptr(rnd.prim_f32), rnd.nprim, N.ptr(eng.gxpos),
           N.ptr(eng.gxmat), N.ptr(eng.xpos), N.ptr(eng.xquat), eng.ngeom, eng.nbody, N.ptr(rgb2), N.ptr(depth2),
           N.ptr(chw), 0, None, 1, N.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(rgb2, frame[0]) and torch.equal(depth2, frame[1])
    want = (frame[0].permute(0, 3, 1, 2).double() / 255.0
            - torch.tensor(MEAN, dtype=torch.float64, device=DEV).view(1, 3, 1, 1)) \
        / torch.tensor(STD, dtype=torch.float64, device=DEV).view(1, 3, 1, 1)
    torch.testing.assert_close(chw.double(), want, rtol=0, atol=1e-6)


@gpu
@torch.no_grad()
@pytest.mark.parametrize("materials", [True, False])
def test_static_cache_without_meshes_equals_the_full_render(materials, monkeypatch):
    """render_kernel<false, 2> (cache built) and <false, 1> (cache reused after the moving body's
    primitives moved), bitwise equal to RMBX_RENDER_CACHE=0 (render_kernel<false, 0>): four
    primitives welded to the world, three on a moving body, a world camera."""
    from robomanipbaselines_amd.render import Renderer

    w, h = 96, 64
    welded = [1, 0, 1, 1, 0, 1, 0]
    a, pos, gm = _in_camera_frame(*_primitives(welded), C70)
    if materials:
        _flat_materials(a, spec=0.4, shin=0.3)
    pos2 = np.stack([pos, pos])
    pos2[1, 1] += (0.1, 0.0, 0.05)  # env 1 differs: its caches are its own
    eng = RC.SceneEngine(pos2, gm, 2, DEV)
    rnd = Renderer(a, DEV, width=w, height=h)
    assert rnd.prim_static.tolist() == welded

    def both(what, want_dirty):
        monkeypatch.setenv("RMBX_RENDER_CACHE", "1")
        got = _frame(rnd, eng, "cam")
        assert rnd._caches["cam"][4].tolist() == want_dirty, what
        s2d = torch.empty((2, h // 2, w // 2, 16), dtype=torch.uint8, device=DEV)
        rnd.render(eng, "cam", policy=s2d)
        monkeypatch.setenv("RMBX_RENDER_CACHE", "0")
        want = _frame(rnd, eng, "cam")
        s2d0 = torch.empty_like(s2d)
        rnd.render(eng, "cam", policy=s2d0)
        torch.cuda.synchronize()
        for name, x, y in zip(("rgb", "depth", "hit", "s2d"), got + (s2d,), want + (s2d0,)):
            assert torch.equal(x, y), (what, name, int((x != y).sum()))
        return want

    first = both("cache built", [1, 1])
    _check_against_oracle(f"cached primitives materials={materials}", a, [eng.pose(0), eng.pose(1)], "cam", w, h, first, surfaces=True)
    for g in (1, 4, 6):  # the moving body's primitives move (in front of and behind static ones)
        eng.gxpos[:, g, 0] += 0.12
        eng.gxpos[:, g, 2] -= 0.05
    moved = both("moving primitives moved", [0, 0])
    assert not torch.equal(first[2], moved[2])
    eng.gxpos[1, 3, 1] += 0.07  # one env's static primitive moves: that env alone rebuilds
    both("static primitive moved", [0, 1])
    both("after the rebuild", [0, 0])


def _mesh_scene():
    """One mesh: a quad of two large triangles at z = -1.5 (several hundred pixel centres each: the
    whole-wave path), a fan of small triangles beside it (the per-lane path), a triangle crossing
    the near plane (a horizontal strip 5 cm below the eye from 0.9 m ahead to 0.1 m behind it: the
    clipped projection has four edges; znear 0.02), a back-facing triangle 1 m away
    in front of the quad, and a sphere behind the quad's edge (the kernel needs a primitive)."""
    q = 0.5
    quad = [[[-q, -q, -1.5], [q, -q, -1.5], [q, q, -1.5]], [[-q, -q, -1.5], [q, q, -1.5], [-q, q, -1.5]]]
    fan, c = [], np.array([0.72, 0.2, -1.4])
    for k in range(12):  # 12 triangles of a 4 cm disc: about 2 pixels each
        a0, a1 = 2 * np.pi * k / 12, 2 * np.pi * (k + 1) / 12
        fan.append([c, c + 0.04 * np.array([np.cos(a0), np.sin(a0), 0.3 * np.cos(a0)]),
                    c + 0.04 * np.array([np.cos(a1), np.sin(a1), 0.3 * np.cos(a1)])])
    near = [[[-0.3, -0.05, -0.9], [0.0, -0.05, 0.1], [0.3, -0.05, -0.9]]]  # 5 cm below the eye, to behind it
    back = [[[-0.2, 0.1, -1.0], [0.0, 0.3, -1.0], [0.2, 0.1, -1.0]]]  # clockwise seen from the camera
    tris = quad + [[list(map(float, v)) for v in t] for t in fan] + near + back
    return RC.scene([(2, (0.3, 0, 0), (0.55, -0.45, -2.5), (0.9, 0.2, 0.2))], tris=tris), len(quad) + len(fan)


@gpu
@torch.no_grad()
def test_large_small_clipped_and_back_facing_triangles():
    w, h = 96, 64
    (a, pos, gm), i_near = _mesh_scene()
    a["rmesh_body"] = np.array([1], np.int32)  # the mesh on body 1: at the origin in env 0, moved and turned in env 1
    _flat_materials(a)
    xpos = np.zeros((2, 2, 3))
    xquat = np.tile([1.0, 0, 0, 0], (2, 2, 1))
    xpos[1, 1] = (0.05, -0.03, -0.1)
    xquat[1, 1] = (np.cos(np.deg2rad(10)), 0, 0, np.sin(np.deg2rad(10)))
    rnd, eng, frame = _render(a, pos, gm, w, h, n_env=2, xpos=xpos, xquat=xquat)
    assert rnd.mesh_tri is not None
    rgb, depth, hit = (x.cpu().numpy() for x in frame)
    res = _check_against_oracle("triangles", a, [eng.pose(0), eng.pose(1)], "cam", w, h, frame, surfaces=True)
    mesh = 1
    # the quad: its projection (closed form: |x|, |y| < 0.5 at depth 1.5) minus the pixels the clipped
    # triangle covers in front of it; more than 64 x RASTER_SMALL centres, across 16-pixel tile borders
    xs, ys = RC.all_pixels(w, h)
    dirs = np.stack([RC.pixel_ray(x, y, w, h) for x, y in zip(xs, ys)]).reshape(h, w, 3)
    inside = (np.abs(dirs[..., 0] * 1.5) < 0.499) & (np.abs(dirs[..., 1] * 1.5) < 0.499)
    quad_px = inside & (np.abs(depth[0] - 1.5) <= 1.5 * RC.DEPTH_RTOL + RC.DEPTH_ATOL) & (hit[0] == mesh)
    assert (hit[0][inside] == mesh).all()
    assert quad_px.sum() > 1000 and (quad_px.sum() + (inside & (depth[0] < 1.0)).sum()) == inside.sum()
    # the back face at depth 1.0 is not drawn: the quad (1.5) is seen through its centroid
    py, px = np.argwhere((np.abs(dirs[..., 0] - 0.0) < 0.01) & (np.abs(dirs[..., 1] - 0.17) < 0.01))[0]
    assert hit[0, py, px] == mesh and abs(depth[0, py, px] - 1.5) < 2e-4
    assert not (np.abs(depth[0] - 1.0) < 1e-3).any()
    # the clipped triangle: drawn where its plane is hit beyond znear, depth by the ray-plane
    # intersection (closed form); nothing nearer than znear anywhere
    tr = a["rmesh_tri"][i_near].astype(np.float64)
    v0, nrm = tr[0:3], np.cross(tr[3:6], tr[6:9])
    tpl = (v0 @ nrm) / (dirs @ nrm)
    near_px = (hit[0] == mesh) & (depth[0] < 0.9)
    assert near_px.sum() > 100 and near_px[h - 1].any()  # it runs off the bottom edge of the image
    np.testing.assert_allclose(depth[0][near_px], tpl[near_px], rtol=RC.DEPTH_RTOL, atol=RC.DEPTH_ATOL)
    assert depth[0].min() > 0.02 and depth[0][near_px].min() < 0.15
    # the fan of small triangles is in the frame
    fan_px = (hit[0] == mesh) & (dirs[..., 0] * 1.4 > 0.6) & (depth[0] > 1.3) & (depth[0] < 1.5)
    assert 10 < fan_px.sum() < 40, int(fan_px.sum())
    assert (res[1].og == mesh).sum() > 1000 and not np.array_equal(hit[0], hit[1])


def _textures():
    rng = np.random.default_rng(5)
    smooth = lambda hh, ww: np.clip(  # noqa: E731
        128 + 100 * np.sin(np.arange(hh)[:, None, None] * 0.9 + np.arange(3)) * np.cos(np.arange(ww)[None, :, None] * 0.7)
        + rng.integers(-20, 20, (hh, ww, 3)), 0, 255).astype(np.uint8)
    return [(1, smooth(8, 8)), (0, smooth(16, 4)), (0, smooth(5, 7)), (1, smooth(4, 16))]


def _material_scene():
    a, pos, gm = _primitives()
    #            sphere: cube  capsule: cube/uni  cylinder: 2d  box: 2d/uni  box: 2d  capsule: none  sphere: cube/uni
    geom_tex = [0, 3, 1, 2, 1, -1, 3]
    matinfo = [[0.8, 0.3, 1, 1, 0, 0.0], [0.0, 0.5, 1, 1, 1, 0.2], [0.3, 0.6, 3, 2, 0, 0.0], [0.0, 0.5, 2.5, 1.5, 1, 0.1],
               [0.5, 0.2, 2, 3, 0, 0.3], [0.9, 0.25, 1, 1, 0, 0.0], [0.2, 0.9, 1, 1, 1, 0.0]]
    return RC.add_materials(a, _textures(), geom_tex, matinfo, sky=SKY), pos, gm


@gpu
@torch.no_grad()
def test_material_combinations_the_shipped_scenes_lack():
    """A cube texture on a sphere (and, texuniform, on a capsule and a sphere), a 2d texture on a box
    and on a cylinder, texuniform 0 and 1, texrepeat != 1, non-square and non-power-of-two images,
    emission, and specular highlights (spheres and capsules always show theirs: some visible normal
    is the half vector)."""
    w, h = 96, 64
    a, pos, gm = _in_camera_frame(*_material_scene(), C70)
    rnd, eng, frame = _render(a, pos, gm, w, h)
    rgb, depth, hit = (x.cpu().numpy() for x in frame)
    res = _check_against_oracle("materials", a, [eng.pose(0)], "cam", w, h, frame, surfaces=True)
    assert set(np.unique(hit[0]).tolist()) == {-1, 0, 1, 2, 3, 4, 5, 6}
    # the textures are really sampled: the same scene without them differs on every textured geom
    a0, p0, g0 = _in_camera_frame(*_material_scene(), C70)
    a0["geom_texid"][:] = -1
    flat = _render(a0, p0, g0, w, h)[2][0].cpu().numpy()
    for g in (0, 1, 2, 3, 4, 6):
        assert (np.abs(flat[0].astype(int) - rgb[0].astype(int)).max(-1)[hit[0] == g] > RC.RGB_TOL).mean() > 0.5, g
    assert np.array_equal(flat[0][hit[0] == 5], rgb[0][hit[0] == 5])
    # the highlight of the untextured capsule (colour 0.9, specular 0.9, no emission): some pixel is
    # brighter than colour x full shade (0.9 x 1.0 = 230 / 255) can be without the specular term
    assert rgb[0][hit[0] == 5].min(-1).max() > 232


def _sphere_grid(n):
    """n small spheres on a 16-column grid 3 m away, filling the 96 x 64 frame."""
    objs = []
    for k in range(n):
        i, j = k % 16, k // 16
        objs.append((2, (0.05 + 0.002 * (k % 5), 0, 0), (-1.65 + 0.22 * i, -1.0 + 0.25 * j, -3.0 - 0.01 * (k % 7)),
                     (0.2 + 0.05 * (k % 16), 0.9 - 0.1 * (k // 16), 0.5)))
    return RC.scene(objs)


@gpu
@torch.no_grad()
def test_128_primitives_render_and_129_are_refused():
    w, h = 96, 64
    a, pos, gm = _sphere_grid(128)
    _flat_materials(a)
    rnd, eng, frame = _render(a, pos, gm, w, h)
    assert rnd.nprim == 128
    _check_against_oracle("128 spheres", a, [eng.pose(0)], "cam", w, h, frame, surfaces=True)
    seen = set(np.unique(frame[2].cpu().numpy()).tolist()) - {-1}
    assert len(seen) >= 120 and 0 in seen and 127 in seen, len(seen)
    a, pos, gm = _sphere_grid(129)
    _flat_materials(a)
    from robomanipbaselines_amd.render import Renderer

    eng = RC.SceneEngine(pos, gm, 1, DEV)
    rnd = Renderer(a, DEV, width=w, height=h)
    rgb, depth, hit = _buffers(1, h, w, fill=(9, -5.0, -7))
    pol = torch.full((1, 3, h, w), -9.0, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="nprim=129"):
        rnd.render(eng, "cam", rgb=rgb, depth=depth, hit_geom=hit, policy=pol)
    torch.cuda.synchronize()
    assert bool((rgb == 9).all()) and bool((depth == -5.0).all()) and bool((hit == -7).all()) and bool((pol == -9.0).all())


# ---- D. the active mask -------------------------------------------------------------------------
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
    return arrays, eng


@gpu
@torch.no_grad()
@pytest.mark.parametrize("cam", ["front", "hand"])
def test_active_mask_skips_an_env_and_leaves_no_trace(cam):
    """active = [1, 0, 1]: env 1's outputs keep their sentinels, envs 0 and 2 are bitwise the
    unmasked frames, and the visibility workspaces are empty again for every env.  Then the arms
    move and an unmasked call equals a fresh Renderer's frames of the new state on all three envs:
    nothing of the masked call survives in the skipped env, whose static cache (front: a world
    camera) is built on that call, dirty == [0, 1, 0]."""
    from robomanipbaselines_amd.render import Renderer

    arrays, eng = _cable3()
    n = 3

    def everything(rnd, active=None, fill=None):
        rgb, depth, hit = _buffers(n, H, W, fill=fill)
        s2d = torch.full((n, H // 2, W // 2, 16), 77, dtype=torch.uint8, device=DEV)
        chw = torch.full((n, 3, H, W), -9.0, dtype=torch.float32, device=DEV)
        rnd.render(eng, cam, rgb=rgb, depth=depth, hit_geom=hit, policy=s2d, active=active)
        dirty = rnd._caches[cam][4].tolist() if cam in rnd._caches else None
        rnd.render(eng, cam, policy=chw, active=active)
        torch.cuda.synchronize()
        return (rgb, depth, hit, s2d, chw), dirty

    names = ("rgb", "depth", "hit", "s2d", "chw")
    want, dirty = everything(Renderer(arrays, DEV, width=W, height=H))
    assert dirty == ([1, 1, 1] if cam == "front" else None)
    rnd = Renderer(arrays, DEV, width=W, height=H)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV)
    got, dirty = everything(rnd, active=active, fill=(9, -5.0, -7))
    sentinels = (9, -5.0, -7, 77, -9.0)
    for name, g, w_, s in zip(names, got, want, sentinels):
        assert bool((g[1] == s).all()), (name, "the skipped env was written")
        assert torch.equal(g[0], w_[0]) and torch.equal(g[2], w_[2]), name
        assert not bool((w_[1] == s).all()), name
    if cam == "front":
        assert dirty[0] == 1 and dirty[2] == 1
    assert bool((rnd._vis == -1).all()) and bool((rnd._tflag == 0).all())  # empty again, the skipped env too
    q = eng.qpos.clone()
    q[:, :6] += torch.tensor([0.3, 0.2, -0.25, 0.4, -0.3, 0.5], dtype=torch.float64, device=DEV)
    eng.qpos.copy_(q)
    eng.forward()
    again, dirty = everything(rnd)
    assert dirty == ([0, 1, 0] if cam == "front" else None)
    fresh, _ = everything(Renderer(arrays, DEV, width=W, height=H))
    for name, g, w_, old in zip(names, again, fresh, want):
        assert torch.equal(g, w_), (name, int((g != w_).sum()))
        assert not torch.equal(w_[1], old[1]), name  # the arm moved in the skipped env's frame
    assert bool((rnd._vis == -1).all()) and bool((rnd._tflag == 0).all())


# ---- E. tile-group invariance -------------------------------------------------------------------
@gpu
@torch.no_grad()
@pytest.mark.parametrize("cam", ["front", "hand"])
def test_tile_groups_do_not_change_the_frame(cam, monkeypatch):
    """RMBX_RENDER_GROUPS = 1, 2, 7, 35 (one tile per block: 7 x 5 tiles) and the default split give
    bitwise the same rgb, depth, hit and space-to-depth policy; 0 and 36 are refused and the next
    valid call is right."""
    from robomanipbaselines_amd.render import Renderer

    arrays, eng, _ = _asset("ur5e_door")
    rnd = Renderer(arrays, DEV, width=W, height=H)

    def everything():
        out = _frame(rnd, eng, cam)
        s2d = torch.full((2, H // 2, W // 2, 16), 3.0, dtype=torch.bfloat16, device=DEV)
        rnd.render(eng, cam, policy=s2d)
        torch.cuda.synchronize()
        return out + (s2d,)

    monkeypatch.delenv("RMBX_RENDER_GROUPS", raising=False)
    want = everything()
    for g in ("1", "2", "7", "35"):
        monkeypatch.setenv("RMBX_RENDER_GROUPS", g)
        for name, x, y in zip(("rgb", "depth", "hit", "s2d"), everything(), want):
            assert torch.equal(x, y), (g, name, int((x != y).sum()))
        for bad in ("0", "36"):
            monkeypatch.setenv("RMBX_RENDER_GROUPS", bad)
            rgb, depth, hit = _buffers(2, H, W, fill=(9, -5.0, -7))
            with pytest.raises(ValueError, match="RMBX_RENDER_GROUPS"):
                rnd.render(eng, cam, rgb=rgb, depth=depth, hit_geom=hit)
            torch.cuda.synchronize()
            assert bool((rgb == 9).all()) and bool((depth == -5.0).all()) and bool((hit == -7).all())
            monkeypatch.setenv("RMBX_RENDER_GROUPS", g)
            for name, x, y in zip(("rgb", "depth", "hit", "s2d"), everything(), want):
                assert torch.equal(x, y), (bad, g, name)


# ---- F. CPU guard against a vacuous comparison (no GPU) -----------------------------------------
def test_oracle_alone_calls_few_pixels_ambiguous():
    """Cable front at 104 x 72 with the scaled jitter: the share of pixels compare_frame would
    excuse wherever the GPU differed (a coincident second surface or a spread under jitter) stays
    <= 2 % -- a later change of the frame size or the jitter cannot silently turn the every-pixel
    tests into tests that excuse everything."""
    from robomanipbaselines_amd import model as MD

    arrays = MD.load("ur5e_cable")
    pose = RC.cpu_pose(arrays, RC.asset_qpos(arrays)[0])
    share = RC.oracle_ambiguous_share(arrays, OR.scene_prims(arrays), pose, "front", W, H)
    print(f"oracle-only ambiguous share, Cable front {W}x{H}: {share:.4f}")
    assert share <= 0.02, share
    assert abs(RC.jitter(H) - 0.003) < 1e-12 and RC.jitter(480) == 0.02
