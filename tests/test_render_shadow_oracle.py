"""CPU tests of the renderer's shadow rule and its host side (no GPU): the composed oracle of
tests/shadow_cases.py against closed forms, the stackless BVH tables of mjcf/bvh.py, the lights the
MJCF compiler emits and the shipped assets carry, and a guard that the every-pixel comparison of
test_render_shadow_gpu.py cannot pass vacuously.

Measured here (Cable at the render_cases.asset_qpos poses, 104 x 72 = 7,488 pixels, env 0 / 1):
front: the shadow changes 256 / 393 pixels by more than RGB_TOL (3.4 % / 5.2 %, above the 2 % cap
on excused pixels), and the oracle's own occlusion verdict flips under the jitter at well below 0.5 %
of the lit pixels."""

import os

import numpy as np
import pytest

import render_cases as RC
import shadow_cases as SC
from oracle import render as OR

W, H = 104, 72
SHADOW_SCENES = ("ur5e_cable", "ur5e_ring", "ur5e_pick")
PLAIN_SCENES = ("ur5e_insert", "ur5e_door", "ur5e_cabinet", "ur5e_toolbox")


# ---- closed form --------------------------------------------------------------------------------
def _look(pos, target):
    d = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    a = np.arctan2(d[1], -d[2])  # a turn about x takes the camera's -z to (0, sin a, -cos a)
    return (float(np.cos(a / 2)), float(np.sin(a / 2)), 0.0, 0.0)


def _project(arrays, pose, X, w, h):
    R, p = OR.camera_pose(arrays, "cam", pose.xpos, pose.xquat)
    t = np.tan(0.5 * float(arrays["cam_fovy"][0]) * np.pi / 180.0)
    c = R.T @ (np.asarray(X, np.float64) - p)
    view = (np.asarray(X, np.float64) - p) / np.linalg.norm(np.asarray(X, np.float64) - p)
    return np.array([(c[0] / -c[2] / (t * w / h) + 1) * w / 2, (1 - c[1] / -c[2] / t) * h / 2]), view


def _box_over_plane(cam_pos, target):
    c_plane, c_box = (0.8, 0.7, 0.6), (0.3, 0.5, 0.9)
    a, pos, gm = RC.scene([(0, (0, 0, 0.1), (0, 0, 0), c_plane), (6, (0.1, 0.1, 0.1), (0, 0, 0.5), c_box)],
                          cam_pos=cam_pos, cam_quat=_look(cam_pos, target))
    pose = RC.Pose(pos, gm, np.zeros((2, 3)), np.tile([1.0, 0, 0, 0], (2, 1)))
    return a, pose, np.array(c_plane), np.array(c_box)


def test_closed_form_box_over_plane():
    w, h = 64, 48
    a, pose, c_plane, c_box = _box_over_plane((0.0, -2.0, 1.5), (0.0, 0.0, 0.0))
    prims = OR.scene_prims(a)
    pts = [(0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (0.02, 0.03, 0.6)]
    proj = [_project(a, pose, X, w, h) for X in pts]
    c = SC.cast(a, prims, pose, "cam", w, h, np.stack([p for p, _ in proj]))
    assert c.geom.tolist() == [0, 0, 1] and c.occluded.tolist() == [True, False, False]
    ndv = [-v[2] for _, v in proj]  # the normals are +z
    np.testing.assert_allclose(c.rgb[0], c_plane * (0.1 + 0.6 * ndv[0]), rtol=0, atol=1e-12)  # under the box
    np.testing.assert_allclose(c.rgb[1], c_plane * (0.1 + 0.6 * ndv[1] + 0.3), rtol=0, atol=1e-12)  # beside it
    np.testing.assert_allclose(c.rgb[2], c_box * (0.1 + 0.6 * ndv[2] + 0.3), rtol=0, atol=1e-12)  # the box's top: lit
    # the shadow's edge is the box's outline: 0.099 in, 0.101 out
    edge = SC.cast(a, prims, pose, "cam", w, h, np.stack([_project(a, pose, (x, 0.0, 0.0), w, h)[0] for x in (0.099, 0.101)]))
    assert edge.occluded.tolist() == [True, False]


def test_closed_form_underside_is_unchanged():
    w, h = 64, 48
    a, pose, c_plane, c_box = _box_over_plane((0.0, -2.0, 0.1), (0.0, 0.0, 0.4))
    prims = OR.scene_prims(a)
    pix, view = _project(a, pose, (0.0, 0.0, 0.4), w, h)
    c = SC.cast(a, prims, pose, "cam", w, h, pix[None])
    assert c.geom.tolist() == [1]
    ndv = view[2]  # the normal is -z: no light term with or without the shadow
    np.testing.assert_allclose(c.rgb[0], c_box * (0.1 + 0.6 * ndv), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(c.rgb, c.lit_rgb)


# ---- BVH tables ---------------------------------------------------------------------------------
def _tri_hit(tri, o, d):
    """Brute force: does the ray hit any triangle [n, 16] (the kernel's rule: one-sided, t > 1e-4)?"""
    t = tri.astype(np.float64)
    v0, e1, e2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    s = o - v0
    front = np.einsum("ij,ij->i", np.cross(e1, e2), s) > 0
    p = np.cross(d, e2)
    det = np.einsum("ij,ij->i", e1, p)
    ok = front & (np.abs(det) > 1e-300)
    det = np.where(ok, det, 1.0)
    u = np.einsum("ij,ij->i", s, p) / det
    q = np.cross(s, e1)
    v = (q @ d) / det
    tt = np.einsum("ij,ij->i", e2, q) / det
    return ok & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (tt > 1e-4)


def _walk(tables, tri, root, O, D):
    """The kernel's stackless walk in numpy, for rays O, D [n, 3] at once (every ray follows its own
    node sequence; a step advances all rays that are still walking): (any hit [n], nodes visited [n])."""
    nodes = tables["bvh_nodes"]
    skip, word = nodes[:, 3].view(np.int32), nodes[:, 7].view(np.int32)
    lo, hi = nodes[:, 0:3].astype(np.float64), nodes[:, 4:7].astype(np.float64)
    inv = 1.0 / np.where(np.abs(D) < 1e-20, np.copysign(1e-20, D), D)
    n = np.full(len(O), int(root), np.int64)
    hit, visited = np.zeros(len(O), bool), np.zeros(len(O), np.int64)
    while True:
        act = np.nonzero(n >= 0)[0]
        if len(act) == 0:
            return hit, visited
        visited[act] += 1
        na = n[act]
        ta, tb = (lo[na] - O[act]) * inv[act], (hi[na] - O[act]) * inv[act]
        t0, t1 = np.maximum(0.0, np.minimum(ta, tb).max(1)), np.maximum(ta, tb).min(1)
        inside = t0 <= t1
        leaf = inside & (word[na] != 0)
        nxt = np.where(inside & ~leaf, na + 1, skip[na])
        for i in np.nonzero(leaf)[0]:
            first, cnt = int(word[na[i]]) >> 3, int(word[na[i]]) & 7
            if _tri_hit(tri[tables["bvh_tri"][first:first + cnt]], O[act[i]], D[act[i]]).any():
                hit[act[i]] = True
                nxt[i] = -1
        n[act] = nxt


def _check_tables(tables, tri, adr, num):
    from robomanipbaselines_amd.mjcf import bvh

    nodes = tables["bvh_nodes"]
    skip, word = nodes[:, 3].view(np.int32), nodes[:, 7].view(np.int32)
    # every triangle in exactly one leaf
    leaves = np.nonzero(word != 0)[0]
    seen = np.concatenate([tables["bvh_tri"][(w >> 3):(w >> 3) + (w & 7)] for w in word[leaves]])
    assert 1 <= (word[leaves] & 7).min() and (word[leaves] & 7).max() <= bvh.LEAF
    assert np.array_equal(np.sort(seen), np.arange(len(tri))) and len(tables["bvh_tri"]) == len(tri)
    t = tri.astype(np.float64)
    verts = np.stack([t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]], 1)
    for k, root in enumerate(tables["bvh_root"]):
        end = int(tables["bvh_root"][k + 1]) if k + 1 < len(tables["bvh_root"]) else len(nodes)
        # depth-first order: a node's subtree is the nodes up to its skip link (the slot's end for -1)
        stop = np.where(skip[root:end] < 0, end, skip[root:end])
        assert (stop > np.arange(root, end)).all() and (stop <= end).all()
        # the box of every node contains the triangles of every leaf of its subtree [n, stop): checked directly per node: every node of a small slot, the root and 60 random nodes of a large one
        pick = np.arange(root, end) if end - root <= 100 else np.unique(np.r_[root, np.random.default_rng(k).integers(root, end, 60)])
        slot_tris = set(range(int(adr[k]), int(adr[k] + num[k])))
        for n in pick:
            sub = np.arange(n, stop[n - root])
            ws = word[sub][word[sub] != 0]
            ids = np.concatenate([tables["bvh_tri"][(w >> 3):(w >> 3) + (w & 7)] for w in ws])
            assert set(ids.tolist()) <= slot_tris
            v = verts[ids].reshape(-1, 3)
            assert (v.min(0) >= nodes[n, 0:3]).all() and (v.max(0) <= nodes[n, 4:7]).all(), (k, n)
        ids = np.concatenate([tables["bvh_tri"][(w >> 3):(w >> 3) + (w & 7)] for w in word[root:end][word[root:end] != 0]])
        assert set(ids.tolist()) == slot_tris  # the root's subtree is the slot


def test_bvh_of_a_12_triangle_mesh():
    from robomanipbaselines_amd.mjcf import bvh

    s = 0.5  # a cube's 12 triangles, outward winding
    c = np.array([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.array([[c[q[0]], c[q[i]], c[q[i + 1]]] for q in quads for i in (1, 2)])
    a = RC.scene([], tris=tris)[0]
    tri = a["rmesh_tri"]
    n = np.cross(tri[:, 3:6], tri[:, 6:9])
    assert (np.einsum("ij,ij->i", n, tri[:, 0:3] + (tri[:, 3:6] + tri[:, 6:9]) / 3) > 0).all()  # outward
    tables = bvh.build(tri, a["rmesh_tri_adr"], a["rmesh_tri_num"])
    assert len(tables["bvh_nodes"]) == 2 * 3 - 1
    _check_tables(tables, tri, a["rmesh_tri_adr"], a["rmesh_tri_num"])
    rng = np.random.default_rng(3)
    O = rng.uniform(-1.5, 1.5, (500, 3))
    D = np.where((np.arange(500) % 2 == 1)[:, None], rng.uniform(-0.6, 0.6, (500, 3)) - O, rng.normal(size=(500, 3)))
    D /= np.linalg.norm(D, axis=1, keepdims=True)  # (half of the rays aimed at the cube)
    want = np.array([bool(_tri_hit(tri, o, d).any()) for o, d in zip(O, D)])
    assert np.array_equal(_walk(tables, tri, tables["bvh_root"][0], O, D)[0], want) and 100 < want.sum() < 450


def test_bvh_of_the_cable_scene():
    from robomanipbaselines_amd import model as MD
    from robomanipbaselines_amd.mjcf import bvh

    a = MD.load("ur5e_cable")
    tri, adr, num = a["rmesh_tri"], a["rmesh_tri_adr"], a["rmesh_tri_num"]
    tables = bvh.build(tri, adr, num)
    _check_tables(tables, tri, adr, num)
    k = int(np.argmax(num))  # the largest slot: 2,000 random rays, the walk against brute force
    sl = tri[adr[k]:adr[k] + num[k]]
    verts = np.concatenate([sl[:, 0:3], sl[:, 0:3] + sl[:, 3:6], sl[:, 0:3] + sl[:, 6:9]]).astype(np.float64)
    lo, hi = verts.min(0), verts.max(0)
    rng = np.random.default_rng(11)
    O = rng.uniform(lo - 0.05, hi + 0.05, (2000, 3))
    # half of the rays aimed at the mesh, so that many hit it
    D = np.where((np.arange(2000) % 2 == 1)[:, None], verts[rng.integers(len(verts), size=2000)] - O, rng.normal(size=(2000, 3)))
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    got, nv = _walk(tables, tri, tables["bvh_root"][k], O, D)
    want = np.array([bool(_tri_hit(sl, o, d).any()) for o, d in zip(O, D)])
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    hits = int(want.sum())
    print(f"slot {k}: {num[k]} triangles, {hits} of 2000 rays hit, {nv.mean():.0f} nodes per ray")
    assert 400 < hits < 1900


# ---- compiler and assets --------------------------------------------------------------------------
def test_shipped_assets_carry_their_lights():
    from robomanipbaselines_amd import model as MD
    from robomanipbaselines_amd import render as RD

    for name in SHADOW_SCENES + PLAIN_SCENES:
        a = MD.load(name)
        assert a["light_castshadow"].tolist() == [1 if name in SHADOW_SCENES else 0], name
        assert RD.scene_casts_shadows(a) == (name in SHADOW_SCENES)
        # the values equal the shading constants of the kernel
        np.testing.assert_allclose(a["light_dir"], [[0, 0, -1]], atol=1e-12)
        assert a["light_directional"].tolist() == [1]
        np.testing.assert_allclose(a["light_diffuse"], [[RD.LIGHT_DIFFUSE] * 3])
        np.testing.assert_allclose(a["headlight_ambient"], [RD.AMBIENT] * 3)
        np.testing.assert_allclose(a["headlight_diffuse"], [RD.HEADLIGHT_DIFFUSE] * 3)
        np.testing.assert_allclose(a["headlight_specular"], [0.0] * 3)
        np.testing.assert_array_equal(RD.shadow_light(a), [0, 0, 1])


def test_front_end_refuses_other_lights():
    from robomanipbaselines_amd import model as MD
    from robomanipbaselines_amd import render as RD

    a = dict(MD.load("ur5e_cable"))
    for key, value in (("light_dir", np.array([[0.0, 0.6, -0.8]])), ("light_diffuse", np.array([[0.5, 0.5, 0.5]])),
                       ("headlight_diffuse", np.array([0.4, 0.4, 0.4])), ("light_directional", np.array([0], np.int32))):
        b = dict(a)
        b[key] = value
        with pytest.raises(ValueError, match="shadows"):
            RD.shadow_light(b)
    a2 = RC.scene([(0, (0, 0, 0.1), (0, 0, 0), (1, 1, 1))])[0]  # a synthetic scene has no light arrays
    np.testing.assert_array_equal(RD.shadow_light(a2), [0, 0, 1])
    assert not RD.scene_casts_shadows(a2)


_XML = """<mujoco>
  <option integrator="implicitfast"/>
  <default><light castshadow="false" diffuse="0.3 0.3 0.3"/><default class="sun"><light castshadow="true"/></default></default>
  <visual><headlight ambient="0.1 0.1 0.1" diffuse="0.6 0.6 0.6" specular="0 0 0"/></visual>
  <worldbody>
    {world}
    <geom type="plane" size="1 1 0.1"/>
    <body name="b" pos="0 0 1"><joint type="hinge" axis="0 0 1"/><geom type="sphere" size="0.1"/>{body}</body>
  </worldbody>
</mujoco>"""


def _compile_lights(tmp_path, world="", body=""):
    from robomanipbaselines_amd.mjcf import compiler as C

    p = os.path.join(tmp_path, "m.xml")
    with open(p, "w") as f:
        f.write(_XML.format(world=world, body=body))
    return C.light_arrays(C.compile_mjcf(p))


def test_compiler_lights_and_defaults(tmp_path):
    la = _compile_lights(tmp_path, world='<light directional="true" dir="0 0 -2"/><light class="sun" directional="true" '
                                         'dir="0 1 0" diffuse="0.2 0.2 0.2" specular="0.1 0.1 0.1"/>')
    assert la["light_castshadow"].tolist() == [0, 1] and la["light_directional"].tolist() == [1, 1]  # <default> inherited
    np.testing.assert_allclose(la["light_dir"], [[0, 0, -1], [0, 1, 0]])  # normalised
    np.testing.assert_allclose(la["light_diffuse"], [[0.3] * 3, [0.2] * 3])
    np.testing.assert_allclose(la["light_specular"], [[0.3] * 3, [0.1] * 3])  # MuJoCo's default 0.3
    np.testing.assert_allclose(la["headlight_ambient"], [0.1] * 3)
    np.testing.assert_allclose(la["headlight_diffuse"], [0.6] * 3)
    np.testing.assert_allclose(la["headlight_specular"], [0.0] * 3)
    # MuJoCo's defaults without the elements: a light casts shadows; headlight 0.1 / 0.4 / 0.5
    p = os.path.join(tmp_path, "d.xml")
    with open(p, "w") as f:
        f.write('<mujoco><option integrator="implicitfast"/><worldbody><light directional="true"/><geom type="plane" size="1 1 0.1"/></worldbody></mujoco>')
    from robomanipbaselines_amd.mjcf import compiler as C

    la = C.light_arrays(C.compile_mjcf(p))
    assert la["light_castshadow"].tolist() == [1] and la["light_directional"].tolist() == [1]
    np.testing.assert_allclose(la["light_dir"], [[0, 0, -1]])
    np.testing.assert_allclose(la["light_diffuse"], [[0.7] * 3])
    np.testing.assert_allclose(la["headlight_diffuse"], [0.4] * 3)
    np.testing.assert_allclose(la["headlight_specular"], [0.5] * 3)


def test_compiler_refuses_lights_it_cannot_place(tmp_path):
    with pytest.raises(ValueError, match="light"):
        _compile_lights(tmp_path, body='<light directional="true" dir="0 0 -1"/>')  # on a moving body
    with pytest.raises(ValueError, match="light"):
        _compile_lights(tmp_path, world='<light class="sun" directional="false" pos="0 0 3"/>')  # casts, not directional


# ---- guard: the comparison cannot pass vacuously ------------------------------------------------
def test_shadow_comparison_is_not_vacuous():
    """Cable front at 104 x 72, both test poses: the shadow changes more than 3 % of the pixels (above
    the 2 % cap on excused pixels, so a renderer without shadows fails), the flipped cast B sees the
    same geoms as A, and the oracle's own occlusion verdict flips under the comparison's jitter at
    fewer than 0.5 % of the lit pixels (the cap is not used up by the rule's own edge noise)."""
    from robomanipbaselines_amd import model as MD

    arrays = MD.load("ur5e_cable")
    prims = OR.scene_prims(arrays)
    xs, ys = RC.all_pixels(W, H)
    pix = np.stack([xs + 0.5, ys + 0.5], 1)
    jit = RC.jitter(H)
    for e, q in enumerate(RC.asset_qpos(arrays)):
        pose = RC.cpu_pose(arrays, q)
        c = SC.cast(arrays, prims, pose, "front", W, H, pix)
        fl = SC.flipped(pose)
        bg = OR.cast(arrays, prims, fl.gxpos, fl.gxmat, fl.xpos, fl.xquat, "front", W, H, pix)[0]
        assert np.array_equal(bg, c.geom)
        changed = np.abs(OR.to_u8(c.rgb).astype(int) - OR.to_u8(c.lit_rgb).astype(int)).max(1) > RC.RGB_TOL
        lit = np.nonzero((c.geom >= 0) & ~c.occluded)[0][::4]  # (every fourth lit pixel: the share is what is bounded)
        flips = np.zeros(len(lit), bool)
        for dx in (-jit, jit):
            for dy in (-jit, jit):
                jp = pix[lit] + (dx, dy)
                jg, jd, _ = OR.cast(arrays, prims, pose.gxpos, pose.gxmat, pose.xpos, pose.xquat, "front", W, H, jp)
                ok = jg >= 0
                occ = np.zeros(len(lit), bool)
                occ[ok] = SC.occluded_points(arrays, prims, pose, SC.hit_points(arrays, pose, "front", W, H, jp[ok], jd[ok]))
                flips |= occ
        print(f"Cable front env{e}: shadow-changed {int(changed.sum())} of {len(xs)} ({changed.mean():.3%}), "
              f"occluded {int(c.occluded.sum())}, verdict flips among lit {int(flips.sum())} of {len(lit)}")
        assert changed.mean() > 0.03
        assert flips.mean() < 0.005
