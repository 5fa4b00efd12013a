"""Shared pieces of the shadow tests (test_render_shadow_oracle.py, test_render_shadow_gpu.py): the
expected frame of a render with shadows=True, composed from the unchanged brute-force oracle
(oracle/render_oracle.c), and render_cases.compare_frame's rule on that composed frame.  Plain
module: importing it needs neither torch nor a GPU.

The rule under test (include/rmbx.h rmbx_scene_tables): a hit pixel is occluded iff the ray from
O = P + 1e-3 L along L (L = world +z, towards the light) meets any drawn surface under the camera
rays' own rules; an occluded pixel loses the light's two terms.  Composed from orc_render_rays:

* A: the ordinary cast;
* B: the same cast of the world turned by F = diag(1, -1, -1) (every frame and the camera
  pre-multiplied by F, a half turn about x): the geometry the camera sees is the same, local texture
  coordinates too, but every normal's world z flips, so wherever A has the light's terms B has not.
  They are non-negative and the clamp is monotone, so the colour without the light is min(A, B) per
  channel -- no normal is needed;
* occlusion: per hit pixel one more cast, from a 2 x 2, 45 degree "camera" at O whose -z axis is L,
  through the image centre (pixel coordinate (1, 1): exactly the axis), znear 1e-4, no materials: a
  hit geom >= 0 means occluded;
* the expected colour is where(occluded, min(A, B), A).  Depth and geom are A's.
"""

import ctypes
from collections import namedtuple

import numpy as np

import render_cases as RC
from oracle import render as OR

F = np.diag([1.0, -1.0, -1.0])
QF = np.array([0.0, 1.0, 0.0, 0.0])  # F as a quaternion
L = np.array([0.0, 0.0, 1.0])
OFFSET, TMIN = 1e-3, 1e-4
R_LIGHT = np.ascontiguousarray(F.reshape(-1))  # a camera frame whose -z axis is L

Shadowed = namedtuple("Shadowed", "geom depth rgb depth2 occluded lit_rgb")
Compared = namedtuple("Compared", "differing ambiguous unexplained og od o8 detail occluded lit8")


def _quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def flipped(pose):
    """The pose of the world turned by F."""
    gm = np.asarray(pose.gxmat, np.float64).reshape(-1, 3, 3)
    return RC.Pose(np.asarray(pose.gxpos, np.float64) @ F.T, (F @ gm).reshape(-1, 9),
                   np.asarray(pose.xpos, np.float64) @ F.T,
                   np.stack([_quat_mul(QF, q) for q in np.asarray(pose.xquat, np.float64)]))


def _prim_array(prims, pose):
    gm_all = np.asarray(pose.gxmat, np.float64).reshape(-1, 9)
    plist = []
    for kind, idx, pr in prims:
        if kind == "geom":
            pos, Rm = np.asarray(pose.gxpos[idx], np.float64), gm_all[idx]
        else:
            pos, Rm = np.asarray(pose.xpos[idx], np.float64), OR._quat2mat(np.asarray(pose.xquat[idx], np.float64)).reshape(-1)
        for i in range(3):
            pr.pos[i] = float(pos[i])
        for i in range(9):
            pr.R[i] = float(Rm[i])
        plist.append(pr)
    return (OR._Prim * len(plist))(*plist)


def occluded_points(arrays, prims, pose, points):
    """Per world point P [n, 3]: does the shadow ray from P + 1e-3 L along L meet a drawn surface?"""
    lib = OR._load()
    parr = _prim_array(prims, pose)
    tri = np.ascontiguousarray(arrays["rmesh_tri"] if "rmesh_tri" in arrays else np.zeros((1, 16), np.float32), np.float32)
    pix = np.array([[1.0, 1.0]])
    geom, depth, rgb, depth2 = np.zeros(1, np.int32), np.zeros(1), np.zeros((1, 3)), np.zeros(1)
    out = np.zeros(len(points), bool)
    for k, P in enumerate(np.asarray(points, np.float64)):
        O = np.ascontiguousarray(P + OFFSET * L)
        lib.orc_render_rays(ctypes.cast(parr, ctypes.c_void_p), len(prims), tri.ctypes.data, R_LIGHT.ctypes.data,
                            O.ctypes.data, 45.0, 2, 2, TMIN, pix.ctypes.data, 1, geom.ctypes.data, depth.ctypes.data,
                            rgb.ctypes.data, depth2.ctypes.data, None)
        out[k] = geom[0] >= 0
    return out


def hit_points(arrays, pose, cam, W, H, pix, depth):
    """The world points of the rays through pix [n, 2] at camera depth `depth` [n]."""
    R, p = OR.camera_pose(arrays, cam, pose.xpos, pose.xquat)
    i = [str(x) for x in arrays["names_cam"]].index(cam)
    t = np.tan(0.5 * float(arrays["cam_fovy"][i]) * np.pi / 180.0)
    pix = np.asarray(pix, np.float64)
    dc = np.stack([(2.0 * pix[:, 0] / W - 1.0) * t * W / H, (1.0 - 2.0 * pix[:, 1] / H) * t, -np.ones(len(pix))], 1)
    return p + np.asarray(depth)[:, None] * (dc @ R.T)


def cast(arrays, prims, pose, cam, W, H, pix):
    """The composed shadowed cast of the rays through pix [n, 2] (module docstring)."""
    og, od, oc, od2 = OR.cast(arrays, prims, pose.gxpos, pose.gxmat, pose.xpos, pose.xquat, cam, W, H, pix, second=True)
    fl = flipped(pose)
    bc = OR.cast(arrays, prims, fl.gxpos, fl.gxmat, fl.xpos, fl.xquat, cam, W, H, pix)[2]
    occ = np.zeros(len(og), bool)
    hit = np.nonzero(og >= 0)[0]
    if len(hit):
        occ[hit] = occluded_points(arrays, prims, pose, hit_points(arrays, pose, cam, W, H, np.asarray(pix)[hit], od[hit]))
    rgb = np.where(occ[:, None], np.minimum(oc, bc), oc)
    return Shadowed(og, od, rgb, od2, occ, oc)


def compare_frame(arrays, prims, pose, cam, W, H, xs, ys, hit, depth, rgb):
    """render_cases.compare_frame's rule with the composed colour in place of the oracle's, for the
    centre ray and the four jittered rays alike: geom, depth and colour on every pixel (xs, ys),
    ambiguity evaluated only where the GPU differs."""
    pix = np.stack([xs + 0.5, ys + 0.5], 1)
    c = cast(arrays, prims, pose, cam, W, H, pix)
    og, od, od2 = c.geom, c.depth, c.depth2
    o8 = OR.to_u8(c.rgb)
    gg, gd, g8 = hit[ys, xs], depth[ys, xs], rgb[ys, xs]
    bad = gg != og
    same = ~bad & (og >= 0)
    bad |= same & (np.abs(gd - od) > RC.DEPTH_RTOL * np.abs(od) + RC.DEPTH_ATOL)
    bad |= np.abs(g8.astype(int) - o8.astype(int)).max(1) > RC.RGB_TOL
    idx = np.nonzero(bad)[0]
    amb = np.zeros(len(xs), bool)
    if len(idx):
        jit = RC.jitter(H)
        tie = (og[idx] >= 0) & (od2[idx] - od[idx] <= RC.DEPTH_RTOL * od[idx] + RC.DEPTH_ATOL)
        off = np.array([[dx, dy] for dx in (-jit, jit) for dy in (-jit, jit)])
        rays = (pix[idx][:, None, :] + off[None]).reshape(-1, 2)
        j = cast(arrays, prims, pose, cam, W, H, rays)
        jg, jd = j.geom.reshape(-1, 4), j.depth.reshape(-1, 4)
        j8 = OR.to_u8(j.rgb).astype(int).reshape(-1, 4, 3)
        spread = ((jg != og[idx][:, None]).any(1)
                  | (np.abs(jd - od[idx][:, None]).max(1) > RC.DEPTH_RTOL * np.abs(od[idx]) + RC.DEPTH_ATOL)
                  | (np.abs(j8 - o8[idx][:, None, :].astype(int)).max((1, 2)) > RC.RGB_TOL))
        amb[idx] = tie | spread
    unexplained = np.nonzero(bad & ~amb)[0]
    detail = [(int(xs[k]), int(ys[k]), int(gg[k]), int(og[k]), float(gd[k]), float(od[k]), g8[k].tolist(),
               o8[k].tolist(), bool(c.occluded[k])) for k in unexplained[:8]]
    return Compared(int(bad.sum()), int(amb.sum()), unexplained, og, od, o8, detail, c.occluded, OR.to_u8(c.lit_rgb))


def check(what, arrays, poses, cam, w, h, frame, cap=RC.AMBIGUOUS_CAP):
    """compare_frame on every pixel of every env: zero unexplained pixels, excused ones within the
    cap; the counts are printed before they are asserted.  frame: (rgb, depth, hit) numpy [n, ...]."""
    rgb, depth, hit = frame
    prims = OR.scene_prims(arrays)
    xs, ys = RC.all_pixels(w, h)
    out = []
    for e, pose in enumerate(poses):
        res = compare_frame(arrays, prims, pose, cam, w, h, xs, ys, hit[e], depth[e], rgb[e])
        changed = int((np.abs(res.o8.astype(int) - res.lit8.astype(int)).max(1) > RC.RGB_TOL).sum())
        print(f"{what} env{e}: differing {res.differing}, ambiguous {res.ambiguous}, unexplained "
              f"{len(res.unexplained)} of {len(xs)}; occluded {int(res.occluded.sum())}, shadow-changed {changed}")
        out.append(res)
    for e, res in enumerate(out):
        assert len(res.unexplained) == 0, (what, e, len(res.unexplained), res.detail)
        assert res.ambiguous <= cap * len(xs), (what, e, res.ambiguous)
    return out


# an oblique world camera for the synthetic scenes: at (0, -1.2, 0.9), turned 53.13 degrees about x, so
# it looks along (0, 0.8, -0.6) at the ground near the origin (the light comes straight down: a
# camera looking along -z would hide every shadow under its occluder)
CAM_POS = (0.0, -1.2, 0.9)
CAM_QUAT = (float(np.cos(0.5 * np.arctan2(0.8, 0.6))), float(np.sin(0.5 * np.arctan2(0.8, 0.6))), 0.0, 0.0)
