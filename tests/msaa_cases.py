"""Shared pieces of the 4-samples-per-pixel tests (test_render_msaa_oracle.py, test_render_msaa_gpu.py):
the expected frame of a render with samples=4, composed from the unchanged brute-force oracle
(oracle/render_oracle.c), and the rule a GPU frame is held to.  Plain module: importing it needs
neither torch nor a GPU.

The rule under test (include/rmbx.h rmbx_scene_tables, "Samples"): sample k of pixel (x, y) is the ray
through (x + sx_k, y + sy_k), PATTERN below; each sample is shaded as a pixel-centre ray through that
coordinate, rounded to 8 bits, and the pixel is (s0 + s1 + s2 + s3 + 2) >> 2 per channel.  Composed:

* per pixel four oracle casts at the sample coordinates (with shadows: shadow_cases.cast, the composed
  shadowed cast), OR.to_u8 per sample, then (sum + 2) // 4;
* a pixel is differing if any channel is off by more than RC.RGB_TOL: each GPU sample is within
  RGB_TOL of the oracle's, so the rounded mean is too;
* a differing pixel is excused only if at least one of its four samples is ambiguous under the
  existing rule (render_cases._ambiguous at that sample's coordinate, with RC.jitter(H)); everything
  else is unexplained.
"""

from collections import namedtuple

import numpy as np

import render_cases as RC
import shadow_cases as SC
from oracle import render as OR

PATTERN = ((0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875))
EXCUSED_CAP = 0.05  # share of a frame's compared pixels that may be excused

Samples = namedtuple("Samples", "pix geom depth s8 depth2 resolved occluded")
Compared = namedtuple("Compared", "differing excused unexplained expected detail")


def every_fourth(W, H):
    """The pixels with (x + y) % 4 == 0: a quarter of the frame, every row and column."""
    xs, ys = RC.all_pixels(W, H)
    keep = (xs + ys) % 4 == 0
    return xs[keep], ys[keep]


def cast4(arrays, prims, pose, cam, W, H, xs, ys, shadows=False):
    """The four sample casts of the pixels (xs, ys): pix [n, 4, 2], geom / depth / depth2 [n, 4], the
    8-bit sample colours s8 [n, 4, 3] and the resolved pixel [n, 3] (ints)."""
    n = len(xs)
    pix = np.stack([np.stack([xs + sx, ys + sy], 1) for sx, sy in PATTERN], 1).astype(np.float64)
    flat = pix.reshape(-1, 2)
    if shadows:
        c = SC.cast(arrays, prims, pose, cam, W, H, flat)
        og, od, oc, od2, occ = c.geom, c.depth, c.rgb, c.depth2, c.occluded.reshape(n, 4)
    else:
        og, od, oc, od2 = OR.cast(arrays, prims, pose.gxpos, pose.gxmat, pose.xpos, pose.xquat, cam, W, H, flat,
                                  second=True)
        occ = np.zeros((n, 4), bool)
    s8 = OR.to_u8(oc).astype(int).reshape(n, 4, 3)
    return Samples(pix, og.reshape(n, 4), od.reshape(n, 4), s8, od2.reshape(n, 4), (s8.sum(1) + 2) // 4, occ)


def _ambiguous_shadowed(arrays, prims, pose, cam, W, H, pix, og, od, o8, od2, idx, jit):
    """render_cases._ambiguous with the composed shadowed cast for the jittered rays (as
    shadow_cases.compare_frame does)."""
    amb = np.zeros(len(idx), bool)
    if len(idx) == 0:
        return amb
    tie = (og[idx] >= 0) & (od2[idx] - od[idx] <= RC.DEPTH_RTOL * od[idx] + RC.DEPTH_ATOL)
    off = np.array([[dx, dy] for dx in (-jit, jit) for dy in (-jit, jit)])
    rays = (pix[idx][:, None, :] + off[None]).reshape(-1, 2)
    j = SC.cast(arrays, prims, pose, cam, W, H, rays)
    jg, jd = j.geom.reshape(-1, 4), j.depth.reshape(-1, 4)
    j8 = OR.to_u8(j.rgb).astype(int).reshape(-1, 4, 3)
    spread = ((jg != og[idx][:, None]).any(1)
              | (np.abs(jd - od[idx][:, None]).max(1) > RC.DEPTH_RTOL * np.abs(od[idx]) + RC.DEPTH_ATOL)
              | (np.abs(j8 - o8[idx][:, None, :].astype(int)).max((1, 2)) > RC.RGB_TOL))
    amb[:] = tie | spread
    return amb


def any_sample_ambiguous(arrays, prims, pose, cam, W, H, s, idx, shadows=False):
    """Of the pixels idx (into the Samples s): which have at least one ambiguous sample."""
    rule = _ambiguous_shadowed if shadows else RC._ambiguous
    amb = np.zeros(len(idx), bool)
    for k in range(4):
        amb |= rule(arrays, prims, pose, cam, W, H, s.pix[:, k], s.geom[:, k], s.depth[:, k],
                    s.s8[:, k].astype(np.uint8), s.depth2[:, k], idx, RC.jitter(H))
    return amb


def ambiguous_share(arrays, prims, pose, cam, W, H, xs, ys):
    """The share of the pixels (xs, ys) with any ambiguous sample, by the oracle alone: what compare
    would excuse wherever the GPU differed."""
    s = cast4(arrays, prims, pose, cam, W, H, xs, ys)
    return float(any_sample_ambiguous(arrays, prims, pose, cam, W, H, s, np.arange(len(xs))).mean())


def compare(arrays, prims, pose, cam, W, H, xs, ys, rgb, shadows=False):
    """One env's GPU colours rgb [H, W, 3] u8 against the composed frame on the pixels (xs, ys)."""
    s = cast4(arrays, prims, pose, cam, W, H, xs, ys, shadows)
    g8 = rgb[ys, xs].astype(int)
    bad = np.abs(g8 - s.resolved).max(1) > RC.RGB_TOL
    idx = np.nonzero(bad)[0]
    amb = np.zeros(len(xs), bool)
    amb[idx] = any_sample_ambiguous(arrays, prims, pose, cam, W, H, s, idx, shadows)
    unexplained = np.nonzero(bad & ~amb)[0]
    detail = [(int(xs[k]), int(ys[k]), g8[k].tolist(), s.resolved[k].tolist(), s.geom[k].tolist())
              for k in unexplained[:8]]
    return Compared(int(bad.sum()), int(amb.sum()), unexplained, s, detail)


def check(what, arrays, poses, cam, W, H, xs, ys, rgb, shadows=False):
    """compare on every env: zero unexplained pixels, at most EXCUSED_CAP of the compared pixels
    excused; the counts are printed before they are asserted.  rgb: numpy [n, H, W, 3]."""
    prims = OR.scene_prims(arrays)
    out = []
    for e, pose in enumerate(poses):
        res = compare(arrays, prims, pose, cam, W, H, xs, ys, rgb[e], shadows)
        centre = OR.to_u8(OR.cast(arrays, prims, pose.gxpos, pose.gxmat, pose.xpos, pose.xquat, cam, W, H,
                                  np.stack([xs + 0.5, ys + 0.5], 1))[2]).astype(int)
        moved = int((np.abs(res.expected.resolved - centre).max(1) > RC.RGB_TOL).sum())
        print(f"{what} env{e}: differing {res.differing}, excused {res.excused}, unexplained {len(res.unexplained)} "
              f"of {len(xs)}; expected pixels more than RGB_TOL from the oracle's unshadowed centre sample {moved}")
        out.append(res)
    for e, res in enumerate(out):
        assert len(res.unexplained) == 0, (what, e, len(res.unexplained), res.detail)
        assert res.excused <= EXCUSED_CAP * len(xs), (what, e, res.excused)
    return out
