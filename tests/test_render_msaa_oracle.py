"""The 4-samples-per-pixel mode, the parts that need no GPU: the guard on what the GPU comparison
(test_render_msaa_gpu.py, tests/msaa_cases.py) may excuse, the sample pattern of the header, and the
plumbing (`--offsamples`, Renderer(samples=...), the compiler's <visual><quality offsamples>).

Measured here (the oracle alone, 104 x 72): share of pixels with any ambiguous sample, Cable front env 0
0.0315 of 7,488, Cable hand env 0 on the (x + y) % 4 == 0 subset 0.0235 of 1,872; the composed 4-sample
frame is more than RGB_TOL from the centre-sample frame on 6-10 % of a frame's pixels."""

import os
import re

import numpy as np
import pytest

import msaa_cases as MC
import render_cases as RC
from oracle import render as OR

W, H = 104, 72
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- guard: what the GPU comparison may excuse ----------------------------------------------------
@pytest.mark.parametrize("cam,subset", [("front", False), ("hand", True)])
def test_any_sample_ambiguous_share_stays_under_the_cap(cam, subset):
    """A later change of frame, jitter or pattern cannot silently widen what the GPU test excuses."""
    from robomanipbaselines_amd import model as MD

    arrays = MD.load("ur5e_cable")
    prims = OR.scene_prims(arrays)
    pose = RC.cpu_pose(arrays, RC.asset_qpos(arrays)[0])
    xs, ys = MC.every_fourth(W, H) if subset else RC.all_pixels(W, H)
    s = MC.cast4(arrays, prims, pose, cam, W, H, xs, ys)
    share = float(MC.any_sample_ambiguous(arrays, prims, pose, cam, W, H, s, np.arange(len(xs))).mean())
    centre = OR.to_u8(OR.cast(arrays, prims, pose.gxpos, pose.gxmat, pose.xpos, pose.xquat, cam, W, H,
                              np.stack([xs + 0.5, ys + 0.5], 1))[2]).astype(int)
    moved = float((np.abs(s.resolved - centre).max(1) > RC.RGB_TOL).mean())
    print(f"Cable {cam} env0: any-sample ambiguous share {share:.4f} of {len(xs)} pixels; the 4-sample frame "
          f"is more than RGB_TOL from the centre-sample frame on {moved:.4f}")
    assert share <= MC.EXCUSED_CAP
    if not subset:
        assert moved > MC.EXCUSED_CAP  # a renderer without the mode cannot pass on excuses


def test_the_pattern_is_the_headers():
    with open(os.path.join(ROOT, "include", "rmbx.h")) as f:
        m = re.search(r"#define RMBX_SAMPLE_PATTERN (.*)", f.read())
    vals = [float(v) for v in re.findall(r"([0-9.]+)f", m.group(1))]
    assert np.array_equal(np.array(vals).reshape(4, 2), np.array(MC.PATTERN))
    # the 4x rotated grid: every row and column of the 4 x 4 sub-pixel grid holds one sample
    p = np.array(MC.PATTERN)
    assert sorted(p[:, 0]) == sorted(p[:, 1]) == [0.125, 0.375, 0.625, 0.875]
    assert np.allclose(p.mean(0), 0.5)


# ---- plumbing --------------------------------------------------------------------------------------
def _parse(argv):
    from robomanipbaselines_amd.common.rollout_base import BatchedRolloutBase

    ro = object.__new__(BatchedRolloutBase)
    ro.setup_args(argv=argv)
    return ro.args


def test_offsamples_flag():
    assert _parse(["--num_envs", "2"]).offsamples == "1"  # the default, lockstep
    assert _parse(["--num_envs", "2", "--num_episodes", "5"]).offsamples == "1"  # and streaming
    for v in ("1", "4", "scene"):
        assert _parse(["--num_envs", "2", "--offsamples", v]).offsamples == v
        assert _parse(["--num_envs", "2", "--num_episodes", "5", "--offsamples", v]).offsamples == v
    with pytest.raises(SystemExit):
        _parse(["--offsamples", "2"])


def test_renderer_and_scene_values():
    from robomanipbaselines_amd import model as MD
    from robomanipbaselines_amd.render import Renderer, samples_of, scene_offsamples

    for bad in (3, 0, 2, 8, "4", True, None):
        with pytest.raises(ValueError, match="samples"):
            Renderer({}, "cpu", samples=bad)  # (refused before anything is built)
    # the scene's value: MuJoCo's default 4 when the arrays carry none (the shipped assets)
    assert scene_offsamples(MD.load("ur5e_cable")) == 4 and scene_offsamples({}) == 4
    assert scene_offsamples({"quality_offsamples": np.int32(1)}) == 1
    assert [samples_of(v) for v in (0, 1, 4)] == [1, 1, 4]
    for bad in (2, 8, 16, -1):
        with pytest.raises(ValueError, match="offsamples"):
            samples_of(scene_offsamples({"quality_offsamples": np.int32(bad)}))


_XML = """<mujoco>
  <option integrator="implicitfast"/>
  {visual}
  <worldbody>
    <light directional="true"/>
    <geom type="plane" size="1 1 0.1"/>
    <body name="b" pos="0 0 1"><joint type="hinge" axis="0 0 1"/><geom type="sphere" size="0.1"/></body>
  </worldbody>
</mujoco>"""


@pytest.mark.parametrize("visual,want", [("", 4), ('<visual><headlight ambient="0.1 0.1 0.1"/></visual>', 4),
                                         ('<visual><quality shadowsize="2048"/></visual>', 4),
                                         ('<visual><quality offsamples="8"/></visual>', 8),
                                         ('<visual><quality offsamples="0"/></visual>', 0),
                                         ('<visual><map znear="0.02"/><quality offsamples="1"/></visual>', 1)])
def test_compiler_reads_offsamples(tmp_path, visual, want):
    from robomanipbaselines_amd.mjcf import compiler as C
    from robomanipbaselines_amd.render import scene_offsamples

    p = os.path.join(tmp_path, "m.xml")
    with open(p, "w") as f:
        f.write(_XML.format(visual=visual))
    M = C.compile_mjcf(p)
    assert M.offsamples == want
    q = C.quality_arrays(M)
    assert int(q["quality_offsamples"]) == want and scene_offsamples(q) == want
