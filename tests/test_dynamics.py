"""--dynamics on the host (common/dynamics.py; the rule: include/rmbx.h, rmbx_dynamics_draw): the
parser, the numpy restatement against an independent scalar one, which bodies count as objects, and the
power of the GPU parity tests -- each factor alone moves the CPU oracle well clear of the nominal one."""

import numpy as np
import pytest

import dynamics_cases as DC
from robomanipbaselines_amd import model as MD
from robomanipbaselines_amd.common import dynamics as DY
from robomanipbaselines_amd.envs.ur5e_base import ARM_JOINTS


# -- parser ---------------------------------------------------------------------------------------------
def test_parser_reads_the_four_keys_as_f32():
    s = DY.parse_spec(["friction=0.3", "damping=0.5", "mass=0.25", "gain=0.1"])
    assert s.as_dict() == {"friction": DC.f32(0.3), "damping": 0.5, "mass": 0.25, "gain": DC.f32(0.1)}
    assert list(s.as_dict()) == ["friction", "damping", "mass", "gain"] == list(DY.KEYS)
    assert str(s) == "friction=0.3 damping=0.5 mass=0.25 gain=0.1"
    assert DY.spec_from_dict(s.as_dict()) == s
    assert DY.parse_spec("mass=0.5") == DY.DynamicsSpec(mass=0.5)
    assert s.strengths().dtype == np.float32 and s.strengths().tolist() == [np.float32(0.3), 0.5, 0.25, np.float32(0.1)]


@pytest.mark.parametrize("items", [
    ["stiffness=0.1"], ["Friction=0.1"], ["=0.1"],  # unknown key
    ["mass=0.1", "mass=0.2"], ["gain=0", "friction=0.1", "gain=0"],  # repeated key
    ["mass"], ["mass="], ["mass=abc"], ["mass=0.1x"], ["mass 0.1"], ["mass=0,1"],  # malformed
    ["mass=1"], ["mass=1.0"], ["mass=0.99999999"], ["mass=-0.1"], ["mass=-1e-30"], ["mass=2"],  # outside [0, 1)
    ["mass=inf"], ["mass=nan"], ["mass=1e40"],
])
def test_parser_rejects(items):
    with pytest.raises(ValueError, match="--dynamics"):
        DY.parse_spec(items)


def test_parser_keeps_the_largest_f32_below_one():
    below = float(np.nextafter(np.float32(1), np.float32(0)))
    assert DY.parse_spec([f"gain={below!r}"]).gain == below
    assert DY.parse_spec(["gain=0"]).gain == 0.0 and DY.parse_spec(["gain=-0.0"]).gain == 0.0


# -- the restatement ----------------------------------------------------------------------------------------
def test_zero_spec_gives_exactly_one():
    s = DY.scales(DC.SEED, DC.EPISODES, DY.DynamicsSpec())
    assert s.dtype == np.float64 and s.shape == (len(DC.EPISODES), 4)
    assert s.tobytes() == np.ones((len(DC.EPISODES), 4)).tobytes()
    one = DY.scales(DC.SEED, DC.EPISODES, DY.DynamicsSpec(mass=0.5))
    assert (one[:, [0, 1, 3]] == 1.0).all() and (one[:, 2] != 1.0).all()


@pytest.mark.parametrize("seed", [0, 3, DC.SEED, 2**64 - 1])
def test_scales_match_an_independent_restatement(seed):
    spec = DY.parse_spec([f"{k}={v}" for k, v in DC.STRENGTHS.items()])
    got = DY.scales(seed, DC.EPISODES, spec)
    want = np.array([DC.scale_row(seed, e, spec.strengths()) for e in DC.EPISODES])
    assert got.tobytes() == want.tobytes()
    # a component's draw does not depend on the other strengths
    alone = DY.scales(seed, DC.EPISODES, DY.DynamicsSpec(damping=spec.damping))
    assert alone[:, 1].tobytes() == got[:, 1].tobytes()
    # episode -1 is counter word 0xffffffff, no special case
    assert DY.scales(seed, [-1], spec).tobytes() == DY.scales(seed, [2**32 - 1], spec).tobytes()


def test_scales_lie_inside_their_interval_and_fill_it():
    spec = DY.parse_spec([f"{k}={v}" for k, v in DC.STRENGTHS.items()])
    ep = np.arange(6000)
    s = DY.scales(7, ep, spec)
    S = spec.strengths().astype(np.float64)
    assert np.isfinite(s).all() and (s > 0).all()
    assert (s > 1.0 - S).all() and (s < 1.0 + S).all()
    # uniform over the interval: both outer tenths are reached, the mean is near 1, columns differ
    assert (s.min(0) < 1.0 - 0.9 * S).all() and (s.max(0) > 1.0 + 0.9 * S).all()
    assert (np.abs(s.mean(0) - 1.0) < 0.05 * S).all()
    assert abs(np.corrcoef(s[:, 0], s[:, 1])[0, 1]) < 0.05
    # a function of (seed, episode) alone: any order, any subset
    perm = np.random.default_rng(0).permutation(len(ep))
    assert DY.scales(7, ep[perm], spec).tobytes() == s[perm].tobytes()
    assert DY.scales(8, ep, spec).tobytes() != s.tobytes()
    strongest = DY.DynamicsSpec(*[float(np.nextafter(np.float32(1), np.float32(0)))] * 4)
    s = DY.scales(7, ep, strongest)
    assert (s > 0).all() and (s < 2).all()


# -- object bodies --------------------------------------------------------------------------------------------
def test_object_bodies_of_the_cable_scene():
    arrays = MD.load("ur5e_cable")
    g = DY.object_bodies(arrays, ARM_JOINTS[0])
    names = [str(n) for n in arrays["names_body"]]
    assert g.dtype == np.uint8 and g.shape == (len(names),) == (55,) and int(g.sum()) == 30 and g[0] == 0
    objects = [n for n, v in zip(names, g) if v]
    assert objects == ["table", "stand", "cable"] + [f"cable_B{i}" for i in range(25)] + ["cable_end", "poles"]
    # the arm's whole subtree -- links, gripper linkage, camera mounts -- is outside
    jb = int(arrays["jnt_body"][names_index(arrays, ARM_JOINTS[0])])
    arm_root = arrays["body_rootid"][jb]
    for b in range(1, len(names)):
        assert bool(g[b]) == (arrays["body_rootid"][b] != arm_root)
    for j in ARM_JOINTS:
        assert g[int(arrays["jnt_body"][names_index(arrays, j)])] == 0
    # the dofs that scale are the cable's
    assert int(g[np.asarray(arrays["dof_body"])].sum()) > 40
    with pytest.raises(ValueError, match="no joint"):
        DY.object_bodies(arrays, "no_such_joint")


def names_index(arrays, joint):
    return [str(n) for n in arrays["names_jnt"]].index(joint)


def test_object_bodies_of_the_door_scene_hold_none_of_the_arm():
    arrays = MD.load("ur5e_door")
    g = DY.object_bodies(arrays, ARM_JOINTS[0])
    parent = np.asarray(arrays["body_parent"])
    base = int(arrays["jnt_body"][names_index(arrays, ARM_JOINTS[0])])
    while parent[base] != 0:  # the root of the arm's tree
        base = int(parent[base])
    in_arm = np.zeros(len(g), bool)
    for b in range(1, len(g)):  # bodies are in DFS preorder: a parent precedes its children
        in_arm[b] = b == base or in_arm[parent[b]]
    assert in_arm.sum() >= 7 and g[0] == 0
    assert not g[in_arm].any() and g[1:][~in_arm[1:]].all() and g.sum() >= 1


# -- scaled arrays -------------------------------------------------------------------------------------------
def test_scaled_arrays_touch_what_the_rule_names_and_nothing_else():
    arrays, group = DC.cable()
    a = DY.scaled_arrays(arrays, DC.ROWS[5], group)
    s0, s1, s2, s3 = DC.ROWS[5]
    obj = group.astype(bool)
    changed = {k for k in arrays if isinstance(arrays[k], np.ndarray) and arrays[k].dtype == np.float64
               and not np.array_equal(arrays[k], a[k])}
    assert changed == {"pair_friction", "dof_damping", "body_mass", "body_inertia", "act_gain", "act_bias"}
    fr, fr0 = np.reshape(a["pair_friction"], (-1, 3)), np.reshape(arrays["pair_friction"], (-1, 3))
    assert np.array_equal(fr[:, 0], fr0[:, 0] * s0) and np.array_equal(fr[:, 1:], fr0[:, 1:])
    assert np.array_equal(a["body_mass"][obj], arrays["body_mass"][obj] * s2)
    assert np.array_equal(a["body_mass"][~obj], arrays["body_mass"][~obj])
    I, I0 = np.reshape(a["body_inertia"], (55, -1)), np.reshape(arrays["body_inertia"], (55, -1))
    assert np.array_equal(I[obj], I0[obj] * s2) and np.array_equal(I[~obj], I0[~obj])
    dobj = obj[np.asarray(arrays["dof_body"])]
    assert np.array_equal(a["dof_damping"][dobj], arrays["dof_damping"][dobj] * s1)
    assert np.array_equal(a["dof_damping"][~dobj], arrays["dof_damping"][~dobj])
    b, b0 = np.reshape(a["act_bias"], (-1, 3)), np.reshape(arrays["act_bias"], (-1, 3))
    assert np.array_equal(b[:, 0], b0[:, 0]) and np.array_equal(b[:, 1:], b0[:, 1:] * s3)
    assert np.array_equal(a["act_gain"], arrays["act_gain"] * s3)
    for k in ("body_invweight0", "dof_invweight0"):
        assert a[k] is arrays[k]
    # a row of ones changes no bit
    one = DY.scaled_arrays(arrays, DC.ROWS[0], group)
    for k in changed:
        assert np.asarray(one[k]).tobytes() == np.asarray(arrays[k]).tobytes()


# -- test power -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row, name", [((0.5, 1, 1, 1), "friction 0.5"), ((1, 2, 1, 1), "damping 2"),
                                       ((1, 1, 2, 1), "mass 2"), ((1, 1, 1, 0.8), "gain 0.8")])
def test_each_factor_alone_moves_the_oracle(row, name):
    """From the nominal start under ctrl = INIT + 0.05, gripper 200, each factor alone moves max |qpos|
    from the nominal oracle by more than 1e-4 within 5 env-steps (measured at step 5: 3.8e-3, 3.1e-2,
    4.2e-2, 7.7e-3): a GPU parity test at 1e-9 cannot pass with a scale ignored."""
    arrays, _ = DC.cable()
    qpos, ctrl = DC.start_state(arrays, 0.05, 200.0)
    envs = [DC.oracle_for(DC.ROWS[0]), DC.oracle_for(np.array(row, dtype=np.float64))]
    for o in envs:
        o.set_state(0.0, qpos, np.zeros(o.nv), np.zeros(o.nv), ctrl)
    worst = 0.0
    for _ in range(5):
        for o in envs:
            assert o.step(8) == 0
        worst = max(worst, float(np.abs(envs[0].state()[1] - envs[1].state()[1]).max()))
    print(f"\n{name}: max |d qpos| from the nominal oracle within 5 env-steps {worst:.2e}")
    assert np.isfinite(worst) and worst > 1e-4
