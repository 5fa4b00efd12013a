"""MujocoUR5eRing on the batched kernels (envs/mujoco/ur5e/MujocoUR5eRingEnv.py):
the `<composite type="loop">` ring expanded by the MJCF compiler (a closed 11-element polygon whose
connect equality is satisfied at qpos0), the scene hanging the ring on its hooks in the oracle,
the engine stepping it in agreement with the oracle, rmbx_ring_reward bit-exact against the
reference's _get_reward golden vectors (matplotlib Path.contains_point semantics, NaN subpaths),
the hook reach targets of OperationMujocoUR5eRing, and the AutoEval command line."""

import os

import numpy as np
import pytest

from conftest import GOLDEN
from robomanipbaselines_amd import model as MD

DEV = "cuda:0"


@pytest.fixture(scope="module")
def arrays():
    return MD.load("ur5e_ring")


def _init_state(arrays):
    from robomanipbaselines_amd.envs.ur5e_ring import RING_INIT_QPOS

    q = arrays["qpos0"].copy()
    q[:14] = RING_INIT_QPOS
    return q, np.r_[RING_INIT_QPOS[:6], 0.0]


def test_loop_composite_closes_at_qpos0(arrays):
    from oracle.dyn import OracleEnv

    names = [str(x) for x in arrays["names_body"]]
    ring = [i for i, n in enumerate(names) if n.startswith("ring_B")]
    assert [names[i] for i in ring] == [f"ring_B{i}" for i in range(11)]
    # the connect equality closing the loop holds at qpos0: both anchors at the same world point
    e = [k for k in range(len(arrays["eq_type"])) if arrays["eq_type"][k] == 0
         and names[arrays["eq_obj1"][k]] == "ring_B0"]
    assert len(e) == 1
    o = OracleEnv(arrays)
    q, ctrl = _init_state(arrays)
    o.set_state(0.0, q, np.zeros(o.nv), np.zeros(o.nv), ctrl)
    o.forward()
    x, quat = o.xpos()
    d = arrays["eq_data"].reshape(len(arrays["eq_type"]), -1)[e[0]]

    def world(b, p):
        from oracle.glue import quat2mat

        return x[b] + quat2mat(quat[b]) @ p

    b1, b2 = int(arrays["eq_obj1"][e[0]]), int(arrays["eq_obj2"][e[0]])
    np.testing.assert_allclose(world(b1, d[:3]), world(b2, d[3:6]), rtol=0, atol=1e-12)
    # 11 elements, 2 hinges each except the host, on a ring body with a free joint: nv = 14 + 6 + 20
    assert int(arrays["_nv"]) == 40


def test_ring_hangs_on_the_hooks_in_the_oracle(arrays):
    from oracle.dyn import OracleEnv

    names = [str(x) for x in arrays["names_body"]]
    ring = [i for i, n in enumerate(names) if n.startswith("ring_B")]
    o = OracleEnv(arrays)
    q, ctrl = _init_state(arrays)
    o.set_state(0.0, q, np.zeros(o.nv), np.zeros(o.nv), ctrl)
    for _ in range(150):
        assert o.step(8) == 0
    x, _ = o.xpos()
    _, qp, v, _ = o.state()
    assert np.isfinite(qp).all() and np.abs(v[14:]).max() < 0.1
    hooks_top = 0.795 + 0.25 + 0.01
    top = x[ring][:, 2].max()
    assert hooks_top < top < hooks_top + 0.03, top  # resting on the hooks, not fallen
    assert x[ring][:, 2].min() > 0.82  # above the table


@pytest.mark.gpu
def test_ring_engine_matches_oracle(arrays):
    """The scene with its task contacts live, contact by contact: tests/test_contacts_gpu.py."""
    import torch

    from oracle.dyn import OracleEnv
    from robomanipbaselines_amd.engine import PhysicsEngine

    rng = np.random.default_rng(11)
    states = []
    for i in range(4):
        o = OracleEnv(arrays)
        q, ctrl = _init_state(arrays)
        ctrl = ctrl + np.r_[rng.normal(0, 0.05, 6), rng.uniform(0, 255)]
        o.set_state(0.0, q, np.zeros(o.nv), np.zeros(o.nv), ctrl)
        for _ in range((0, 10, 30, 60)[i]):
            o.step(8)
        states.append((*o.state(), ctrl))
    eng = PhysicsEngine(arrays, 4, DEV)
    eng.time.copy_(torch.tensor([s[0] for s in states], dtype=torch.float64))
    for k, name in ((1, "qpos"), (2, "qvel"), (3, "qacc_ws"), (4, "ctrl")):
        getattr(eng, name).copy_(torch.tensor(np.array([s[k] for s in states])))
    eng.step(8)
    torch.cuda.synchronize()
    qp1 = eng.qpos.cpu().numpy()
    for _ in range(24):
        eng.step(8)
    qp25 = eng.qpos.cpu().numpy()
    assert int(eng.stats[:, 3].sum()) == 0
    for i, (t, qp, qv, qa, c) in enumerate(states):
        o = OracleEnv(arrays)
        o.set_state(t, qp, qv, qa, c)
        o.step(8)
        np.testing.assert_allclose(qp1[i], o.state()[1], rtol=0, atol=1e-8)
        for _ in range(24):
            o.step(8)
        np.testing.assert_allclose(qp25[i], o.state()[1], rtol=0, atol=1e-4)


@pytest.mark.gpu
def test_ring_reward_matches_golden():
    import torch

    from robomanipbaselines_amd import kernels as K

    d = np.load(os.path.join(GOLDEN, "reward_ring.npz"))
    ring = torch.from_numpy(d["ring"]).to(DEV)
    pole = torch.from_numpy(d["pole"]).to(DEV)
    r = K.ring_reward(ring, pole).cpu().numpy()
    np.testing.assert_array_equal(r, d["reward"])


@pytest.mark.gpu
def test_ring_world_placement_and_reward():
    import torch

    from robomanipbaselines_amd.envs.ur5e_ring import POLE_POS_OFFSETS, BatchedMujocoUR5eRingEnv

    env = BatchedMujocoUR5eRingEnv(6, DEV, world_random_scale=[0.01, 0.01, 0.0])
    env.modify_world(world_idx=np.arange(6))
    env.reset()
    pole = env.engine.xpos[:, env._pole].cpu().numpy()
    base = env.original_pole_pos + POLE_POS_OFFSETS
    assert np.all(np.abs(pole[:, :2] - base[:, :2]) <= 0.01 + 1e-12)
    np.testing.assert_allclose(pole[:, 2], base[:, 2], rtol=0, atol=1e-12)
    assert (env._get_reward().cpu().numpy() == 0).all()  # the ring starts on the hooks
    # the env wires the ring bodies (in body order) and the pole into the kernel: a horizontal
    # ring of radius 6 cm around each env's pole, 3 cm above its base, succeeds; one shifted
    # 10 cm sideways, or lifted above pole z + 0.08, does not
    th = torch.linspace(0, 2 * np.pi, 12, dtype=torch.float64, device=DEV)[:11]
    circle = torch.stack([0.06 * torch.cos(th), 0.06 * torch.sin(th), torch.zeros_like(th)], 1)
    pole_t = env.engine.xpos[:, env._pole].clone()
    r0, r1 = env._ring_bodies[0], env._ring_bodies[-1] + 1
    env.engine.xpos[:, r0:r1] = pole_t[:, None] + circle[None] + torch.tensor([0, 0, 0.03], dtype=torch.float64,
                                                                                device=DEV)
    assert (env._get_reward().cpu().numpy() == 1).all()
    env.engine.xpos[:, r0:r1, 1] += 0.1
    assert (env._get_reward().cpu().numpy() == 0).all()
    env.engine.xpos[:, r0:r1, 1] -= 0.1
    env.engine.xpos[:, r0:r1, 2] += 0.06
    assert (env._get_reward().cpu().numpy() == 0).all()


@pytest.mark.gpu
def test_ring_reach_targets_follow_the_hooks(arrays):
    import torch

    from oracle.dyn import OracleEnv
    from robomanipbaselines_amd.envs.operation.OperationMujocoUR5eRing import HAND_R, OperationMujocoUR5eRing
    from robomanipbaselines_amd.policy.mlp.rollout_mlp import RolloutMlp

    class Rollout(OperationMujocoUR5eRing, RolloutMlp):
        pass

    ro = Rollout(argv=["--num_envs", "3", "--device", DEV, "--world_idx_list", "0", "1", "2"])
    targets = []
    orig = [ph.target for ph in ro.pre_phases]
    for ph, f in zip(ro.pre_phases, orig):
        if f is not None:
            ph.target = (lambda r, _f=f: targets.append(tuple(t.cpu().numpy().copy() for t in _f(r))) or
                         tuple(torch.tensor(t, device=DEV) for t in targets[-1]))
    ro.reset()
    while ro.phase_idx < len(ro.pre_durations):
        ro.step_once()
    assert len(targets) == 2
    o = OracleEnv(arrays)
    o.forward()
    gx, _ = o.geom_frames()
    gn = [str(x) for x in arrays["names_geom"]]
    mid = 0.5 * (gx[gn.index("fook1")] + gx[gn.index("fook2")])
    for (R, p), off in zip(targets, ([-0.15, 0.05, -0.05], [-0.1, 0.05, -0.05])):
        np.testing.assert_array_equal(R, np.tile(HAND_R.reshape(9), (3, 1)))
        np.testing.assert_allclose(p, np.tile(mid + off, (3, 1)), rtol=0, atol=1e-12)
    assert torch.isfinite(ro.env.engine.qpos).all()


@pytest.mark.gpu
def test_ring_autoeval_command_line(tmp_path):
    import yaml

    from robomanipbaselines_amd.bin.Rollout import main

    res = os.path.join(tmp_path, "result.yaml")
    ro = main(["Mlp", "MujocoUR5eRing", "--auto_exit", "--no_plot", "--no_render", "--world_idx_list", "0", "5",
               "--result_filename", res, "--max_duration", "1.0"])
    with open(res) as f:
        data = yaml.safe_load(f)
    assert len(data["success"]) == 2
    assert np.isfinite(ro.env.engine.qpos.cpu().numpy()).all()
