"""bench.py's command line: a plain run is the headline only (--full off by default), and
--dump-outputs writes the rollout's last-step arrays as float32 / float64 .npy files (host logic,
exercised on CPU tensors)."""
import types

import numpy as np
import torch


def test_plain_run_is_the_default():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def _fake_group(n, seed):
    from robomanipbaselines_amd import kernels as K

    g = torch.Generator().manual_seed(seed)
    f64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    eng = types.SimpleNamespace(qpos=f64(n, 5), qvel=f64(n, 4), time=f64(n))
    return types.SimpleNamespace(
        n=n, env=types.SimpleNamespace(engine=eng), obs={"joint_pos": f64(n, 7), "wrench": f64(n, 6)},
        reward=f64(n), policy_action=f64(n, 7), q_cmd=f64(n, 6), grip_cmd=f64(n, 1), sched=K.sched_alloc(n, "cpu"),
        _img=torch.randint(0, 255, (n, 1, 2, 3, 16), generator=g, dtype=torch.uint8))


def test_dump_outputs(tmp_path):
    import bench

    groups = [_fake_group(6, 0), _fake_group(3, 1)]
    shapes = bench.dump_outputs(groups, str(tmp_path / "out"))
    files = {p.name[:-4]: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(files) == set(shapes) and all(list(files[k].shape) == s for k, s in shapes.items())
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    # the groups' envs in env order, f64 kept as f64
    np.testing.assert_array_equal(files["qpos"], torch.cat([g.env.engine.qpos for g in groups]).numpy())
    np.testing.assert_array_equal(files["obs_wrench"], torch.cat([g.obs["wrench"] for g in groups]).numpy())
    assert files["policy_action"].dtype == np.float64 and files["episode_success"].shape == (9,)
    # the frame sample: the same seeded envs of group 0 on every call, as float32
    idx = files["policy_frame_envs"].astype(int)
    assert len(idx) == min(bench.DUMP_FRAME_ENVS, 6) and len(set(idx)) == len(idx)
    assert files["policy_frame"].dtype == np.float32
    np.testing.assert_array_equal(files["policy_frame"], groups[0]._img[idx].numpy().astype(np.float32))
    assert sum(a.nbytes for a in files.values()) <= bench.DUMP_MAX_BYTES
