"""--episode_metrics without a device: the numpy model of rmbx_episode_metrics against a hand-worked
episode, the flag, the result / YAML form, the Wilson interval and the summary, the multi-GPU
gather (gloo, two ranks) and the C entry point's argument checks."""

import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

import metrics_cases as MC
from robomanipbaselines_amd import _native as N
from robomanipbaselines_amd.common import episode_metrics as EM
from robomanipbaselines_amd.distributed import gather_table, shard_range


# -- the model, by hand ---------------------------------------------------------------------------------
def _one_slot_call(phase, f, t, v, u, q, p, reward, bad=0):
    """A call for one slot with the arm at qpos / qvel / ctrl addresses 0..5."""
    sched = np.zeros(1, dtype=N.SCHED_DTYPE)
    sched["phase"] = phase
    pad = lambda x: np.array([list(x) + [0.0] * (6 - len(x))], np.float64)  # noqa: E731
    return {"sched": sched, "active": None, "slot_episode": None, "bad_resets": np.array([bad], np.int32),
            "reward": np.array([reward], np.float64), "qpos": pad(q), "qvel": pad(v), "ctrl": pad(u),
            "sensordata": np.array([list(f) + list(t)], np.float64), "ee": np.array([p], np.float64)}


def test_model_reproduces_a_hand_worked_episode():
    """Four counted steps after one step of a pre-motion phase, then a bad-state reset.
      k  force      torque   max|v|  u          q                  p          reward
      1  (3,4,0)    (0,0,2)  0.5     (1,0..)    (0.5,0..)          (0,0,0)    0
      2  (NaN,1,1)  (1,2,2)  0.25    (2,0..)    (1.5,0,0,0,0,-.25) (3,4,0)    0
      3  (0,0,6)    (0,0,0)  2.0     (4,1,0..)  (1.5,1,0,0,0,-.25) (3,4,12)   1
      4  (1,0,0)    (0,0,0)  0       (4,1,0..)  (4,1,0..)          (3,4,12)   1
    peaks: force max(5, -, 6, 1) = 6 (the NaN row is ignored); torque max(2, 3, 0, 0) = 3; speed 2;
    tracking error max(0.5, 0.5, 2.5, 0) = 2.5.  ee_path = 5 + 12 + 0 = 17 (k = 1 seeds only).
    joint_path = (1 + .25) + 1 + (2.5 + 0 + .25) = 5.  cmd_roughness starts at k = 3:
    k = 3: (4 - 2*2 + 1)^2 + (1 - 0 + 0)^2 = 2;  k = 4: (4 - 8 + 2)^2 + (1 - 2 + 0)^2 = 5;  total 7."""
    kw = dict(n_pre=2, episode_base=40, arm_qadr=range(6), arm_dof=range(6))
    table, hist = MC.empty_table(1), np.zeros((1, MC.HIST))
    nan = float("nan")
    # a step of the last pre-motion phase: not the policy's
    table, hist, counted = MC.metrics_model(table, hist, _one_slot_call(
        1, (9, 9, 9), (9, 9, 9), (9,), (9,), (0,), (7, 7, 7), 1.0), **kw)
    assert not counted[0] and table.tobytes() == MC.empty_table(1).tobytes() and not hist.any()
    steps = [((3, 4, 0), (0, 0, 2), (0.5,), (1,), (0.5,), (0, 0, 0), 0.0),
             ((nan, 1, 1), (1, 2, 2), (0, -0.25), (2,), (1.5, 0, 0, 0, 0, -0.25), (3, 4, 0), 0.0),
             ((0, 0, 6), (0, 0, 0), (0, 0, 2.0), (4, 1), (1.5, 1, 0, 0, 0, -0.25), (3, 4, 12), 1.0),
             ((1, 0, 0), (0, 0, 0), (0,), (4, 1), (4, 1), (3, 4, 12), 1.0)]
    for k, (f, t, v, u, q, p, rew) in enumerate(steps, 1):
        table, hist, counted = MC.metrics_model(table, hist, _one_slot_call(2, f, t, v, u, q, p, rew), **kw)
        assert counted[0] and table["steps"][0] == k
        if k == 1:  # the first step seeds the history and adds to no sum
            assert table["ee_path"][0] == table["joint_path"][0] == table["cmd_roughness"][0] == 0.0
            assert hist[0].tolist() == [0, 0, 0, 0.5, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
        if k == 2:  # roughness needs three commands
            assert table["cmd_roughness"][0] == 0.0 and table["ee_path"][0] == 5.0
            assert table["peak_force"][0] == 5.0  # the NaN force row left the peak alone
    want = {"episode": 40, "steps": 4, "first_success_step": 3, "flags": 0, "peak_force": 6.0, "peak_torque": 3.0,
            "peak_joint_speed": 2.0, "peak_tracking_error": 2.5, "ee_path": 17.0, "joint_path": 5.0,
            "cmd_roughness": 7.0}
    assert {k: table[k][0].item() for k in want} == want
    # the divergence guard: nothing accumulates, the row is flagged
    before = table.copy()
    table, hist2, counted = MC.metrics_model(table, hist, _one_slot_call(
        2, (99, 0, 0), (0, 0, 0), (9,), (9,), (0,), (9, 9, 9), 1.0, bad=1), **kw)
    assert counted[0] and table["flags"][0] == 1 and hist2.tobytes() == hist.tobytes()
    before["flags"] = 1
    assert table.tobytes() == before.tobytes()
    # ... and an empty row stays empty, unflagged
    empty, _, _ = MC.metrics_model(MC.empty_table(1), np.zeros((1, MC.HIST)), _one_slot_call(
        2, (1, 0, 0), (0, 0, 0), (1,), (1,), (0,), (1, 1, 1), 1.0, bad=2), **kw)
    assert empty.tobytes() == MC.empty_table(1).tobytes()


def test_model_covers_every_slot_kind_of_the_synthetic_calls():
    """The generator of the GPU test does produce the cases it names."""
    for addressed in (True, False):
        table, hist = MC.empty_table(MC.N_EPISODES), np.zeros((257, MC.HIST))
        for call in MC.make_calls(257, addressed):
            table, hist, _ = MC.metrics_model(table, hist, call, episode_base=MC.EPISODE_BASE)
        assert np.isfinite(table["peak_force"][0]) and table["peak_force"][0] > 0  # despite the NaN row
        if addressed:
            # rows: counted, inactive, guard after 3 steps, the slot that changed episode (3 + 4), after
            # two pre-phase calls, done, bad from the start (empty, unflagged), the second block
            assert table["steps"].tolist() == [7, 0, 3, 3, 4, 5, 0, 0, 7]
        else:  # row = slot: ..., pre-phase, done, counted, counted, past RolloutPhase
            assert table["steps"].tolist() == [7, 0, 3, 7, 5, 0, 7, 7, 0]
        assert table["flags"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0]
        assert (table["episode"][table["steps"] > 0] - MC.EPISODE_BASE == np.nonzero(table["steps"] > 0)[0]).all()


# -- the flag ---------------------------------------------------------------------------------------------
def _parse(argv):
    from robomanipbaselines_amd.common.rollout_base import BatchedRolloutBase
    from robomanipbaselines_amd.policy.mlp.rollout_mlp import RolloutMlp

    ro = RolloutMlp.__new__(RolloutMlp)  # the parser alone: no env, no device
    BatchedRolloutBase.setup_args(ro, argv=argv)
    return ro.args


def test_flag_parsing_and_the_off_path():
    assert _parse([]).episode_metrics is False  # off by default
    assert _parse(["--episode_metrics", "--num_envs", "2"]).episode_metrics is True
    assert _parse(["--episode_metrics", "--num_episodes", "5", "--num_envs", "2"]).episode_metrics is True


def _finished_rollout(n, flag, tmp_path=None):
    """BatchedRolloutBase.finish() of a lockstep run that has ended, on the host: the schedule and,
    with the flag, an accumulator whose table() is a fixed array."""
    import types

    from robomanipbaselines_amd.common.rollout_base import BatchedRolloutBase

    g = np.arange(n)
    rec = np.zeros(n, dtype=N.SCHED_DTYPE)
    rec["success"], rec["result_reward"], rec["duration"] = g % 2 == 0, (g % 2 == 0) * 1.0, 0.032 * (g + 5)
    ro = object.__new__(BatchedRolloutBase)
    ro.device, ro.n = torch.device("cpu"), n
    ro.sched = torch.from_numpy(rec.view(np.uint8).reshape(n, N.SCHED_DTYPE.itemsize).copy())
    ro.result = {k: [] for k in ("success", "reward", "duration")}
    ro.inference_duration_list, ro._infer_events = [], []
    ro.world_idx = g % 3
    ro.env = types.SimpleNamespace(frame_skip=8, sim_timestep=0.004)
    ro.args = types.SimpleNamespace(save_last_image=False, env_offset=0, episode_metrics=flag,
                                    result_filename=None if tmp_path is None else str(tmp_path / "r.yaml"))
    if flag:
        ro._metrics = types.SimpleNamespace(table=lambda: _fixed_table(n))
    return ro


def _fixed_table(n, base=0):
    t = np.zeros(n, dtype=N.METRICS_DTYPE)
    g = base + np.arange(n)
    t["episode"], t["steps"] = g, 10 + g
    t["first_success_step"] = np.where(g % 2 == 0, 3 + g, 0)
    t["flags"] = g % 4 == 3
    for i, f in enumerate(EM.F64_FIELDS):
        t[f] = (g + 1) * (i + 1) / 7.0
    return t


def test_without_the_flag_there_is_no_accumulator_and_no_extra_key(capsys):
    ro = _finished_rollout(4, False)
    ro.finish()
    assert getattr(ro, "_metrics", None) is None and not hasattr(ro, "episode_metrics")
    assert set(ro.result) == {"success", "reward", "duration"}
    out = capsys.readouterr().out
    assert "Wilson" not in out and "Episode metrics" not in out


def test_result_yaml_round_trip(tmp_path, capsys):
    n = 5
    ro = _finished_rollout(n, True, tmp_path)
    ro.finish()
    out = capsys.readouterr().out
    with open(tmp_path / "r.yaml") as f:
        data = yaml.safe_load(f)
    assert set(data) == {"success", "reward", "duration", "metrics"}
    m = data["metrics"]
    assert set(m) == set(EM.RESULT_KEYS) and "episode" not in m and len(m) == 11
    assert all(len(v) == n == len(data["success"]) for v in m.values())
    t = _fixed_table(n)
    for f in EM.INT_FIELDS:
        assert m[f] == t[f].tolist() and all(isinstance(x, int) for x in m[f])
    for f in EM.F64_FIELDS:
        assert m[f] == t[f].tolist()  # f64 survives the YAML round trip
    assert m["first_success_time"] == [float(s) * (8 * 0.004) for s in t["first_success_step"]]
    assert ro.episode_metrics.tobytes() == t.tobytes()
    # the summary follows the existing statistics
    assert out.index("Statistics on policy inference") < out.index("Episode metrics")
    assert "Wilson 95% interval" in out and "Success per world index | 0: 1/2, 1: 1/2, 2: 1/1" in out
    for f in ("steps", "first_success_time") + EM.F64_FIELDS:
        assert f"  - {f}" in out


# -- Wilson interval and summary ----------------------------------------------------------------------------
def test_wilson_interval_known_values():
    lo, hi = EM.wilson_interval(0, 10)
    assert lo == 0.0 and abs(hi - MC.WILSON_0_OF_10[1]) <= 1e-12
    assert abs(hi - 0.27753) <= 1e-5  # the textbook figure of 0 / 10
    lo, hi = EM.wilson_interval(50, 100)
    assert abs(lo - MC.WILSON_50_OF_100[0]) <= 1e-12 and abs(hi - MC.WILSON_50_OF_100[1]) <= 1e-12
    assert abs(lo - 0.40383) < 1e-4 and abs(hi - 0.59617) < 1e-4
    lo, hi = EM.wilson_interval(10, 10)
    assert abs(hi - 1.0) <= 1e-12 and abs(lo - (1 - MC.WILSON_0_OF_10[1])) <= 1e-12  # symmetric
    assert EM.wilson_interval(0, 0) == (0.0, 1.0)


def test_summary_known_answers():
    t = _fixed_table(6)
    t["steps"][5] = 0  # an episode the run never reached: not counted
    succ = np.array([1, 0, 1, 0, 1, 0], bool)
    s = EM.summarize(t, succ, [0, 1, 2, 0, 1, 2], 0.032)
    assert (s["episodes"], s["counted"], s["successes"], s["flagged"]) == (6, 5, 3, 1)
    assert s["success_rate"] == 0.5 and s["per_world"] == {0: (1, 2), 1: (1, 2), 2: (1, 2)}
    assert s["wilson95"] == EM.wilson_interval(3, 6)
    mean, med, p95 = s["stats"]["steps"]["all"]
    assert (mean, med) == (12.0, 12.0) and abs(p95 - 13.8) < 1e-12  # 10..14: linear percentile
    assert s["stats"]["steps"]["success"][:2] == (12.0, 12.0)  # 10, 12, 14
    # first success of episodes 0, 2, 4 at steps 3, 5, 7
    assert np.allclose(s["stats"]["first_success_time"]["all"][:2], 5 * 0.032, rtol=1e-14, atol=0)
    mean, med, _ = s["stats"]["ee_path"]["all"]
    assert abs(mean - 3 * 5 / 7.0) < 1e-12 and abs(med - 3 * 5 / 7.0) < 1e-12
    assert EM.summarize(t[:0], succ[:0], [], 0.032)["stats"]["steps"]["all"] is None
    assert len(EM.summary_lines(s)) == 3 + 2 + len(EM.F64_FIELDS)


def test_table_columns_round_trip():
    t = _fixed_table(7, base=2**31 - 10)  # episode indices near the top of int32 are exact in f64
    cols = EM.table_to_columns(t, np.arange(7) % 3)
    assert cols.shape == (7, len(EM.TABLE_COLUMNS)) == (7, 12)
    back, widx = EM.columns_to_table(cols)
    assert back.tobytes() == t.tobytes() and widx.tolist() == (np.arange(7) % 3).tolist()


# -- the gather ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, total, out_dir):
    """One rank: gather_table on its own, then finish() of a sharded lockstep run with the flag."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g0, g1 = shard_range(rank, world, total)
    local = EM.table_to_columns(_fixed_table(g1 - g0, base=g0), np.arange(g0, g1) % 3)
    np.save(os.path.join(out_dir, f"g{rank}.npy"), gather_table(local, "cpu"))
    ro = _finished_rollout(g1 - g0, True)
    ro.args.env_offset = g0
    ro.args.result_filename = os.path.join(out_dir, f"result_r{rank}.yaml")
    ro.world_idx = np.arange(g0, g1) % 3
    ro._metrics.table = lambda: _fixed_table(g1 - g0, base=g0)
    ro.finish()
    np.save(os.path.join(out_dir, f"m{rank}.npy"), ro.episode_metrics)
    dist.destroy_process_group()


def test_gather_table_gloo_world2_unequal_shards(tmp_path):
    total, world = 7, 2  # shards of 4 and 3
    mp.spawn(_gather_worker, args=(world, _free_port(), total, str(tmp_path)), nprocs=world, join=True)
    want = _fixed_table(total)
    exp = EM.table_to_columns(want, np.arange(total) % 3)
    for r in range(world):
        np.testing.assert_array_equal(np.load(tmp_path / f"g{r}.npy"), exp)
        assert np.load(tmp_path / f"m{r}.npy").tobytes() == want.tobytes()  # every rank: global order
    with open(tmp_path / "result_r0.yaml") as f:
        data = yaml.safe_load(f)
    assert data["metrics"]["steps"] == want["steps"].tolist() and len(data["success"]) == total
    assert data["metrics"]["ee_path"] == want["ee_path"].tolist()
    assert not (tmp_path / "result_r1.yaml").exists()  # only rank 0 writes


# -- argument checks of the C entry point: before any device call -------------------------------------------
def _bufs(**over):
    b = N.MetricsBuffers()
    keep = np.zeros(64, np.float64)  # any non-NULL host address: the checks never dereference it
    for name in ("sched", "reward", "qpos", "qvel", "ctrl", "sensordata", "ee_pos", "table", "hist"):
        setattr(b, name, keep.ctypes.data)
    b.n_env, b.n_episodes, b.episode_base, b.n_pre = 4, 9, 10, 3
    b.nq, b.nv, b.nu, b.ctrl_stride, b.ee_stride = MC.NQ, MC.NV, MC.NU, MC.CTRL_STRIDE, MC.EE_STRIDE
    for j in range(6):
        b.arm_qadr[j], b.arm_dof[j] = MC.ARM_QADR[j], MC.ARM_DOF[j]
    for k, v in over.items():
        if k in ("arm_qadr", "arm_dof"):
            getattr(b, k)[v[0]] = v[1]
        else:
            setattr(b, k, v)
    return b, keep


@pytest.mark.parametrize("over,word", [
    (dict(ctrl_stride=MC.NU - 1), "ctrl_stride"), (dict(nu=5, ctrl_stride=8), "nu must be at least 6"),
    (dict(arm_qadr=(5, MC.NQ)), "arm_qadr[5]"), (dict(arm_qadr=(0, -1)), "arm_qadr[0]"),
    (dict(arm_dof=(2, MC.NV)), "arm_dof[2]"), (dict(ee_stride=2), "ee_stride"), (dict(n_env=-1), "negative"),
    (dict(n_episodes=-1), "negative"), (dict(table=None), "NULL"), (dict(hist=None), "NULL"),
    (dict(ee_pos=None), "NULL"), (dict(sched=None), "NULL"), (dict(reward=None), "NULL")])
def test_argument_checks_return_before_any_device_call(over, word):
    lib = N.load()
    b, keep = _bufs(**over)
    assert lib.rmbx_episode_metrics(ctypes.byref(b), None) == -1
    msg = lib.rmbx_last_error().decode()
    assert msg.startswith("rmbx_episode_metrics: ") and word in msg, msg


def test_null_struct_and_empty_batch():
    lib = N.load()
    assert lib.rmbx_episode_metrics(None, None) == -1
    assert b"bufs is NULL" in lib.rmbx_last_error()
    b, keep = _bufs(n_env=0)
    assert lib.rmbx_episode_metrics(ctypes.byref(b), None) == 0  # nothing to do: no launch
    assert ctypes.sizeof(N.MetricsBuffers) == 12 * 8 + 9 * 4 + 12 * 4 + 4  # 12 pointers, 21 ints, padded to 8
    assert N.METRICS_DTYPE.itemsize == 72 and N.METRICS_DTYPE.names[0] == "episode"


def test_wrapper_rejects_host_tensors_and_bad_addresses():
    """kernels.EpisodeMetrics checks shapes, dtypes and devices before it binds a pointer."""
    import types

    from robomanipbaselines_amd import kernels as K

    n = 3
    eng = types.SimpleNamespace(nq=MC.NQ, nv=MC.NV, nu=MC.NU, qpos=torch.zeros(n, MC.NQ, dtype=torch.float64),
                                qvel=torch.zeros(n, MC.NV, dtype=torch.float64),
                                _ctrl_store=torch.zeros(n, MC.CTRL_STRIDE, dtype=torch.float64),
                                sensordata=torch.zeros(n, 6, dtype=torch.float64))
    sched = torch.zeros(n, N.SCHED_DTYPE.itemsize, dtype=torch.uint8)
    ee = torch.zeros(n, MC.EE_STRIDE, dtype=torch.float64)[:, 5:8]
    with pytest.raises(ValueError, match="device tensor"):
        K.EpisodeMetrics(sched, eng, 3, 9, arm_qadr=MC.ARM_QADR, arm_dof=MC.ARM_DOF, ee_pos=ee)
    with pytest.raises(ValueError, match="out of range"):
        K.EpisodeMetrics(sched, eng, 3, 9, arm_qadr=(0, 1, 2, 3, 4, MC.NQ), arm_dof=MC.ARM_DOF, ee_pos=ee)
    with pytest.raises(ValueError, match="6 entries"):
        K.EpisodeMetrics(sched, eng, 3, 9, arm_qadr=(0, 1, 2), arm_dof=MC.ARM_DOF, ee_pos=ee)
    with pytest.raises(ValueError, match="required"):
        K.EpisodeMetrics(sched, eng, 3, 9, ee_pos=ee)
    eng.nu = 5
    with pytest.raises(ValueError, match="at least 6"):
        K.EpisodeMetrics(sched, eng, 3, 9, arm_qadr=MC.ARM_QADR, arm_dof=MC.ARM_DOF, ee_pos=ee)


def test_bench_policy_passes_the_flag_through(monkeypatch):
    import importlib.util

    from conftest import ROOT

    # (the script sets a MIOpen variable when it is imported: keep it out of this process)
    monkeypatch.delenv("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", raising=False)
    monkeypatch.setattr("sys.path", list(__import__("sys").path))
    spec = importlib.util.spec_from_file_location("bench_policy_metrics_under_test",
                                                  os.path.join(ROOT, "scripts", "bench_policy.py"))
    bp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bp)
    assert "--episode_metrics" in bp.rollout_argv(bp.parse_args(["Act", "--episode_metrics"]))
    assert "--episode_metrics" not in bp.rollout_argv(bp.parse_args(["Act"]))
    assert _parse(bp.rollout_argv(bp.parse_args(["Mlp", "--episode_metrics"]))).episode_metrics is True
    assert math.isclose(EM.Z95, MC.Z95)
