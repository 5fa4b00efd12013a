"""Streaming rollouts (--num_episodes) on the device: the recycle / phase / bad-state kernels
against their numpy models (tests/stream_cases.py) bit for bit, the alignment invariant of the
schedule, and the equivalence of a streamed episode with the same episode of a lockstep run --
results and final qpos, bitwise -- which holds only if the world, the engine state, the motion
commands and the policy state of a recycled slot were all re-armed exactly."""

import types

import numpy as np
import pytest
import torch
import yaml

import stream_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_stream(st):
    """A kernels.EpisodeStream over device copies of the synthetic state `st` (SC.make_state)."""
    from robomanipbaselines_amd import _native as N
    from robomanipbaselines_amd import kernels as K

    n = len(st["sched"])
    eng = types.SimpleNamespace(nq=SC.NQ, nv=SC.NV, nu=SC.NU, nbody=SC.NBODY, time=_t(st["time"]), qpos=_t(st["qpos"]),
                                qvel=_t(st["qvel"]), qacc_ws=_t(st["qacc_ws"]), _ctrl_store=_t(st["ctrl"]),
                                body_pos=_t(st["body_pos"]), stats=_t(st["stats"]))
    sched = _t(st["sched"].view(np.uint8).reshape(n, N.SCHED_DTYPE.itemsize))
    es = K.EpisodeStream(sched, eng, _t(st["q_cmd"]), _t(st["grip_cmd"]), _t(st["target_R"]), _t(st["target_p"]),
                         _t(st["bad_resets"]), st["qpos0"], st["ctrl0"], st["motion0"], st["world_idx"],
                         st["world_pos"], episode_base=st["episode_base"], world_body=st["world_body"],
                         world_qadr=st["world_qadr"], final_qpos=True)
    es.slot_episode.copy_(_t(st["slot_episode"]))
    es.recycled.copy_(_t(st["recycled"]))
    es.counters.copy_(_t(st["counters"]))
    es.results.copy_(_t(st["results"].view(np.uint8).reshape(len(st["results"]), -1)))
    es.final_qpos.copy_(_t(st["final_qpos"]))
    es.last_elapsed.copy_(_t(st["last_elapsed"]))
    return es


def _device_state(es):
    q_cmd, grip_cmd, tgt_R, tgt_p = es.motion
    e = es.engine
    tensors = {"sched": es.sched, "slot_episode": es.slot_episode, "recycled": es.recycled, "counters": es.counters,
               "results": es.results, "final_qpos": es.final_qpos, "time": e.time, "qpos": e.qpos, "qvel": e.qvel,
               "qacc_ws": e.qacc_ws, "ctrl": e._ctrl_store, "body_pos": e.body_pos, "stats": e.stats, "q_cmd": q_cmd,
               "grip_cmd": grip_cmd, "target_R": tgt_R, "target_p": tgt_p, "bad_resets": es.bad_resets,
               "last_elapsed": es.last_elapsed}
    return {k: v.cpu().numpy() for k, v in tensors.items()}


def _assert_state_equal(got, want, what):
    for k in SC.STATE_KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), f"{what}: {k} differs"


# -- 1. the recycle kernel against the numpy model ------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 300])  # 300 crosses the kernel's 256-slot chunk
@pytest.mark.parametrize("pattern", ["none", "all", "alternating"])
@pytest.mark.parametrize("queue", ["more", "fewer", "empty"])
def test_recycle_kernel_matches_model_bitwise(n, pattern, queue):
    done = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0}[pattern]
    M = 2 * n + 4
    next_local = {"more": n, "fewer": M - int(done.sum()) // 2, "empty": M}[queue]
    st = SC.make_state(n, M, done, next_local)
    es = _device_stream(st)
    es.recycle()
    torch.cuda.synchronize()
    want = SC.recycle_model(st)
    got = _device_state(es)
    _assert_state_equal(got, want, "first launch")
    # slots that were not done: byte-identical to the input
    keep = ~done
    for k in SC.STATE_KEYS:
        if k not in ("recycled", "counters", "results", "final_qpos"):
            assert got[k][keep].tobytes() == np.ascontiguousarray(st[k][keep]).tobytes(), k
    # the episodes went to the finished slots in increasing slot order
    newly = got["slot_episode"][done]
    given = newly[newly >= 0]
    assert given.tolist() == list(range(10 + next_local, 10 + next_local + len(given)))
    assert (newly[len(given):] == -1).all()
    # a second launch: re-armed slots are running, retired slots are recorded once and never again
    es.recycle()
    torch.cuda.synchronize()
    again = _device_state(es)
    _assert_state_equal(again, SC.recycle_model(want), "second launch")
    assert again["results"].tobytes() == got["results"].tobytes()
    assert again["counters"].tolist() == got["counters"].tolist()


def test_recycle_kernel_places_a_free_body():
    n, M = 5, 14
    done = np.array([1, 0, 1, 1, 0], bool)
    st = SC.make_state(n, M, done, next_local=6, world_body=-1, world_qadr=4)
    es = _device_stream(st)
    es.recycle()
    got = _device_state(es)
    _assert_state_equal(got, SC.recycle_model(st), "free body")
    for rank, s in enumerate((0, 2, 3)):
        np.testing.assert_array_equal(got["qpos"][s, 4:7], st["world_pos"][6 + rank])
        np.testing.assert_array_equal(got["qpos"][s, :4], st["qpos0"][:4])
    assert got["body_pos"].tobytes() == st["body_pos"].tobytes()
    # neither: the task moves nothing (Pick)
    st = SC.make_state(n, M, done, next_local=6, world_body=-1, world_qadr=-1)
    es = _device_stream(st)
    es.recycle()
    got = _device_state(es)
    _assert_state_equal(got, SC.recycle_model(st), "no world")
    np.testing.assert_array_equal(got["qpos"][0], st["qpos0"])


def test_recycle_argument_checks():
    st = SC.make_state(3, 8, np.ones(3, bool), 3)
    st["world_body"] = SC.NBODY  # out of range
    with pytest.raises(ValueError):
        _device_stream(st)
    st["world_body"], st["world_qadr"] = 1, 2  # both
    with pytest.raises(ValueError):
        _device_stream(st)
    st["world_body"], st["world_qadr"] = -1, SC.NQ - 2  # runs past the row
    with pytest.raises(ValueError):
        _device_stream(st)


# -- 2. rmbx_sched_phases and rmbx_sched_close_bad against numpy ------------------------------------
def test_sched_phases_and_close_bad_match_models():
    from robomanipbaselines_amd import _native as N
    from robomanipbaselines_amd import kernels as K

    n, n_pre = 300, 4
    rng = np.random.default_rng(3)
    sched = np.zeros(n, dtype=N.SCHED_DTYPE)
    prev = np.full(n, -1, np.int32)
    d_prev, d_phase, d_ent = _t(prev), torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    last = np.zeros(n)
    d_last = _t(last)
    for it in range(8):
        # scripted: some slots advance a phase, every third call re-arms a few slots to phase 0
        adv = rng.random(n) < 0.4
        sched["phase"] = np.minimum(sched["phase"] + adv, n_pre + 1)
        if it % 3 == 2:
            rearm = rng.random(n) < 0.2
            sched["phase"][rearm] = 0
            sched["done"][rearm] = 0
        sched["done"] |= (sched["phase"] == n_pre + 1) & (rng.random(n) < 0.5)
        sched["phase_start"] = rng.random(n)
        time = 1.0 + rng.random(n)
        bad = (rng.random(n) < 0.1).astype(np.int32)
        d_sched = _t(sched.view(np.uint8).reshape(n, -1))
        K.sched_close_bad(d_sched, _t(time), _t(bad), d_last, n_pre)
        sched, last = SC.close_bad_model(sched, time, bad, last, n_pre)
        assert d_sched.cpu().numpy().tobytes() == sched.tobytes(), it
        assert d_last.cpu().numpy().tobytes() == last.tobytes(), it
        K.sched_phases(d_sched, d_prev, d_phase, d_ent)
        phase, ent, prev = SC.sched_phases_model(sched, prev)
        np.testing.assert_array_equal(d_phase.cpu().numpy(), phase)
        np.testing.assert_array_equal(d_ent.cpu().numpy(), ent)
        np.testing.assert_array_equal(d_prev.cpu().numpy(), prev)
        if it % 3 == 2:
            assert ent[(phase == 0)].any()  # a re-armed slot reports phase 0 as entered


# -- rollouts ------------------------------------------------------------------------------------
def _compose(policy):
    from robomanipbaselines_amd.envs.operation.OperationMujocoUR5eCable import OperationMujocoUR5eCable

    if policy == "Sarnn":
        from robomanipbaselines_amd.policy.sarnn.rollout_sarnn import RolloutSarnn as P
    elif policy == "Act":
        from robomanipbaselines_amd.policy.act.rollout_act import RolloutAct as P
    elif policy == "Mlp":
        from robomanipbaselines_amd.policy.mlp.rollout_mlp import RolloutMlp as P
    elif policy == "DiffusionPolicy":
        from robomanipbaselines_amd.policy.diffusion_policy.rollout_diffusion_policy import RolloutDiffusionPolicy as P
    else:
        from robomanipbaselines_amd.policy.diffusion_policy_3d.rollout_diffusion_policy_3d import (
            RolloutDiffusionPolicy3d as P)

    class Rollout(OperationMujocoUR5eCable, P):
        pass

    return Rollout


def _force_success(ro, episode_of_slot, at=0.1):
    """Reward wrapper of the tests: success is forced from `at` seconds of RolloutPhase on, for the
    episodes with episode % 3 == 1.  It reads the schedule as the step's reward does: before
    rmbx_sched_update of that step."""
    env, inner, n_pre = ro.env, ro.env._get_reward, len(ro.pre_durations)

    def wrapped():
        r = inner()
        sched = getattr(ro, "sched", None)
        if sched is None:
            return r
        phase = sched.view(torch.int32)[:, 0]
        start = sched.view(torch.float64)[:, 2]
        hit = (phase == n_pre) & (env.engine.time - start >= at) & (episode_of_slot() % 3 == 1)
        return torch.where(hit, torch.ones_like(r), r)

    env._get_reward = wrapped


def _run_streaming_checked(ro):
    """run_streaming() step by step, reading the alignment invariant after every step: every slot in
    RolloutPhase has sched.rollout_time_idx == the host's index mod P; slots change episode only on
    aligned steps."""
    from robomanipbaselines_amd import kernels as K

    ro.reset_streaming()
    P, n_pre, M = ro.stream_period, len(ro.pre_durations), ro.args.num_episodes
    seen_rollout = 0
    slot_ep = ro.slot_episode.cpu().numpy().copy()
    for g in range(4000):
        ro.step_stream()
        v = K.sched_view(ro.sched)
        in_rollout = (v["phase"] == n_pre) & (v["done"] == 0)
        seen_rollout += int(in_rollout.sum())
        assert ((v["rollout_time_idx"][in_rollout] - ro.rollout_time_idx) % P == 0).all(), (g, v["rollout_time_idx"])
        now = ro.slot_episode.cpu().numpy().copy()
        if (g + 1) % P != 0:
            np.testing.assert_array_equal(now, slot_ep, err_msg=f"slot changed episode on unaligned step {g}")
        slot_ep = now
        if int(ro.stream.counters.cpu()[1]) >= M:
            break
    else:
        raise AssertionError("the streaming run did not end")
    assert seen_rollout > 0
    ro.finish()


@pytest.mark.parametrize("policy", ["Sarnn", "Act", "Mlp"])
def test_streamed_episodes_equal_lockstep_episodes(policy):
    from robomanipbaselines_amd import kernels as K

    n, M = 3, 7
    ro = _compose(policy)(argv=["--num_envs", str(n), "--num_episodes", str(M), "--device", DEV, "--max_duration", "1.6",
                                "--world_idx_list", "0", "1", "2", "3", "4", "5", "--world_random_scale", "0.01", "0.01",
                                "0.0", "--seed", "3", "--precision", "fp32"])
    if policy == "Mlp":
        ro.model_meta_info["data"]["n_obs_steps"] = 2
        ro.model_meta_info["data"]["n_action_steps"] = 2
        ro.setup_policy()
        assert ro.n_obs_steps == 2 and ro.stream_period == 2 * ro.args.skip
    assert ro.n == n
    ro.record_final_qpos = True
    offset = [0]
    _force_success(ro, lambda: (ro.slot_episode if ro.args.num_episodes is not None
                                else offset[0] + torch.arange(n, dtype=torch.int32, device=DEV)))
    if policy == "Sarnn":
        _run_streaming_checked(ro)
    else:
        ro.run()
    rec = ro.episode_records
    final = ro.stream.final_qpos.cpu().numpy()
    assert len(ro.result["success"]) == M and rec["episode"].tolist() == list(range(M))
    assert int(ro.stream.counters.cpu()[1]) == M
    assert len(set(rec["slot"].tolist())) > 1 and sorted(set(rec["slot"].tolist())) <= [0, 1, 2]
    print(f"\n{policy}: slots {rec['slot'].tolist()} steps {rec['rollout_time_idx'].tolist()} "
          f"success {rec['success'].tolist()}")
    # the lockstep baseline: three runs of 3 envs at --env_offset 0, 3, 6, same object and weights
    ro.args.num_episodes = None
    for off in (0, 3, 6):
        offset[0] = off
        ro.args.env_offset = ro.env.env_offset = off
        ro.run()
        v = K.sched_view(ro.sched)
        qpos = ro.env.engine.qpos.cpu().numpy()
        for e in range(n):
            i = off + e
            if i >= M:
                continue
            assert rec["world_idx"][i] == ro.world_idx[e] == i % 6
            assert bool(rec["success"][i]) == bool(v["success"][e]) == (i % 3 == 1), i
            assert rec["reward"][i] == v["result_reward"][e], i
            assert rec["duration"][i] == v["duration"][e], i
            assert rec["rollout_time_idx"][i] == v["rollout_time_idx"][e], i
            assert final[i].tobytes() == qpos[e].tobytes(), f"episode {i}: final qpos differs from lockstep env {e}"
    # forced successes end about 1.1 s into the rollout, the others at max_duration
    assert rec["rollout_time_idx"][1] < rec["rollout_time_idx"][0]


@pytest.mark.parametrize("policy", ["DiffusionPolicy", "DiffusionPolicy3d"])
def test_diffusion_policies_stream(policy):
    n, M = 2, 5
    # (skip 6: P = 48 env-steps, so the 100-step DDPM sampler runs half as often as at the default 3)
    ro = _compose(policy)(argv=["--num_envs", str(n), "--num_episodes", str(M), "--device", DEV, "--max_duration", "0.3",
                                "--world_idx_list", "0", "1", "2", "--skip", "6"])
    assert ro.stream_period == 6 * ro.n_action_steps
    ro.run()
    rec = ro.episode_records
    assert len(rec) == M and sorted(rec["episode"].tolist()) == list(range(M))
    assert np.isfinite(rec["reward"]).all() and np.isfinite(rec["duration"]).all()
    assert (rec["duration"] > 0.3).all() and (rec["bad_state"] == 0).all()
    assert ro.stream.counters.cpu().tolist() == [M, M]
    assert rec["world_idx"].tolist() == [0, 1, 2, 0, 1]
    assert np.isfinite(ro.env.engine.qpos.cpu().numpy()).all()


def test_cli_streams_more_episodes_than_envs(tmp_path, capsys):
    from robomanipbaselines_amd.bin.Rollout import main

    res = str(tmp_path / "result.yaml")
    ro = main(["Sarnn", "MujocoUR5eCable", "--num_envs", "2", "--num_episodes", "5", "--world_idx_list", "0", "1", "2",
               "--max_duration", "0.3", "--result_filename", res])
    out = capsys.readouterr().out
    with open(res) as f:
        data = yaml.safe_load(f)
    assert set(data) == {"success", "reward", "duration"}
    assert len(data["success"]) == len(data["reward"]) == len(data["duration"]) == 5
    assert out.count("Rollout result: ") == 5
    assert ro.n == 2 and ro.episode_records["world_idx"].tolist() == [0, 1, 2, 0, 1]
    assert ro.episode_records["episode"].tolist() == [0, 1, 2, 3, 4]
    for d in data["duration"]:
        assert 0.3 < d <= 0.3 + 0.032 + 1e-9


def test_bad_state_closes_the_episode_and_the_run_ends():
    n, M, hit_step, hit_slot = 2, 4, 100, 1
    ro = _compose("Sarnn")(argv=["--num_envs", str(n), "--num_episodes", str(M), "--device", DEV, "--max_duration", "1.0"])
    calls = [0]
    inner = ro.env._reset_bad_states

    def injected():
        # the seam: what the divergence guard reports, with no diverging physics
        inner()
        if calls[0] == hit_step:
            ro.env.bad_resets[hit_slot] += 1
        calls[0] += 1

    ro.env._reset_bad_states = injected
    steps = ro.run()
    rec = ro.episode_records
    N_pre = ro._entry_steps[-1]
    assert N_pre < hit_step
    assert rec["episode"].tolist() == list(range(M)) and steps < 600
    assert rec["bad_state"].tolist() == [0, 1, 0, 0]
    assert not rec["success"][1] and rec["reward"][1] == 0.0
    # its rollout-phase time at the last step before the reset
    assert abs(rec["duration"][1] - 0.032 * (hit_step - N_pre)) < 1e-9
    others = [0, 2, 3]
    assert (rec["duration"][others] > 1.0).all() and (rec["duration"][others] <= 1.0 + 0.032 + 1e-9).all()
    assert ro.bad_state_episodes == 1
    # the closed slot was recycled: three episodes ran in its slot or the other
    assert sorted(rec["slot"].tolist()) != [0, 0, 0, 0]
