"""The episode trace (--trace_dir) on the device: the trace kernel against its numpy model
(tests/trace_cases.py) bit for bit over consecutive calls, the trace of a streamed episode against
the trace of the same episode of a lockstep run -- every field of every row -- the run with and
without tracing, Replay against the frames of the live steps, stride and selection, and the CLIs.
Every comparison is bitwise."""

import glob
import os
import types

import numpy as np
import pytest
import torch

import trace_cases as TC
from robomanipbaselines_amd.common import episode_trace as ET

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENGINE_KEYS = ("time", "ctrl", "qpos", "qvel", "gxpos", "gxmat", "xpos", "xquat")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Device:
    """A kernels.EpisodeTrace over device copies of a synthetic state (TC.make_state).  The chunk has
    `guard` rows more than the kernel is told of, filled like the rest with TC.FILL."""

    def __init__(self, st, dims, n_episodes, episode_base, slot_episode, select, stride, capacity, guard=0,
                 bad_resets=True):
        from robomanipbaselines_amd import _native as N
        from robomanipbaselines_amd import kernels as K

        n = len(st["sched"])
        self.eng = types.SimpleNamespace(_ctrl_store=_t(st["ctrl"]), **dims,
                                         **{k: _t(st[k]) for k in ENGINE_KEYS if k != "ctrl"})
        self.sched = _t(st["sched"].view(np.uint8).reshape(n, N.SCHED_DTYPE.itemsize))
        self.slot_episode = None if slot_episode is None else _t(slot_episode)
        self.bad = _t(st["bad_resets"]) if bad_resets else None
        self.reward = _t(st["reward"])
        self.tr = K.EpisodeTrace(self.sched, self.eng, n_episodes, TC.N_PRE, episode_base=episode_base,
                                 slot_episode=self.slot_episode, select=None if select is None else _t(select),
                                 stride=stride, bad_resets=self.bad, capacity=capacity + guard)
        self.tr._bufs.capacity = capacity
        for k, v in TC.new_chunk(capacity + guard, dims).items():
            self.tr.chunk[k].copy_(_t(v))

    def load(self, st, slot_episode=None):
        """The arrays of the next env-step."""
        n = len(st["sched"])
        self.sched.copy_(_t(st["sched"].view(np.uint8).reshape(n, -1)))
        self.eng._ctrl_store.copy_(_t(st["ctrl"]))
        for k in ENGINE_KEYS:
            if k != "ctrl":
                getattr(self.eng, k).copy_(_t(st[k]))
        self.reward = _t(st["reward"])  # a new tensor every step, as the env's reward is
        if self.bad is not None:
            self.bad.copy_(_t(st["bad_resets"]))
        if slot_episode is not None:
            self.slot_episode.copy_(_t(slot_episode))

    def state(self):
        tr = self.tr
        return (tr.trace_episode.cpu().numpy(), tr.trace_step.cpu().numpy(), tr.rows.cpu().numpy(),
                {k: v.cpu().numpy() for k, v in tr.chunk.items()})


def _assert_same(got, want, what):
    for name, g, w in zip(("trace_episode", "trace_step", "rows"), got[:3], want[:3]):
        assert g.tobytes() == w.tobytes(), f"{what}: {name} {g.tolist()} != {w.tolist()}"
    for k in ET.FIELDS:
        assert got[3][k].tobytes() == want[3][k].tobytes(), f"{what}: chunk field {k} differs"


def _drive(n, dims, ctrl_stride, stepped_pattern, select_kind, stride, lockstep=False, calls=5, seed=0):
    """`calls` consecutive launches against the model: the per-slot step counters carry over, `done`
    falls on steps the stride would drop, and (with a slot map) slots change episode between calls."""
    rng = np.random.default_rng(100 * n + seed)
    base, M = 10, 2 * n + 4
    st = TC.make_state(n, dims, ctrl_stride, seed=n)
    slot_episode = None if lockstep else (base + rng.permutation(M)[:n]).astype(np.int32)
    select = {"null": None, "some": (np.arange(M) % 3 != 0).astype(np.uint8), "none": np.zeros(M, np.uint8)}[select_kind]
    capacity = calls * n
    dev = _Device(st, dims, M, base, slot_episode, select, stride, capacity, guard=2)
    chunk = TC.new_chunk(capacity + 2, dims)
    written = 0
    for c in range(calls):
        stepped = {"none": np.zeros(n, np.uint8), "all": None, "alternating": ((np.arange(n) + c) % 2).astype(np.uint8)}[
            stepped_pattern]
        st.update(TC.step_inputs(n, dims, ctrl_stride, rng))
        if slot_episode is not None and c in (2, 3):
            # slots whose episode changes between calls: one gets a fresh episode, one is retired
            slot_episode = slot_episode.copy()
            slot_episode[0] = base + M - 1 - c
            if n > 1:
                slot_episode[n - 1] = -1
        dev.load(st, slot_episode)
        dev.tr.record(None if stepped is None else _t(stepped), dev.reward)
        te, ts, rows, chunk = TC.trace_model(st, chunk, capacity, dims, slot_episode, stepped, select, base, M, stride)
        _assert_same(dev.state(), (te, ts, rows, chunk), f"call {c}")
        st.update(trace_episode=te, trace_step=ts, rows=rows)
        written = int(rows[0])
    return written, chunk, dev


# -- 1. the kernel against the numpy model --------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 300])  # 300 crosses the kernel's 256-slot scan chunk
@pytest.mark.parametrize("stepped", ["none", "all", "alternating"])
@pytest.mark.parametrize("select", ["null", "some", "none"])
@pytest.mark.parametrize("stride", [1, 3])
def test_trace_kernel_matches_model_bitwise(n, stepped, select, stride):
    written, chunk, dev = _drive(n, TC.DIMS, TC.CTRL_STRIDE, stepped, select, stride)
    if stepped == "none" or select == "none":
        assert written == 0
    elif stepped == "all" and select == "null" and stride == 1 and n == 5:
        assert 5 * (n - 2) <= written <= 5 * n
    if written:
        # the flush hands back exactly the used rows and empties the chunk
        rows = dev.tr.flush()
        for k in ET.FIELDS:
            assert rows[k].tobytes() == chunk[k][:written].tobytes(), k
        assert dev.tr.rows.cpu().tolist() == [0, 0] and dev.tr.flush() is None


def test_trace_kernel_without_a_slot_map_and_with_the_cable_dimensions():
    # slot_episode = NULL: slot e holds episode episode_base + e (a lockstep run)
    written, chunk, _ = _drive(5, TC.DIMS, TC.CTRL_STRIDE, "alternating", "some", 3, lockstep=True)
    assert written > 0 and set(chunk["episode"][:written] - chunk["slot"][:written]) == {10}
    written, _, _ = _drive(300, TC.DIMS, TC.CTRL_STRIDE, "all", "null", 1, lockstep=True, calls=3)
    assert written == 900
    # the Cable scene's rows: nq = 69 doubles, a ctrl row stride equal to nu
    written, chunk, _ = _drive(37, TC.CABLE_DIMS, TC.CABLE_DIMS["nu"], "all", "null", 1, calls=3)
    assert written > 2 * 37
    written, _, _ = _drive(6, TC.CABLE_DIMS, TC.CABLE_DIMS["nu"], "alternating", "some", 3, calls=4)
    assert written > 0


def test_trace_kernel_overflow_keeps_the_rows_that_fit_and_touches_nothing_else():
    n, dims, capacity, guard = 300, TC.DIMS, 420, 3
    st = TC.make_state(n, dims, TC.CTRL_STRIDE, seed=5)
    dev = _Device(st, dims, n, 0, None, None, 1, capacity, guard=guard)
    chunk = TC.new_chunk(capacity + guard, dims)
    rng = np.random.default_rng(9)
    for c in range(2):  # 300 rows, then 300 more of which 120 fit
        st.update(TC.step_inputs(n, dims, TC.CTRL_STRIDE, rng))
        dev.load(st)
        dev.tr.record(None, dev.reward)
        te, ts, rows, chunk = TC.trace_model(st, chunk, capacity, dims, None, None, None, 0, n, 1)
        st.update(trace_episode=te, trace_step=ts, rows=rows)
    got = dev.state()
    _assert_same(got, (te, ts, rows, chunk), "overflow")
    assert got[2].tolist() == [capacity, 1]
    assert got[3]["slot"][300:capacity].tolist() == list(range(120)) and (got[3]["step"][300:capacity] == 2).all()
    for k, (dt, _) in ET.FIELDS.items():  # the guard rows keep their fill value
        assert (got[3][k][capacity:] == TC.FILL[np.dtype(dt)]).all(), k
    assert (got[1] == 2).all()  # the step counters advanced for the dropped rows too
    with pytest.raises(RuntimeError, match="overflowed"):
        dev.tr.flush()


def test_trace_argument_checks():
    import ctypes

    from robomanipbaselines_amd import _native as N
    from robomanipbaselines_amd import kernels as K

    st = TC.make_state(4, TC.DIMS, TC.CTRL_STRIDE)
    dev = _Device(st, TC.DIMS, 4, 0, None, None, 1, 8)
    lib, b = N.load(), dev.tr._bufs
    b.stepped, b.reward = None, N.ptr(dev.reward)

    def status(**change):
        keep = {k: getattr(b, k) for k in change}
        for k, v in change.items():
            setattr(b, k, v)
        code = lib.rmbx_episode_trace(ctypes.byref(b), None)
        for k, v in keep.items():
            setattr(b, k, v)
        return code, lib.rmbx_last_error()

    for field in ("sched", "reward", "qpos", "xquat", "trace_step", "slot_row", "out_gxmat", "out_flags", "rows"):
        s, msg = status(**{field: None})
        assert s == -1 and b"NULL" in msg, field
    s, msg = status(stride=0)
    assert s == -1 and b"stride" in msg
    s, msg = status(capacity=0)
    assert s == -1 and b"capacity" in msg
    s, msg = status(nq=0)
    assert s == -1 and b"positive" in msg
    s, msg = status(ctrl_stride=TC.DIMS["nu"] - 1)
    assert s == -1 and b"ctrl_stride" in msg
    assert lib.rmbx_episode_trace(None, None) == -1
    torch.cuda.synchronize()
    assert dev.tr.rows.cpu().tolist() == [0, 0]  # no refused call launched anything
    # the wrapper refuses what it can see
    with pytest.raises(ValueError, match="stride"):
        K.EpisodeTrace(dev.sched, dev.eng, 4, TC.N_PRE, stride=0)
    with pytest.raises(ValueError, match="capacity"):
        K.EpisodeTrace(dev.sched, dev.eng, 4, TC.N_PRE, capacity=0)
    with pytest.raises(ValueError, match="qpos"):
        K.EpisodeTrace(dev.sched, types.SimpleNamespace(**dict(vars(dev.eng), qpos=dev.eng.qvel)), 4, TC.N_PRE)
    with pytest.raises(ValueError, match="select"):
        K.EpisodeTrace(dev.sched, dev.eng, 4, TC.N_PRE, select=torch.zeros(3, dtype=torch.uint8, device=DEV))


# -- rollouts ------------------------------------------------------------------------------------
def _rows_equal(a, b, what, skip=("slot",)):
    assert len(a["step"]) == len(b["step"]), f"{what}: {len(a['step'])} rows against {len(b['step'])}"
    for k in ET.FIELDS:
        if k not in skip:
            assert a[k].tobytes() == b[k].tobytes(), f"{what}: field {k} differs"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The streaming configuration of test_stream_gpu.py::test_streamed_episodes_equal_lockstep_episodes
    (SARNN, 3 slots, 7 episodes, forced early successes, --max_duration 1.6), run once with a full
    trace, once without tracing, once with --trace_stride 3 --trace_episodes 1 4, and the lockstep
    runs at --env_offset 0, 3, 6 with tracing on -- one rollout object, as in that test."""
    from test_stream_gpu import _compose, _force_success

    n, M = 3, 7
    root = tmp_path_factory.mktemp("traces")
    ro = _compose("Sarnn")(argv=["--num_envs", str(n), "--num_episodes", str(M), "--device", DEV, "--max_duration", "1.6",
                                 "--world_idx_list", "0", "1", "2", "3", "4", "5", "--world_random_scale", "0.01", "0.01",
                                 "0.0", "--seed", "3", "--precision", "fp32", "--trace_dir", str(root / "stream")])
    ro.record_final_qpos = True
    offset = [0]
    _force_success(ro, lambda: (ro.slot_episode if ro.args.num_episodes is not None
                                else offset[0] + torch.arange(n, dtype=torch.int32, device=DEV)))
    out = {"M": M, "n": n, "ro": ro}

    def stream(name, trace_dir, stride=1, episodes=("all",)):
        ro.args.trace_dir, ro.args.trace_stride, ro.args.trace_episodes = trace_dir, stride, list(episodes)
        ro.result = {key: [] for key in ("success", "reward", "duration")}
        steps = ro.run()
        out[name] = {"records": ro.episode_records.copy(), "final_qpos": ro.stream.final_qpos.cpu().numpy(),
                     "steps": steps, "dir": trace_dir}

    stream("stream", str(root / "stream"))
    stream("plain", None)
    stream("sparse", str(root / "sparse"), stride=3, episodes=("1", "4"))
    ro.args.num_episodes, ro.args.trace_stride, ro.args.trace_episodes = None, 1, ["all"]
    out["lockstep"] = []
    for off in (0, 3, 6):
        offset[0] = off
        ro.args.env_offset = ro.env.env_offset = off
        ro.args.trace_dir = str(root / f"lockstep{off}")
        ro.run()
        out["lockstep"].append(ro.args.trace_dir)
    return out


# -- 2. streaming equals lockstep over the whole trajectory ---------------------------------------
def test_streamed_trace_equals_lockstep_trace(runs):
    M = runs["M"]
    st = ET.TraceReader(runs["stream"]["dir"])
    rec, final = runs["stream"]["records"], runs["stream"]["final_qpos"]
    assert st.traced_episodes == list(range(M))
    assert st.header["streaming"] and st.header["dims"] == TC.CABLE_DIMS and st.header["policy"] == "Sarnn"
    # episodes.npy is the run's episode_records
    assert st.episodes.tobytes() == rec.tobytes() and st.episodes.dtype == rec.dtype
    seen = 0
    for d, off in zip(runs["lockstep"], (0, 3, 6)):
        lk = ET.TraceReader(d)
        assert not lk.header["streaming"] and lk.header["episode_base"] == off
        for i in lk.traced_episodes:
            if i >= M:
                continue
            a, b = st.episode(i), lk.episode(i)
            _rows_equal(a, b, f"episode {i}")
            K_ = len(a["step"])
            assert a["step"].tolist() == list(range(1, K_ + 1)), i  # 1 .. K without gaps
            assert a["flags"][-1] & ET.FLAG_DONE and not (a["flags"][:-1] & ET.FLAG_DONE).any(), i
            assert bool(a["flags"][-1] & ET.FLAG_SUCCESS) == bool(rec["success"][i]) == (i % 3 == 1), i
            assert not (a["flags"] & ET.FLAG_BAD_STATE).any()
            assert a["qpos"][-1].tobytes() == final[i].tobytes(), f"episode {i}: last row is not the final qpos"
            assert a["rollout_time_idx"][-1] == rec["rollout_time_idx"][i] and (a["slot"] == rec["slot"][i]).all()
            assert (b["slot"] == i - off).all()
            assert (np.diff(a["time"]) > 0).all()
            # the lockstep records carry the same results
            r = lk.record(i)
            for f in ("world_idx", "success", "reward", "duration", "rollout_time_idx", "bad_state"):
                assert r[f] == rec[f][i], (i, f)
            seen += 1
    assert seen == M
    # forced successes end early, so the episodes differ in length and the slots ran out of step
    lengths = [len(st.episode(i)["step"]) for i in range(M)]
    assert lengths[1] < lengths[0] and len(set(rec["slot"].tolist())) > 1


# -- 3. tracing does not disturb the run ----------------------------------------------------------
def test_tracing_does_not_disturb_the_run(runs):
    a, b = runs["stream"], runs["plain"]
    assert a["records"].tobytes() == b["records"].tobytes()
    assert a["final_qpos"].tobytes() == b["final_qpos"].tobytes()
    assert a["steps"] == b["steps"]
    assert runs["sparse"]["records"].tobytes() == b["records"].tobytes()


# -- 5. stride and selection end to end -----------------------------------------------------------
def test_stride_and_selection(runs):
    full, sp = ET.TraceReader(runs["stream"]["dir"]), ET.TraceReader(runs["sparse"]["dir"])
    assert sp.traced_episodes == [1, 4] and sp.header["stride"] == 3 and sp.header["trace_episodes"] == [1, 4]
    assert sp.episodes.tobytes() == full.episodes.tobytes()  # the records are of every episode
    for i in (1, 4):
        a, b = full.episode(i), sp.episode(i)
        last = int(a["step"][-1])
        want = sorted(set(range(3, last + 1, 3)) | {last})
        assert b["step"].tolist() == want, i
        pick = np.searchsorted(a["step"], b["step"])
        _rows_equal({k: v[pick] for k, v in a.items()}, b, f"episode {i} at stride 3", skip=())


# -- 4. replay equals the live frames -------------------------------------------------------------
@pytest.mark.parametrize("shadows,offsamples", [("off", "1"), ("scene", "4")])
def test_replay_equals_the_live_frames(tmp_path, shadows, offsamples):
    from test_stream_gpu import _compose

    from robomanipbaselines_amd.bin import Replay
    from robomanipbaselines_amd.common.image_io import decode_png

    steps, mid, cams = 90, (40, 85), ("front", "hand")
    trace, images = str(tmp_path / "trace"), str(tmp_path / "images")
    ro = _compose("Mlp")(argv=["--num_envs", "2", "--device", DEV, "--world_idx_list", "1", "4", "--max_steps", str(steps),
                               "--save_last_image", "--output_image_dir", images, "--trace_dir", trace,
                               "--shadows", shadows, "--offsamples", offsamples])
    assert ro.env.renderer.shadows == (shadows == "scene") and ro.env.renderer.samples == int(offsamples)
    assert ro.run() == steps
    reader = ET.TraceReader(trace)
    assert (reader.header["shadows"], reader.header["offsamples"]) == (shadows, offsamples)
    assert reader.header["image_size"] == [480, 640] and reader.header["camera_names"] == ["front", "side", "hand"]
    assert mid[1] > ro._phase_entry_steps()[-1] > mid[0]  # one step of the pre-motion, one of the rollout
    # (a) --steps last of each episode is the PNG --save_last_image wrote
    for e in range(2):
        (live,) = glob.glob(os.path.join(images, f"*_world{(1, 4)[e]}_failure_*_env{e}.png"))
        (path,) = Replay.main([trace, "--episode", str(e), "--steps", "last", "--output_image_dir", str(tmp_path / "replay")])
        assert os.path.basename(path) == f"RolloutMlp_MujocoUR5eCable_world{(1, 4)[e]}_failure_ep{e}_step{steps}.png"
        with open(live, "rb") as f, open(path, "rb") as g:
            a, b = decode_png(f.read()), decode_png(g.read())
        assert a.shape == b.shape == (480, 3 * 640, 3) and a.tobytes() == b.tobytes(), f"episode {e}: last frame differs"
    # (b) the same rollout stepped by hand: the frames of two cameras at two mid-episode steps
    ro.args.trace_dir, ro.args.save_last_image = None, False
    ro.reset()
    live = {}
    for k in range(1, mid[1] + 1):
        ro.step_once()
        if k in mid:
            live[k] = torch.cat([ro.info["rgb_images"][c] for c in cams], dim=2).cpu().numpy()
    renderer = Replay.make_renderer(reader.header, DEV)  # the header's shadows / offsamples
    assert renderer.shadows == (shadows == "scene") and renderer.samples == int(offsamples)
    for e in range(2):
        rows = reader.episode(e)
        assert rows["step"].tolist() == list(range(1, steps + 1)) and not rows["flags"].any()
        got = Replay.render_rows(renderer, rows, Replay.select_rows(rows, [str(k) for k in mid]), list(cams), DEV)
        for j, k in enumerate(mid):
            assert got[j].tobytes() == live[k][e].tobytes(), f"episode {e}, step {k}: replay differs from the live frame"
        # in batches of one step (a long episode is drawn in several batches): the same pixels
        one = Replay.render_rows(renderer, rows, Replay.select_rows(rows, [str(k) for k in mid]), list(cams), DEV,
                                 batch_bytes=1)
        assert one.tobytes() == got.tobytes()
    if shadows == "scene":
        # the settings matter: the header's are not the defaults' pixels
        plain = Replay.make_renderer(reader.header, DEV, shadows="off", offsamples="1")
        rows = reader.episode(0)
        other = Replay.render_rows(plain, rows, Replay.select_rows(rows, [str(mid[0])]), list(cams), DEV)
        assert other[0].tobytes() != live[mid[0]][0].tobytes()


# -- 6. CLI ---------------------------------------------------------------------------------------
def test_cli_trace_and_replay(tmp_path, capsys):
    from robomanipbaselines_amd.bin import Replay
    from robomanipbaselines_amd.bin.Rollout import main
    from robomanipbaselines_amd.common.image_io import decode_png

    d = str(tmp_path / "D")
    ro = main(["Sarnn", "MujocoUR5eCable", "--num_envs", "2", "--num_episodes", "5", "--world_idx_list", "0", "1", "2",
               "--max_duration", "0.3", "--trace_dir", d])
    out = capsys.readouterr().out
    assert "Episode trace:" in out and "bytes per row" in out
    r = ET.TraceReader(d)
    assert r.traced_episodes == [0, 1, 2, 3, 4] and r.episodes.tobytes() == ro.episode_records.tobytes()
    assert r.header["policy"] == "Sarnn" and r.header["num_slots"] == 2
    for i in range(5):
        rows = r.episode(i)
        assert rows["step"].tolist() == list(range(1, len(rows["step"]) + 1)) and rows["flags"][-1] & ET.FLAG_DONE
        assert rows["rollout_time_idx"][-1] == ro.episode_records["rollout_time_idx"][i]
    last = int(r.episode(3)["step"][-1])
    paths = Replay.main([d, "--episode", "3", "--steps", "1", "50", "last", "--cameras", "front", "side",
                         "--output_image_dir", str(tmp_path / "png")])
    outcome = "success" if ro.episode_records["success"][3] else "failure"
    assert [os.path.basename(p) for p in paths] == [f"RolloutSarnn_MujocoUR5eCable_world0_{outcome}_ep3_step{k}.png"
                                                    for k in (1, 50, last)]
    with open(paths[-1], "rb") as f:
        img = decode_png(f.read())
    assert img.shape == (480, 2 * 640, 3) and len(np.unique(img)) > 10
    (single,) = Replay.main([d, "--episode", "3", "--output_image_dir", str(tmp_path / "png1")])
    assert single.endswith(f"_ep3_step{last}.png")
    with pytest.raises(ValueError, match="were not recorded"):
        Replay.main([d, "--episode", "3", "--steps", str(last + 1)])
