"""Host side of the episode trace (--trace_dir), no device: the numpy model of the row rule the GPU
test compares the kernel against, the TraceWriter -> TraceReader round trip on synthetic chunks
(interleaved episodes, two ranks, an empty flush), Replay's argument errors and the flags."""

import json
import os

import numpy as np
import pytest

import trace_cases as TC
from robomanipbaselines_amd.common import episode_trace as ET


# -- the numpy model of the row rule ------------------------------------------------------------
def test_row_rule_model():
    n, dims = 6, TC.DIMS
    st = TC.make_state(n, dims, TC.CTRL_STRIDE, seed=1)
    # slot 2 ends its episode with this step: the schedule moved it past RolloutPhase (`done` itself
    # follows a call later, when the slot no longer steps)
    st["sched"]["done"] = 0
    st["sched"]["phase"] = [0, TC.N_PRE, TC.N_PRE + 1, 1, 2, 3]
    st["sched"]["success"] = [0, 1, 1, 0, 0, 0]
    st["bad_resets"][:] = [0, 0, 1, 0, 1, 0]
    slot_episode = np.array([10, 11, 12, -1, 14, 15], np.int32)
    stepped = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    select = np.ones(8, np.uint8)
    select[5] = 0  # episode 15
    chunk = TC.new_chunk(8, dims)
    te, ts, rows, out = TC.trace_model(st, chunk, 8, dims, slot_episode, stepped, select, episode_base=10, n_episodes=8,
                                       stride=2)
    # slot 3 holds no episode, 4 was not stepped, 5 is not selected: their state is untouched
    assert te.tolist() == [10, 11, 12, -1, -1, -1] and ts.tolist() == [1, 1, 1, 0, 0, 0]
    # step 1 of a stride of 2 writes no row, except for the slot that finished
    assert rows.tolist() == [1, 0]
    assert (out["episode"][0], out["slot"][0], out["step"][0], out["flags"][0]) == (12, 2, 1, 1 | 2 | 4)
    assert out["qpos"][0].tobytes() == st["qpos"][2].tobytes()
    assert out["ctrl"][0].tobytes() == st["ctrl"][2, :dims["nu"]].tobytes()
    assert out["episode"][1] == TC.FILL[np.dtype(np.int32)]
    # second step: k = 2 for the three running slots, in slot order after the first row
    st2 = dict(st, trace_episode=te, trace_step=ts, rows=rows)
    st2["sched"] = st["sched"].copy()
    st2["sched"]["phase"][:] = TC.N_PRE
    st2["sched"]["done"][1] = 1  # closed at once, as rmbx_sched_close_bad does
    te, ts, rows, out = TC.trace_model(st2, out, 8, dims, slot_episode, stepped, select, episode_base=10,
                                       n_episodes=8, stride=2)
    assert rows.tolist() == [4, 0] and out["slot"][:4].tolist() == [2, 0, 1, 2] and out["step"][:4].tolist() == [1, 2, 2, 2]
    assert out["flags"][1:4].tolist() == [0, 1 | 2, 2]
    # a new episode in slot 0 starts at step 1 again
    slot_episode[0] = 16
    st3 = dict(st2, trace_episode=te, trace_step=ts, rows=rows)
    te, ts, rows, out = TC.trace_model(st3, out, 8, dims, slot_episode, stepped, select, episode_base=10,
                                       n_episodes=8, stride=1)
    assert te[0] == 16 and ts.tolist()[:3] == [1, 3, 3]
    assert out["episode"][4:7].tolist() == [16, 11, 12] and out["step"][4:7].tolist() == [1, 3, 3]
    # overflow: rows that fit are written in order, the flag is set, nothing past capacity changes
    st4 = dict(st3, trace_episode=te, trace_step=ts, rows=rows)
    te, ts, rows, out2 = TC.trace_model(st4, out, 8, dims, slot_episode, stepped, select, episode_base=10,
                                        n_episodes=8, stride=1)
    assert rows.tolist() == [8, 1] and out2["slot"][7] == 0 and ts.tolist()[:3] == [2, 4, 4]
    # lockstep form: no slot map, no masks, every slot writes
    te, ts, rows, out = TC.trace_model(st, TC.new_chunk(8, dims), 8, dims, episode_base=3)
    assert rows.tolist() == [6, 0] and out["episode"][:6].tolist() == [3, 4, 5, 6, 7, 8]


def test_row_bytes_of_the_cable_scene():
    d = TC.CABLE_DIMS
    doubles = 2 + d["nu"] + d["nq"] + d["nv"] + 12 * d["ngeom"] + 7 * d["nbody"]
    assert ET.row_bytes(d) == 8 * doubles + 5 * 4 + 1
    assert 13000 < ET.row_bytes(d) < 15000  # "about 14 KB per row"


# -- writer -> reader ---------------------------------------------------------------------------
def _concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in ET.FIELDS}


def test_writer_reader_round_trip(tmp_path):
    d = str(tmp_path / "trace")
    w = ET.TraceWriter(d, TC.header())
    # episodes 4 and 7 interleaved over two chunks; 9 joins in the second; then an empty flush
    c0 = TC.synthetic_rows(TC.DIMS, [4, 7], [1, 2, 3], seed=1)
    c1 = TC.synthetic_rows(TC.DIMS, [4, 9, 7], [4, 5], seed=2)
    c1["step"][c1["episode"] == 9] = [1, 2]
    c1["flags"][-3:] = [ET.FLAG_DONE, ET.FLAG_DONE, ET.FLAG_DONE | ET.FLAG_SUCCESS]
    w.append(c0)
    w.append(None)
    w.append({k: v[:0] for k, v in c0.items()})
    w.append(c1)
    rec = TC.records([4, 7, 9])
    w.finish(rec)
    assert sorted(os.listdir(d)) == ["chunk_000000.npz", "chunk_000001.npz", "episodes.npy", "header.json"]
    with np.load(os.path.join(d, "chunk_000001.npz")) as z:  # the chunk file is the rows it was given
        for k in ET.FIELDS:
            assert z[k].tobytes() == c1[k].tobytes() and z[k].dtype == c1[k].dtype
    with open(os.path.join(d, "header.json")) as f:
        h = json.load(f)
    assert h["format_version"] == ET.FORMAT_VERSION and h["chunks"] == 2 and h["rows"] == 12
    assert h["dims"] == TC.DIMS and h["model_name"] == "ur5e_cable" and h["camera_names"] == ["front", "side", "hand"]
    r = ET.TraceReader(d)
    assert r.traced_episodes == [4, 7, 9]
    assert r.episodes.tobytes() == rec.tobytes() and r.record(7)["duration"] == rec["duration"][1]
    both = _concat([c0, c1])
    for ep, steps in ((4, [1, 2, 3, 4, 5]), (7, [1, 2, 3, 4, 5]), (9, [1, 2])):
        rows = r.episode(ep)
        assert rows["step"].tolist() == steps and (rows["episode"] == ep).all()
        m = both["episode"] == ep
        for k in ET.FIELDS:
            assert rows[k].tobytes() == both[k][m].tobytes(), (ep, k)
    assert r.episode(9)["flags"].tolist() == [0, ET.FLAG_DONE]
    with pytest.raises(ValueError, match="traced episodes: 4, 7, 9"):
        r.episode(5)
    with pytest.raises(ValueError, match="not part of the run"):
        r.record(5)
    # a directory that holds a trace is not written into again
    with pytest.raises(ValueError, match="already holds a trace"):
        ET.TraceWriter(d, TC.header())
    with pytest.raises(RuntimeError):
        w.append(c0)


def test_reader_merges_ranks_and_restores_step_order(tmp_path):
    d = tmp_path / "trace"
    parts = {}
    for rank, eps in ((0, [0, 1, 2]), (1, [3, 4])):
        w = ET.TraceWriter(str(d / f"rank{rank}"), TC.header(rank=rank, world_size=2))
        a = TC.synthetic_rows(TC.DIMS, eps, [3, 6], seed=10 + rank)
        b = TC.synthetic_rows(TC.DIMS, eps[:1], [7], seed=20 + rank)
        w.append(a)
        w.append(b)
        w.finish(TC.records(eps))
        parts[rank] = _concat([a, b])
    r = ET.TraceReader(str(d))
    assert len(r.headers) == 2 and r.header["rank"] == 0
    assert r.episodes["episode"].tolist() == [0, 1, 2, 3, 4] and r.traced_episodes == [0, 1, 2, 3, 4]
    assert r.episode(3)["step"].tolist() == [3, 6, 7] and r.episode(4)["step"].tolist() == [3, 6]
    rows = r.episode(3)
    m = parts[1]["episode"] == 3
    for k in ET.FIELDS:
        assert rows[k].tobytes() == parts[1][k][m].tobytes(), k
    # a trace without its header is not a finished trace
    os.remove(d / "rank1" / "header.json")
    with pytest.raises(ValueError, match="not a finished trace"):
        ET.TraceReader(str(d))


def test_writer_rejects_malformed_rows_and_an_empty_trace_reads(tmp_path):
    w = ET.TraceWriter(str(tmp_path / "a"), TC.header())
    rows = TC.synthetic_rows(TC.DIMS, [0], [1])
    with pytest.raises(ValueError, match="without the fields"):
        w.append({k: v for k, v in rows.items() if k != "xquat"})
    with pytest.raises(ValueError, match="flags"):
        w.append(dict(rows, flags=rows["flags"].astype(np.int32)))
    w.finish(TC.records([0]))
    r = ET.TraceReader(str(tmp_path / "a"))
    assert r.traced_episodes == [] and r.episodes["episode"].tolist() == [0]
    with pytest.raises(ValueError, match="traced episodes: none"):
        r.episode(0)


# -- Replay's argument errors (found before the device is touched) ------------------------------
def _small_trace(tmp_path):
    d = str(tmp_path / "t")
    w = ET.TraceWriter(d, TC.header(stride=3))
    rows = TC.synthetic_rows(TC.DIMS, [2], [3, 6, 9, 10])
    rows["flags"][-1] = ET.FLAG_DONE
    w.append(rows)
    w.finish(TC.records([1, 2]))
    return d


def test_replay_argument_errors(tmp_path):
    from robomanipbaselines_amd.bin import Replay

    d = _small_trace(tmp_path)
    rows = ET.TraceReader(d).episode(2)
    assert Replay.select_rows(rows, ["last"]).tolist() == [3]
    assert Replay.select_rows(rows, ["all"]).tolist() == [0, 1, 2, 3]
    assert Replay.select_rows(rows, ["9", "3"]).tolist() == [2, 0]
    with pytest.raises(ValueError, match=r"recorded steps: 3, 6, 9-10"):
        Replay.select_rows(rows, ["4"])
    # through the command line: a step the stride dropped, a step past the end, an episode that ran
    # but was not traced, an episode the run never had, a camera the scene does not have
    with pytest.raises(ValueError, match=r"step\(s\) \[4\] of episode 2 were not recorded"):
        Replay.main([d, "--episode", "2", "--steps", "4", "--device", "cpu"])
    with pytest.raises(ValueError, match="were not recorded"):
        Replay.main([d, "--episode", "2", "--steps", "3", "11", "--device", "cpu"])
    with pytest.raises(ValueError, match="episode 1 has no rows"):
        Replay.main([d, "--episode", "1", "--device", "cpu"])
    with pytest.raises(ValueError, match="episode 5 is not part of the run"):
        Replay.main([d, "--episode", "5", "--device", "cpu"])
    with pytest.raises(ValueError, match="unknown camera"):
        Replay.main([d, "--episode", "2", "--cameras", "top", "--device", "cpu"])
    with pytest.raises(ValueError, match="--steps takes"):
        Replay.main([d, "--episode", "2", "--steps", "first", "--device", "cpu"])
    assert Replay.image_name(TC.header(), TC.records([1, 2])[0], 7) == "RolloutMlp_MujocoUR5eCable_world1_success_ep1_step7.png"


# -- flags ----------------------------------------------------------------------------------------
def _parse(argv):
    from robomanipbaselines_amd.common.rollout_base import BatchedRolloutBase

    ro = object.__new__(BatchedRolloutBase)
    ro.setup_args(argv=argv)
    return ro.args


def test_flags():
    a = _parse(["--num_envs", "2"])
    assert a.trace_dir is None and a.trace_stride == 1 and ET.parse_episodes(a.trace_episodes) is None
    a = _parse(["--num_envs", "2", "--num_episodes", "9", "--trace_dir", "D", "--trace_episodes", "4", "1", "4",
                "--trace_stride", "3"])
    assert (a.trace_dir, a.trace_stride) == ("D", 3) and ET.parse_episodes(a.trace_episodes) == [1, 4]
    assert ET.parse_episodes(_parse(["--trace_episodes", "all"]).trace_episodes) is None
    with pytest.raises(ValueError):
        _parse(["--trace_stride", "0"])
    with pytest.raises(ValueError):
        _parse(["--trace_episodes", "some"])
    with pytest.raises(ValueError):
        _parse(["--trace_episodes", "-1"])
    # the pinned refusal stays: tracing is how a streamed episode's last frame is had
    with pytest.raises(ValueError, match="save_last_image"):
        _parse(["--num_episodes", "4", "--save_last_image", "--trace_dir", "D"])
    # the select mask of a shard: only its own episodes
    assert ET.select_mask([1, 4, 9], 3, 4).tolist() == [0, 1, 0, 0] and ET.select_mask(None, 0, 4) is None
