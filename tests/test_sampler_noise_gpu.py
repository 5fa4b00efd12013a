"""The per-episode sampler noise on the device (include/rmbx.h, rmbx_philox_normal): the kernel
against the numpy restatement (tests/philox_cases.py), its independence of the batch layout, its
bounds, the diffusion samplers with a noise source, and DiffusionPolicy / DP3 episodes that consume
the same noise streamed, in lockstep and in shards."""

import functools

import numpy as np
import pytest
import torch

import philox_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

NS, LS, PLANES, SEEDS = (1, 5, 300), (4, 21, 112), ((0, 1), (1, 3), (1, 99)), (0, 3, 2**40 + 7)
CANARY, GUARD = 0x5A5A5A5A, 64
# |device f32 - restatement f64| of a normal: r <= 5.77 and logf / sqrtf / sincospif at <= 2 ulp
# each with an exact sincospi argument give about 2.4e-6; the bar leaves a 1.7x margin
NORMAL_BAR = 4e-6


def _rows(n, shift):
    """episodes with -1, 0 and 2^31 - 1, draws with 0 and 2^31 - 1; `shift` rotates which of them a
    one-row batch gets."""
    ep = np.roll(np.array([-1, 0, 2**31 - 1, 4117, 7], dtype=np.int64), -shift)
    dr = np.roll(np.array([0, 2**31 - 1, 1, 2], dtype=np.int64), -shift)
    return np.resize(ep, n).astype(np.int32), np.resize(dr, n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _want_words(seed, n, shift, L, plane0, nplane):
    ep, dr = _rows(n, shift)
    w = PC.words_batch(seed, ep, dr, plane0, nplane, L)
    w.setflags(write=False)
    return w


def _launch(seed, ep, dr, plane0, nplane, L, words, offset=0):
    """The kernel into a guarded buffer, `offset` elements (4 bytes each) off a 16-byte boundary.
    Returns (values [nplane, n, row] as numpy, canary intact)."""
    from robomanipbaselines_amd import kernels as K

    n = len(ep)
    row = 4 * ((L + 3) // 4) if words else L
    numel = nplane * n * row
    buf = torch.full((GUARD + offset + numel + GUARD,), CANARY, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + offset: GUARD + offset + numel].view(nplane, n, row)
    e, d = torch.from_numpy(ep).to(DEV), torch.from_numpy(dr).to(DEV)
    if words:
        K.philox_normal(seed, e, d, view, plane0=plane0, L=L, words=True)
    else:
        K.philox_normal(seed, e, d, view.view(torch.float32), plane0=plane0)
    host = buf.cpu().numpy()
    intact = (host[: GUARD + offset] == CANARY).all() and (host[GUARD + offset + numel:] == CANARY).all()
    vals = host[GUARD + offset: GUARD + offset + numel].reshape(nplane, n, row)
    return (vals.view(np.uint32) if words else vals.view(np.float32)), bool(intact)


@pytest.mark.parametrize("planes", PLANES)
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_words_equal_the_restatement_bitwise(n, L, planes):
    """kind 1, every seed, aligned and 4 bytes off (dword stores): the restatement's words, bit for
    bit, and nothing written outside out."""
    plane0, nplane = planes
    for shift, seed in enumerate(SEEDS):
        ep, dr = _rows(n, shift)
        want = _want_words(seed, n, shift, L, plane0, nplane)
        for offset in (0, 1):
            got, intact = _launch(seed, ep, dr, plane0, nplane, L, True, offset)
            assert intact, (seed, offset)
            assert np.array_equal(got, want), (seed, offset)


@pytest.mark.parametrize("planes", PLANES)
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_normals_follow_the_restatement(n, L, planes):
    """kind 0 against the restatement's f64 normals of the same words: finite, |z| <= 5.78, within
    NORMAL_BAR; the dword-store path (4 bytes off, and the tail of L = 21) writes the same bits; the
    canary stands.  Measured maximum over all cases on the MI355X: 6.6e-7."""
    plane0, nplane = planes
    worst = 0.0
    for shift, seed in enumerate(SEEDS):
        ep, dr = _rows(n, shift)
        want = PC.normals_from_words(_want_words(seed, n, shift, L, plane0, nplane), L)
        got, intact = _launch(seed, ep, dr, plane0, nplane, L, False, 0)
        off, intact_off = _launch(seed, ep, dr, plane0, nplane, L, False, 1)
        assert intact and intact_off, seed
        assert got.tobytes() == off.tobytes(), seed
        assert np.isfinite(got).all() and np.abs(got).max() <= 5.78
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print(f"\nnormals n={n} L={L} planes={planes}: max |device - f64| {worst:.3e}")
    assert worst <= NORMAL_BAR, worst


@pytest.mark.parametrize("words", [True, False])
@pytest.mark.parametrize("L", [21, 112])
def test_a_row_does_not_depend_on_the_layout(L, words):
    """The row of (episode e, draw d): alone, at any position of a 300-row batch, after permuting
    the batch, with the planes split over several calls, 4 bytes off a 16-byte boundary."""
    rng = np.random.default_rng(5)
    n, plane0, nplane, seed = 300, 1, 3, 2**40 + 7
    ep = rng.permutation(100000)[:n].astype(np.int32)
    ep[[0, 17, 299]] = [-1, 0, 2**31 - 1]
    dr = rng.integers(0, 50, n).astype(np.int32)
    dr[[3, 299]] = [2**31 - 1, 0]
    full, intact = _launch(seed, ep, dr, plane0, nplane, L, words)
    assert intact
    for r in (0, 1, 17, 137, 298, 299):  # alone
        one, intact = _launch(seed, ep[r: r + 1], dr[r: r + 1], plane0, nplane, L, words)
        assert intact and one.tobytes() == full[:, r: r + 1].tobytes(), r
    perm = rng.permutation(n)
    got, intact = _launch(seed, ep[perm], dr[perm], plane0, nplane, L, words)
    assert intact and got.tobytes() == full[:, perm].tobytes()
    parts = [_launch(seed, ep, dr, plane0 + k, c, L, words)[0] for k, c in ((0, 1), (1, 2))]
    assert np.concatenate(parts).tobytes() == full.tobytes()
    got, intact = _launch(seed, ep, dr, plane0, nplane, L, words, offset=1)
    assert intact and got.tobytes() == full.tobytes()
    # and the rows differ from one another: neighbours in episode, draw, plane and seed
    assert len({full[0, r].tobytes() for r in range(n)}) == n
    assert full[0].tobytes() != full[1].tobytes()
    assert _launch(seed + 1, ep, dr, plane0, nplane, L, words)[0].tobytes() != full.tobytes()


def test_argument_errors_launch_nothing():
    import ctypes

    from robomanipbaselines_amd import _native as N
    from robomanipbaselines_amd import kernels as K

    n, L = 4, 12
    ep = torch.arange(n, dtype=torch.int32, device=DEV)
    dr = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = torch.full((2, n, L), 7.0, device=DEV)
    lib = N.load()
    ok = dict(episode=ep.data_ptr(), draw=dr.data_ptr(), plane0=0, nplane=2, out=out.data_ptr(), n=n, L=L, kind=0)
    for over in (dict(episode=None), dict(draw=None), dict(out=None), dict(n=0), dict(L=0), dict(L=-1), dict(nplane=0),
                 dict(plane0=-1), dict(kind=2)):
        a = dict(ok)
        a.update(over)
        st = lib.rmbx_philox_normal(ctypes.c_uint64(3), a["episode"], a["draw"], a["plane0"], a["nplane"], a["out"],
                                    a["n"], a["L"], a["kind"], N.stream_ptr())
        assert st == -1, over
        with pytest.raises(ValueError, match="rmbx_philox_normal"):
            N.check(st)
    for kw in (dict(seed=-1), dict(plane0=-1), dict(draw=dr[:3]), dict(episode=ep.long()), dict(out=out[:, :3].contiguous()),
               dict(out=out.double()), dict(out=out, words=True, L=L), dict(episode=ep.cpu())):
        a = dict(seed=3, episode=ep, draw=dr, out=out)
        a.update(kw)
        with pytest.raises(ValueError):
            K.philox_normal(**a)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    K.philox_normal(3, ep, dr, out)
    assert (out != 7.0).all()


# -- the samplers ----------------------------------------------------------------------------------
def _source(B, seed=3, draw0=0):
    ep = np.resize(np.array([4117, -1, 0, 2**31 - 1, 6], dtype=np.int64), B).astype(np.int32)
    dr = (np.resize(np.array([0, 3, 2**31 - 2, 1, 9], dtype=np.int64), B) + draw0).astype(np.int32)
    return (seed, torch.from_numpy(ep).to(DEV), torch.from_numpy(dr).to(DEV)), ep, dr


def _check_planes(x0, noise, seed, ep, dr, L):
    """The filled x0 / noise against the restatement rows of (seed, ep, dr): planes 0 and 1 + k."""
    nn_ = 0 if noise is None else noise.shape[0]
    got = torch.cat([x0[None]] + ([noise] if nn_ else [])).reshape(1 + nn_, len(ep), L).cpu().numpy()
    want = PC.normals_from_words(PC.words_batch(seed, ep, dr, 0, 1 + nn_, L), L)
    assert np.abs(got.astype(np.float64) - want).max() <= NORMAL_BAR
    return got


@torch.no_grad()
@pytest.mark.parametrize("kind", ["dp", "dp3"])
def test_sampler_with_a_noise_source(kind):
    """Small model, B = 5: with a noise source the graph replay equals the eager loop; the same
    (episode, draw) replays bit for bit, draw + 1 does not; what the loop reads (the static buffers
    on the graph path, fresh ones on the eager path) are the restatement's rows; DP3 (DDIM, eta 0)
    takes plane 0 alone."""
    from robomanipbaselines_amd import kernels as K
    from robomanipbaselines_amd.policy.diffusion_policy.dp_model import DiffusionPolicyModel
    from robomanipbaselines_amd.policy.diffusion_policy_3d.dp3_model import DP3Model

    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    torch.manual_seed(0)
    if kind == "dp":
        m = DiffusionPolicyModel(7, 7, 1, crop_hw=(64, 96), down_dims=(64, 128, 256), num_inference_steps=100)
    else:
        m = DP3Model(7, 7, down_dims=(64, 128, 256))
    m = m.eval().requires_grad_(False).to(DEV)
    B, L = 5, 16 * 7
    nn_ = m._n_noise()
    assert nn_ == (99 if kind == "dp" else 0)
    gc = torch.randn(B, m.obs_feature_dim * 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    src, ep, dr = _source(B)
    seen = []
    m.noise_hook = lambda x0, noise: seen.append((x0.clone(), None if noise is None else noise.clone(),
                                                  x0.data_ptr()))
    eager = m.conditional_sample(gc, use_graph=False, noise_source=src).clone()
    graph = m.conditional_sample(gc, use_graph=True, noise_source=src).clone()  # captures, then replays
    again = m.conditional_sample(gc, use_graph=True, noise_source=src).clone()
    assert torch.isfinite(graph).all()
    assert torch.equal(graph, eager) and torch.equal(again, graph)
    g, gcb, xb, nb, out, planes = m._graphs[(B, torch.float32)]
    assert len(seen) == 3 and seen[1][2] == seen[2][2] == xb.data_ptr()  # the static buffers, filled in place
    assert (nb is None) == (nn_ == 0) and planes.shape[0] == 1 + nn_
    first = None
    for x0, noise, _ in seen + [(xb, nb, 0)]:
        got = _check_planes(x0, noise, src[0], ep, dr, L)
        first = got if first is None else first
        assert got.tobytes() == first.tobytes()  # eager and graph paths read the same bits
    # the same bits as the kernel called directly, and its words are the restatement's
    direct = torch.empty((1 + nn_, B, L), device=DEV)
    K.philox_normal(src[0], src[1], src[2], direct)
    assert direct.cpu().numpy().tobytes() == first.tobytes()
    w = torch.empty((1 + nn_, B, L), dtype=torch.int32, device=DEV)
    K.philox_normal(src[0], src[1], src[2], w, L=L, words=True)
    assert np.array_equal(w.cpu().numpy().view(np.uint32), PC.words_batch(src[0], ep, dr, 0, 1 + nn_, L))
    # the next draw of the same episodes is another sample
    src1, _, dr1 = _source(B, draw0=1)
    nxt = m.conditional_sample(gc, use_graph=True, noise_source=src1).clone()
    assert not torch.equal(nxt, graph)
    _check_planes(xb, nb, src1[0], ep, dr1, L)
    assert torch.equal(m.conditional_sample(gc, use_graph=False, noise_source=src1), nxt)
    # a row's sample follows its (episode, draw), not its position: the batch reversed
    rev = torch.arange(B - 1, -1, -1, device=DEV)
    flipped = m.conditional_sample(gc[rev].contiguous(), use_graph=True,
                                   noise_source=(src[0], src[1][rev].contiguous(), src[2][rev].contiguous()))
    print(f"\n{kind}: rows of the reversed batch equal bitwise: {torch.equal(flipped[rev], graph)}; "
          f"max |d| {(flipped[rev] - graph).abs().max().item():.3e}")
    with pytest.raises(ValueError):
        m.conditional_sample(gc, noise_source=src, x0=torch.zeros(B, 16, 7, device=DEV))


@torch.no_grad()
@pytest.mark.parametrize("use_graph", [False, True])
def test_default_noise_path_is_unchanged(use_graph):
    """Without a noise source the sampler draws x0 and then the noise with torch.randn from the
    device's default generator, as before: a seeded call equals the call with those draws passed
    explicitly."""
    from robomanipbaselines_amd.policy.diffusion_policy.dp_model import DiffusionPolicyModel

    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    torch.manual_seed(0)
    m = DiffusionPolicyModel(7, 7, 1, crop_hw=(64, 96), down_dims=(64, 128, 256), num_inference_steps=100)
    m = m.eval().requires_grad_(False).to(DEV)
    B = 5
    gc = torch.randn(B, m.obs_feature_dim * 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    calls = []
    m.noise_hook = lambda *a: calls.append(a)
    torch.manual_seed(11)
    got = m.conditional_sample(gc, use_graph=use_graph).clone()
    torch.manual_seed(11)
    x0 = torch.randn(B, 16, 7, device=DEV)
    noise = torch.randn(m._n_noise(), B, 16, 7, device=DEV)
    want = m.conditional_sample(gc, use_graph=use_graph, x0=x0, noise=noise).clone()
    assert torch.equal(got, want) and not calls
    if use_graph:
        xb, nb = m._graphs[(B, torch.float32)][2:4]
        assert torch.equal(xb, x0) and torch.equal(nb, noise)


# -- rollouts --------------------------------------------------------------------------------------
def _compose(policy):
    from robomanipbaselines_amd.envs.operation.OperationMujocoUR5eCable import OperationMujocoUR5eCable

    if policy == "DiffusionPolicy":
        from robomanipbaselines_amd.policy.diffusion_policy.rollout_diffusion_policy import RolloutDiffusionPolicy as P
    else:
        from robomanipbaselines_amd.policy.diffusion_policy_3d.rollout_diffusion_policy_3d import (
            RolloutDiffusionPolicy3d as P)

    class Rollout(OperationMujocoUR5eCable, P):
        pass

    return Rollout


def _force_success(ro, episode_of_slot, at=0.1):
    """Success is forced from `at` seconds of RolloutPhase on for the episodes with episode % 3 == 1
    (read as the step's reward reads the schedule: before rmbx_sched_update of that step)."""
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


def _hash_rows(x0, noise):
    """i64 [B]: a hash of every row's (x0, noise) bytes, on the device."""
    planes = x0[None] if noise is None else torch.cat([x0[None], noise])
    bits = planes.reshape(planes.shape[0], planes.shape[1], -1).view(torch.int32).to(torch.int64)
    P, _, L = bits.shape
    k = torch.arange(P * L, dtype=torch.int64, device=bits.device).view(P, 1, L)
    weight = (k * 0x1E3779B97F4A7C15 + 0x632BE59BD9B4E019) | 1  # wraps mod 2^64: fixed odd weights
    return ((bits + 0x1234567) * weight).sum(dim=(0, 2))


def _log_fills(ro, log):
    """Record (episode, draw, in RolloutPhase, row hashes) of every fill of ro's sampler, as device
    tensors (no host sync in the run)."""
    n_pre = len(ro.pre_durations)

    def hook(x0, noise):
        _, episode, draw = ro._noise_source()
        if ro.args.num_episodes is not None:
            live = ro.stream.phase == n_pre
        else:
            live = torch.ones(ro.n, dtype=torch.bool, device=x0.device)
        log.append((episode.clone(), draw.clone(), live.clone(), _hash_rows(x0, noise)))

    ro.policy.noise_hook = hook


def _by_episode(log):
    """{episode: [(draw, hash), ...] in call order} over the rows that were in RolloutPhase."""
    out = {}
    for episode, draw, live, h in log:
        episode, draw, live, h = (t.cpu().numpy() for t in (episode, draw, live, h))
        for r in range(len(episode)):
            if live[r]:
                out.setdefault(int(episode[r]), []).append((int(draw[r]), int(h[r])))
    return out


@pytest.mark.parametrize("policy", ["DiffusionPolicy", "DiffusionPolicy3d"])
def test_streamed_episodes_equal_lockstep_episodes(policy):
    """--sampler_noise episode: 7 episodes streamed through 3 slots, then the same episodes as
    three lockstep runs at --env_offset 0, 3, 6 (same object, same weights).  Per episode: every
    inference consumed the same (x0, noise) bytes, with the draw counter 0, 1, 2, ...; the records
    and the final qpos are equal bit for bit."""
    from robomanipbaselines_amd import kernels as K

    n, M = 3, 7
    ro = _compose(policy)(argv=["--num_envs", str(n), "--num_episodes", str(M), "--device", DEV, "--max_duration", "1.6",
                                "--world_idx_list", "0", "1", "2", "3", "4", "5", "--world_random_scale", "0.01", "0.01",
                                "0.0", "--seed", "3", "--precision", "fp32", "--skip", "6", "--sampler_noise", "episode"])
    assert ro.n == n and ro.stream_period == 6 * ro.n_action_steps
    P = ro.stream_period
    ro.record_final_qpos = True
    offset = [0]
    _force_success(ro, lambda: (ro.slot_episode if ro.args.num_episodes is not None
                                else offset[0] + torch.arange(n, dtype=torch.int32, device=DEV)))
    streamed_log = []
    _log_fills(ro, streamed_log)
    ro.run()
    rec = ro.episode_records
    final = ro.stream.final_qpos.cpu().numpy()
    assert len(ro.result["success"]) == M and rec["episode"].tolist() == list(range(M))
    assert len(set(rec["slot"].tolist())) > 1
    streamed = _by_episode(streamed_log)
    assert sorted(e for e in streamed if e >= 0) == list(range(M))
    print(f"\n{policy}: slots {rec['slot'].tolist()} steps {rec['rollout_time_idx'].tolist()} "
          f"inferences {[len(streamed[i]) for i in range(M)]}")
    ro.args.num_episodes = None
    qpos_equal = []
    for off in (0, 3, 6):
        offset[0] = off
        ro.args.env_offset = ro.env.env_offset = off
        lock_log = []
        _log_fills(ro, lock_log)
        ro.run()
        lock = _by_episode(lock_log)
        v = K.sched_view(ro.sched)
        qpos = ro.env.engine.qpos.cpu().numpy()
        for e in range(n):
            i = off + e
            if i >= M:
                continue
            # the noise: the streamed episode's inferences count 0, 1, 2, ... and each read the bytes
            # the lockstep env read at that count
            draws = [d for d, _ in streamed[i]]
            assert draws == list(range(len(draws))) and len(draws) >= -(-int(rec["rollout_time_idx"][i]) // P) >= 1, i
            assert [d for d, _ in lock[i]][: len(draws)] == draws, i
            assert [h for _, h in lock[i]][: len(draws)] == [h for _, h in streamed[i]], f"episode {i}: noise differs"
            # the records
            assert rec["world_idx"][i] == ro.world_idx[e] == i % 6
            assert bool(rec["success"][i]) == bool(v["success"][e]) == (i % 3 == 1), i
            assert rec["reward"][i] == v["result_reward"][e], i
            assert rec["duration"][i] == v["duration"][e], i
            assert rec["rollout_time_idx"][i] == v["rollout_time_idx"][e], i
            qpos_equal.append(final[i].tobytes() == qpos[e].tobytes())
    print(f"{policy}: final qpos equal to lockstep, per episode: {qpos_equal}")
    assert all(qpos_equal), f"final qpos differs from lockstep: {qpos_equal}"
    assert rec["rollout_time_idx"][1] < rec["rollout_time_idx"][0]


def test_the_mode_is_printed_and_written_into_the_trace_header(tmp_path, capsys):
    """A re-run must ask for the noise the traced run had: header.json carries sampler_noise (both
    modes), and the rollout prints it when the policy is set up."""
    import json

    argv = ["--num_envs", "2", "--device", DEV, "--world_idx_list", "0", "1", "--max_duration", "0.1", "--skip", "6",
            "--trace_stride", "6"]
    ro = _compose("DiffusionPolicy3d")(argv=argv + ["--trace_dir", str(tmp_path / "b")])
    assert "[Rollout] Sampler noise: batch" in capsys.readouterr().out
    ro.reset()
    assert ro._trace.header["sampler_noise"] == "batch"
    ro._trace.abort()
    ro = _compose("DiffusionPolicy3d")(argv=argv + ["--trace_dir", str(tmp_path / "e"), "--sampler_noise", "episode"])
    assert "[Rollout] Sampler noise: episode" in capsys.readouterr().out
    ro.run()
    with open(tmp_path / "e" / "header.json") as f:
        header = json.load(f)
    assert header["sampler_noise"] == "episode" and header["policy"] == "DiffusionPolicy3d" and header["seed"] == 0


@pytest.mark.parametrize("policy", ["DiffusionPolicy", "DiffusionPolicy3d"])
def test_shards_read_the_same_noise(policy):
    """One lockstep run of 4 envs against two of 2 at --env_offset 0, 2: the first inference's
    (x0, noise) rows are equal bit for bit per episode.  Whether the actions are too (another batch
    size: other GEMM routes) is printed, not asserted (Streaming)."""
    argv = ["--device", DEV, "--world_idx_list", "0", "1", "2", "3", "--world_random_scale", "0.01", "0.01", "0.0",
            "--seed", "3", "--precision", "fp32", "--sampler_noise", "episode"]

    def first_inference(ro, off):
        ro.args.env_offset = ro.env.env_offset = off
        got = {}
        ro.policy.noise_hook = lambda x0, noise: got.setdefault(
            "planes", (x0[None] if noise is None else torch.cat([x0[None], noise])).clone())
        inner = ro.policy.predict_action

        def spy(*a, **k):
            got["episode"] = k["noise_source"][1].clone()
            got["draw"] = k["noise_source"][2].clone()
            got["chunk"] = inner(*a, **k).clone()
            return got["chunk"]

        ro.policy.predict_action = spy
        ro.reset()
        for _ in range(2000):
            ro.step_once()
            if "chunk" in got:
                break
        ro.policy.predict_action = inner
        assert got["draw"].tolist() == [0] * ro.n and got["episode"].tolist() == list(range(off, off + ro.n))
        return got["planes"].cpu().numpy(), got["chunk"].float().cpu().numpy()

    whole = _compose(policy)(argv=argv + ["--num_envs", "4"])
    half = _compose(policy)(argv=argv + ["--num_envs", "2"])
    half.policy.load_state_dict(whole.policy.state_dict())
    planes4, chunk4 = first_inference(whole, 0)
    same, worst = True, 0.0
    for off in (0, 2):
        planes2, chunk2 = first_inference(half, off)
        assert planes2.tobytes() == planes4[:, off: off + 2].tobytes(), off
        same &= chunk2.tobytes() == chunk4[off: off + 2].tobytes()
        worst = max(worst, float(np.abs(chunk2 - chunk4[off: off + 2]).max()))
    assert np.isfinite(chunk4).all()
    print(f"\n{policy}: 4 envs vs 2 + 2: first action chunks equal bitwise: {same}; max |d| {worst:.3e}")
