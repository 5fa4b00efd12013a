"""The per-episode actuation perturbation on the device (include/rmbx.h, rmbx_action_perturb): the
kernel against the numpy restatement fed with the device's own normals (bitwise) and against the
independent loop-written oracle (tests/actuation_cases.py), its independence of the batch, masks and
argument errors; then --actuation in the lockstep rollouts, shards and the streaming loop, with the
policy replaced by a scripted one so that the closed loop does not enter the expectation."""

import ctypes
import functools
import json

import numpy as np
import pytest
import torch
import yaml

import actuation_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1234.5  # what out holds where the kernel must not write
T = AC.T


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _spec(comp, D):
    from robomanipbaselines_amd.common.actuation import ActuationSpec

    return ActuationSpec(delay=D, **{k: AC.f32(v) for k, v in AC.COMPONENTS[comp].items()})


def _device(spec, skip, bs, ns, ep, r, acts, mask_in=None, seed=AC.SEED, ring_fill=AC.RING_FILL):
    """The kernel over the steps of a case: out f64 [T, n, A] (SENTINEL where it did not write), mask
    u8 [T, n], the final ring, and one guard row past the end of out, mask and ring (all buffers are
    allocated one row longer and must keep their fill there).  r i32 [T, n]."""
    from robomanipbaselines_amd import kernels as K

    steps, n, A = acts.shape
    D = spec.delay
    ring = torch.full((n + 1, D + 1, A), ring_fill, dtype=torch.float64, device=DEV)
    out = torch.full((steps, n + 1, A), SENTINEL, dtype=torch.float64, device=DEV)
    mask = torch.full((steps, n + 1), 77, dtype=torch.uint8, device=DEV)
    a, e, rr = _t(acts), _t(np.broadcast_to(ep, (steps, n))), _t(r.astype(np.int32))
    m = None if mask_in is None else _t(mask_in)
    b, s = _t(bs), _t(ns)
    for t in range(steps):
        K.action_perturb(a[t], seed, e[t], rr[t], ring[:n], b, s, out[t, :n], mask[t, :n], noise=spec.noise,
                         bias=spec.bias, delay=D, hold=spec.hold, skip=skip, mask_in=None if m is None else m[t])
    torch.cuda.synchronize()
    out, mask, ring = out.cpu().numpy(), mask.cpu().numpy(), ring.cpu().numpy()
    assert (out[:, n] == SENTINEL).all() and (mask[:, n] == 77).all()
    assert np.array_equal(ring[n], np.full_like(ring[n], ring_fill), equal_nan=True)
    return out[:, :n], mask[:, :n], ring[:n]


def _normals(ep, r, skip, A, seed=AC.SEED):
    """The device's own normals of the NOISE plane at the draws r - r % skip: f32 [T, n, A]."""
    from robomanipbaselines_amd import kernels as K

    steps, n = r.shape
    z = torch.empty((1, steps * n, A), dtype=torch.float32, device=DEV)
    draw = (r - r % skip).astype(np.int32).reshape(-1)
    K.philox_normal(seed, _t(np.broadcast_to(ep, (steps, n)).reshape(-1)), _t(draw), z, plane0=AC.PLANE_NOISE)
    return z[0].reshape(steps, n, A).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(n, A, D, skip, comp):
    """The inputs of a case and what the device made of them, computed once."""
    spec = _spec(comp, D)
    acts = AC.actions(n, A)
    scale, bs, ns = AC.scale_arrays(A, spec.noise, spec.bias)
    ep, r0 = AC.EPISODES[:n], AC.R0[:n]
    r = (r0[None, :] + np.arange(T)[:, None]).astype(np.int32)
    out, mask, ring = _device(spec, skip, bs, ns, ep, r, acts)
    return spec, acts, bs, ns, ep, r0, r, out, mask, ring


def _same(out, mask, want, wmask, what):
    """out equals want bit for bit where something arrives, and holds SENTINEL where nothing does."""
    assert mask.tolist() == wmask.tolist(), what
    arrived = mask != 0
    assert out[arrived].tobytes() == want[arrived].tobytes(), (what, int((out[arrived] != want[arrived]).sum()))
    assert (out[~arrived] == SENTINEL).all(), what


SHAPES = [(n, A) for n in AC.NS for A in AC.AS]


# -- 1. identity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, A", SHAPES)
def test_zero_spec_is_the_identity(n, A):
    from robomanipbaselines_amd.common.actuation import ActuationSpec

    acts = AC.actions(n, A)
    scale, bs, ns = AC.scale_arrays(A)
    r = (AC.R0[None, :n] + np.arange(T)[:, None]).astype(np.int32)
    mask_in = (np.random.default_rng(3).random((T, n)) < 0.7).astype(np.uint8)
    for skip in AC.SKIPS:
        out, mask, _ = _device(ActuationSpec(), skip, bs, ns, AC.EPISODES[:n], r, acts)
        assert out.tobytes() == acts.tobytes() and (mask == 1).all()
        out, mask, _ = _device(ActuationSpec(), skip, bs, ns, AC.EPISODES[:n], r, acts, mask_in=mask_in)
        assert mask.tobytes() == mask_in.tobytes()
        assert out[mask != 0].tobytes() == acts[mask != 0].tobytes() and (out[mask == 0] == SENTINEL).all()


# -- 2. exact against the restatement with the device's normals; the oracle with the host's ---------------
@pytest.mark.parametrize("comp", list(AC.COMPONENTS))
@pytest.mark.parametrize("n, A", SHAPES)
def test_exact_against_the_restatement_with_device_normals(n, A, comp):
    from robomanipbaselines_amd.common import actuation as ACT

    for D in AC.DS:
        for skip in AC.SKIPS:
            spec, acts, bs, ns, ep, r0, r, out, mask, ring = _case(n, A, D, skip, comp)
            z32 = _normals(ep, r, skip, A) if spec.noise != 0 else None
            host_ring = np.full((n, D + 1, A), AC.RING_FILL)
            want, wmask = ACT.restate(spec, AC.SEED, skip, bs, ns, ep, r, acts, z32=z32, ring=host_ring)
            _same(out, mask, want, wmask, (D, skip))
            assert ring.tobytes() == host_ring.tobytes(), (D, skip)
            # and the loop-written oracle fed the same normals
            want, wmask = AC.oracle(AC.SEED, skip, bs, ns, ep, r0, acts, noise=spec.noise, bias=spec.bias, delay=D,
                                    hold=spec.hold, z32=z32)
            _same(out, mask, want, wmask, (D, skip, "oracle"))
            if comp == "all" and n == 5:  # the case does something: lost packets, late commands, other values
                assert 0 < mask.sum() < (r >= D).sum() and not np.array_equal(out[-1], acts[-1])


@pytest.mark.parametrize("comp", ["noise", "all"])
@pytest.mark.parametrize("n, A", SHAPES)
def test_against_the_independent_oracle(n, A, comp):
    """Against the oracle with its own f64 Box-Muller normals the mask is equal and an element differs
    by at most ns_k x the bar the philox tests hold the device normals to (plus the f64 roundings):
    AC.tolerance.  The bar is not widened here."""
    worst = 0.0
    for D in AC.DS:
        for skip in AC.SKIPS:
            spec, acts, bs, ns, ep, r0, r, out, mask, ring = _case(n, A, D, skip, comp)
            want, wmask = AC.oracle(AC.SEED, skip, bs, ns, ep, r0, acts, noise=spec.noise, bias=spec.bias, delay=D,
                                    hold=spec.hold, normals="f64")
            assert mask.tolist() == wmask.tolist(), (D, skip)
            arrived = mask != 0
            err = np.abs(np.where(arrived[..., None], out - np.where(arrived[..., None], want, 0.0), 0.0))
            rel = (err / AC.tolerance(acts, bs, ns)).max()
            worst = max(worst, float(rel))
            assert rel <= 1.0, (D, skip, rel)
    print(f"\nn={n} A={A} {comp}: max |device - oracle| / tolerance {worst:.3f}")


# -- 3. the noise is the NOISE plane's, held over the skip steps ------------------------------------------
@pytest.mark.parametrize("A", AC.AS)
def test_noise_is_philox_normal_and_held_over_the_skip_steps(A):
    """With a zero action, unit scale and strength 1 (ns = 1.0) the output is (double)z: bit for bit
    rmbx_philox_normal's element k of a row of length A at (seed, episode, r - r % skip, NOISE plane)."""
    from robomanipbaselines_amd.common.actuation import ActuationSpec

    n, skip = 5, 3
    r = (AC.R0[None, :] + np.arange(T)[:, None]).astype(np.int32)
    acts, one = np.zeros((T, n, A)), np.ones(A)
    out, mask, _ = _device(ActuationSpec(noise=1.0), skip, one, one, AC.EPISODES, r, acts)
    z = _normals(AC.EPISODES, r, skip, A)
    assert (mask == 1).all() and out.tobytes() == z.astype(np.float64).tobytes()
    for i in range(n):
        for t in range(1, T):
            held = r[t, i] // skip == r[t - 1, i] // skip
            assert np.array_equal(out[t, i], out[t - 1, i]) == held, (i, t)
    # skip 1: a new draw at every step
    out1, _, _ = _device(ActuationSpec(noise=1.0), 1, one, one, AC.EPISODES, r, acts)
    assert out1.tobytes() == _normals(AC.EPISODES, r, 1, A).astype(np.float64).tobytes()
    assert all(not np.array_equal(out1[t], out1[t - 1]) for t in range(1, T))


# -- 4. a row does not depend on the batch ----------------------------------------------------------------
@pytest.mark.parametrize("A", [5, 8])
def test_a_row_does_not_depend_on_n_slot_or_neighbours(A):
    D, skip = 3, 3
    spec, acts, bs, ns, ep, r0, r, full, fmask, fring = _case(5, A, D, skip, "all")
    perm = np.array([3, 0, 4, 2, 1])
    out, mask, ring = _device(spec, skip, bs, ns, ep[perm], r[:, perm], acts[:, perm])
    assert out.tobytes() == full[:, perm].tobytes() and mask.tobytes() == fmask[:, perm].tobytes()
    assert ring.tobytes() == fring[perm].tobytes()
    for i in (0, 3):
        out, mask, ring = _device(spec, skip, bs, ns, ep[i:i + 1], r[:, i:i + 1], acts[:, i:i + 1])
        assert out.tobytes() == full[:, i:i + 1].tobytes() and mask.tobytes() == fmask[:, i:i + 1].tobytes(), i
    out, mask, _ = _device(spec, skip, bs, ns, ep[1:3], r[:, 1:3], acts[:, 1:3])
    assert out.tobytes() == full[:, 1:3].tobytes() and mask.tobytes() == fmask[:, 1:3].tobytes()
    # another episode or seed: another result
    other, _, _ = _device(spec, skip, bs, ns, ep + 1, r, acts)
    assert other.tobytes() != full.tobytes()
    other, _, _ = _device(spec, skip, bs, ns, ep, r, acts, seed=AC.SEED + 1)
    assert other.tobytes() != full.tobytes()


# -- 5. inactive rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 7])
def test_inactive_rows_write_nothing(A):
    """Rows 1 and 2 are inactive at every step: their out and ring keep the fill, their mask_out is 0
    (the rule's step 7; mask_in itself is not written), the active rows are what they are in a batch
    of their own, and the row past the end of every buffer keeps its fill (_device asserts it)."""
    D, skip, n = 3, 3, 5
    spec, acts, bs, ns, ep, r0, r, full, fmask, fring = _case(n, A, D, skip, "all")
    mask_in = np.ones((T, n), np.uint8)
    mask_in[:, 1:3] = 0
    keep = _t(mask_in)
    out, mask, ring = _device(spec, skip, bs, ns, ep, r, acts, mask_in=mask_in)
    live = [0, 3, 4]
    assert out[:, live].tobytes() == full[:, live].tobytes() and mask[:, live].tobytes() == fmask[:, live].tobytes()
    assert ring[live].tobytes() == fring[live].tobytes()
    assert (out[:, 1:3] == SENTINEL).all() and (ring[1:3] == AC.RING_FILL).all() and not mask[:, 1:3].any()
    assert keep.cpu().numpy().tobytes() == mask_in.tobytes()
    # a row that becomes active at its r = 0, as a recycled slot does, needs no reset of its ring
    late = np.ones((T, n), np.uint8)
    late[:4, 0] = 0
    r2 = r.copy()
    r2[:, 0] = np.maximum(np.arange(T) - 4, 0)
    out, mask, _ = _device(spec, skip, bs, ns, ep, r2, acts, mask_in=late, ring_fill=np.nan)
    from robomanipbaselines_amd.common import actuation as ACT

    z32 = _normals(ep, r2, skip, A)
    want, wmask = ACT.restate(spec, AC.SEED, skip, bs, ns, ep, r2, acts, mask_in=late, z32=z32,
                              ring=np.full((n, D + 1, A), np.nan))
    assert mask.tolist() == wmask.tolist() and not mask[:4 + D, 0].any()
    assert out[mask != 0].tobytes() == want[mask != 0].tobytes()
    assert not np.isnan(out[:, 0][mask[:, 0] != 0]).any()  # nothing from before the episode arrives


# -- 6. argument errors -------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from robomanipbaselines_amd import _native as N
    from robomanipbaselines_amd import kernels as K

    n, A, D = 3, 5, 2
    f64 = dict(dtype=torch.float64, device=DEV)
    action = torch.full((n, A), 0.5, **f64)
    out = torch.full((n + 1, A), SENTINEL, **f64)
    ring = torch.full((n + 1, D + 1, A), AC.RING_FILL, **f64)
    mask = torch.full((n + 1,), 77, dtype=torch.uint8, device=DEV)
    bs, ns = torch.full((A,), 0.1, **f64), torch.full((A,), 0.2, **f64)
    ep = torch.arange(n, dtype=torch.int32, device=DEV)
    r = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    lib = N.load()

    def params(**over):
        v = dict(noise=0.3, bias=0.2, hold=0.4, delay=D, skip=3)
        v.update(over)
        return N.ActuationParams(v["noise"], v["bias"], v["hold"], v["delay"], v["skip"])

    ok = dict(action=action.data_ptr(), out=out.data_ptr(), mask_out=mask.data_ptr(), ring=ring.data_ptr(), p=params(),
              bs=bs.data_ptr(), ns=ns.data_ptr(), episode=ep.data_ptr(), r=r.data_ptr(), n=n, A=A)
    inf, nan = float("inf"), float("nan")
    bad = [dict(action=None), dict(out=None), dict(mask_out=None), dict(ring=None), dict(p=None), dict(bs=None),
           dict(ns=None), dict(episode=None), dict(r=None), dict(n=0), dict(n=-1), dict(A=0), dict(A=-3),
           dict(p=params(delay=65)), dict(p=params(delay=-1)), dict(p=params(skip=0)), dict(p=params(skip=-2)),
           dict(p=params(noise=-1.0)), dict(p=params(noise=inf)), dict(p=params(noise=nan)), dict(p=params(bias=-0.5)),
           dict(p=params(bias=inf)), dict(p=params(bias=nan)), dict(p=params(hold=1.0)), dict(p=params(hold=-0.1)),
           dict(p=params(hold=nan)), dict(n=2**20, A=2**10, p=params(delay=1)), dict(out=action.data_ptr()),
           dict(out=action.data_ptr() + 8 * A), dict(out=ring.data_ptr() + 8), dict(ring=action.data_ptr()),
           dict(action=action.data_ptr() + 4), dict(episode=ep.data_ptr() + 2)]
    for over in bad:
        a = dict(ok)
        a.update(over)
        st = lib.rmbx_action_perturb(a["action"], a["out"], a["mask_out"], a["ring"],
                                     None if a["p"] is None else ctypes.byref(a["p"]), a["bs"], a["ns"], ctypes.c_uint64(3),
                                     a["episode"], a["r"], None, a["n"], a["A"], N.stream_ptr())
        assert st == -1, {k: v for k, v in over.items() if k != "p"}
        with pytest.raises(ValueError, match="rmbx_action_perturb"):
            N.check(st)
    for kw in (dict(seed=-1), dict(seed=2**64), dict(action=action.float()), dict(action=action[0]),
               dict(action=action[:, :0]), dict(action=action.t()), dict(episode=ep[:2]), dict(episode=ep.long()),
               dict(r=r[:2]), dict(r=r.cpu()), dict(ring=ring[:n, :2].contiguous()), dict(ring=ring[:n].float()),
               dict(bias_scale=bs[:4]), dict(noise_scale=ns.float()), dict(out=out[:2]), dict(out=out[:n, :4].contiguous()),
               dict(mask_out=mask[:2]), dict(mask_out=mask[:n].bool()), dict(mask_in=torch.ones(n, device=DEV)),
               dict(mask_in=mask[:2]), dict(delay=65), dict(delay=-1), dict(skip=0)):
        a = dict(action=action, seed=3, episode=ep, r=r, ring=ring[:n], bias_scale=bs, noise_scale=ns, out=out[:n],
                 mask_out=mask[:n], noise=0.3, bias=0.2, delay=D, hold=0.4, skip=3)
        a.update(kw)
        with pytest.raises(ValueError):
            K.action_perturb(**a)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (ring == AC.RING_FILL).all() and (mask == 77).all() and (action == 0.5).all()
    K.action_perturb(action, 3, ep, r, ring[:n], bs, ns, out[:n], mask[:n], noise=0.3, bias=0.2, delay=D, hold=0.0, skip=3)
    assert (mask[:n] == 1).all() and (out[:n] == AC.RING_FILL).all() and (ring[:n] != AC.RING_FILL).any()
    assert (out[n] == SENTINEL).all() and (ring[n] == AC.RING_FILL).all() and int(mask[n]) == 77


# -- rollouts ---------------------------------------------------------------------------------------------
BASE = ["--device", DEV, "--world_random_scale", "0.01", "0.01", "0.0", "--seed", "3", "--precision", "fp32"]
ALL = ["noise=0.05", "bias=0.1", "delay=2", "hold=0.3"]


def _compose(policy):
    from test_stream_gpu import _compose as compose

    return compose(policy)


def _rows_now(ro):
    """(episode i64 [n], r i64 [n], live bool [n]) of the rows at this point of the step, on the host."""
    n = ro.n
    if ro.args.num_episodes is not None:
        return (ro.stream.slot_episode.cpu().numpy().astype(np.int64),
                ro.sched.view(torch.int32)[:, 1].cpu().numpy().astype(np.int64),
                (ro.stream.phase == len(ro.pre_durations)).cpu().numpy())
    return ro.args.env_offset + np.arange(n), np.full(n, int(ro.rollout_time_idx)), np.ones(n, bool)


def _script(ro, relative=False):
    """Replace infer_policy by a scripted policy: the action of a row depends on its (episode, r) only
    -- a joint command near the initial pose, or a small increment."""
    base = np.zeros(ro.action_dim) if relative else np.concatenate([ro.env.init_qpos[:6], [100.0]])[:ro.action_dim]
    step = 2.0**-16 if relative else 2.0**-13  # at most 0.01 / 0.09 rad away

    def action(episode, r):
        return base + step * ((int(episode) % 13) + 1) * (1 + (int(r) % 29)) * (1.0 + np.arange(ro.action_dim) / 8.0)

    def infer():
        episode, r, _ = _rows_now(ro)
        ro.policy_action = _t(np.stack([action(e, t) for e, t in zip(episode, r)]))

    ro.infer_policy = infer
    return action


def _log_commands(ro, log):
    """Log (episode, r, live, q_cmd, grip_cmd) at every env.step of the RolloutPhase: the command state
    the step executes, right after set_command_data / the streaming motion_command."""
    inner, n_pre = ro.env.step, len(ro.pre_durations)

    def step(action, **kw):
        streaming = ro.args.num_episodes is not None
        if streaming or ro.phase_idx == n_pre:
            episode, r, live = _rows_now(ro)
            log.append((episode, r, live, ro.q_cmd.cpu().numpy().copy(), ro.grip_cmd.cpu().numpy().copy()))
        return inner(action, **kw)

    ro.env.step = step


def _lockstep(ro, log, steps):
    """reset, remember the command state the pre-rollout phases leave, and run `steps` rollout steps."""
    ro.reset()
    n_pre, pre = len(ro.pre_durations), None
    for _ in range(1000):
        if ro.phase_idx == n_pre and pre is None:
            pre = (ro.q_cmd.cpu().numpy().copy(), ro.grip_cmd.cpu().numpy().copy())
        ro.step_once()
        if len(log) >= steps:
            return pre
    raise AssertionError("the rollout never reached its RolloutPhase")


def _expected(ro, action, episodes, steps, z_from_device=True):
    """(arrived f64 [steps, n, A], mask u8 [steps, n]): the restatement of the run's spec on the scripted
    actions of the episodes, steps 0 .. steps - 1, with the device's normals."""
    from robomanipbaselines_amd.common import actuation as ACT

    spec, skip, n = ro.actuation_spec, int(ro.args.skip), len(episodes)
    ep = np.asarray(episodes, np.int32)
    r = np.broadcast_to(np.arange(steps, dtype=np.int32)[:, None], (steps, n)).copy()
    acts = np.stack([np.stack([action(e, t - t % skip) for e in episodes]) for t in range(steps)])
    bs, ns = ACT.scales(spec, ro.action_stats())
    z32 = _normals(ep, r, skip, ro.action_dim, seed=int(ro.args.seed)) if spec.noise != 0 else None
    return ACT.restate(spec, int(ro.args.seed), skip, bs, ns, ep, r, acts, z32=z32)


def test_delay_executes_the_command_of_two_steps_ago():
    """7. command_joint_pos, delay=2: q_cmd after set_command_data at step r is bitwise the scripted
    action of step r - 2, and for r < 2 the command the pre-rollout phases left."""
    ro = _compose("Mlp")(argv=BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--env_offset", "3", "--skip", "1",
                                      "--actuation", "delay=2"])
    action, log = _script(ro), []
    _log_commands(ro, log)
    pre_q, pre_g = _lockstep(ro, log, 8)
    assert [int(x[1][0]) for x in log] == list(range(8))
    for episode, r, _, q, g in log:
        for i in range(2):
            if r[i] < 2:
                assert q[i].tobytes() == pre_q[i].tobytes() and g[i].tobytes() == pre_g[i].tobytes(), r[i]
            else:
                want = action(3 + i, r[i] - 2)
                assert q[i].tobytes() == want[:6].tobytes() and float(g[i, 0]) == want[6], (r[i], i)
    assert log[2][3].tobytes() != log[1][3].tobytes() and log[3][3].tobytes() != log[2][3].tobytes()


def test_hold_updates_the_command_on_the_steps_a_packet_arrives():
    """8. hold=0.5: q_cmd changes exactly on the steps the restatement says a packet arrives."""
    ro = _compose("Mlp")(argv=BASE + ["--num_envs", "3", "--world_idx_list", "0", "1", "2", "--env_offset", "5", "--skip", "1",
                                      "--actuation", "hold=0.5"])
    action, log = _script(ro), []
    _log_commands(ro, log)
    steps = 16
    pre_q, _ = _lockstep(ro, log, steps)
    want, mask = _expected(ro, action, [5, 6, 7], steps)
    assert 0 < mask.sum() < mask.size and len({tuple(c) for c in mask.T.tolist()}) == 3  # per episode
    prev = pre_q
    for t in range(steps):
        q = log[t][3]
        for i in range(3):
            assert (q[i].tobytes() != prev[i].tobytes()) == bool(mask[t, i]), (t, i)
            if mask[t, i]:
                assert q[i].tobytes() == want[t, i, :6].tobytes()
        prev = q


def test_relative_increments_follow_the_delayed_skip_phase():
    """9. command_joint_pos_rel, skip 3, delay=1: the increment is added exactly on the steps with
    (r - 1) % 3 == 0, where the command that arrives is the one an inference step made."""
    ro = _compose("Mlp")(argv=BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--skip", "3", "--state_keys",
                                      "measured_joint_pos", "--action_keys", "command_joint_pos_rel", "--actuation", "delay=1"])
    assert ro.action_keys == ["command_joint_pos_rel"] and ro.args.skip == 3
    action, log = _script(ro, relative=True), []
    _log_commands(ro, log)
    steps = 11
    pre_q, _ = _lockstep(ro, log, steps)
    prev = pre_q
    for t in range(steps):
        q = log[t][3]
        for i in range(2):
            if t >= 1 and (t - 1) % 3 == 0:
                made_at = t - 1  # an inference step: its action was scripted for (episode, made_at)
                assert q[i].tobytes() == (prev[i] + action(i, made_at)[:6]).tobytes(), (t, i)
                assert q[i].tobytes() != prev[i].tobytes()
            else:
                assert q[i].tobytes() == prev[i].tobytes(), (t, i)
        prev = q


def test_flag_off_launches_nothing(monkeypatch):
    """10. Without --actuation the kernel wrapper is never called (it is replaced by one that raises),
    there is no Actuator and the result carries no key."""
    from robomanipbaselines_amd import kernels as K

    def refuse(*a, **k):
        raise AssertionError("action_perturb was called without --actuation")

    monkeypatch.setattr(K, "action_perturb", refuse)
    ro = _compose("Mlp")(argv=BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--max_duration", "0.1"])
    assert ro.actuation_spec is None
    calls, inner = [], ro.infer_policy

    def counted():
        calls.append(int(ro.rollout_time_idx))
        assert ro._actuation is None
        inner()

    ro.infer_policy = counted
    ro.run()
    assert len(calls) >= 1 and calls[0] == 0 and ro._actuation is None and "actuation" not in ro.result
    assert len(ro.result["success"]) == 2
    # and with the flag the same wrapper is what runs
    on = _compose("Mlp")(argv=BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--max_duration", "0.1", "--actuation",
                                      "delay=1"])
    with pytest.raises(AssertionError, match="action_perturb was called"):
        on.run()


def _by_key(log):
    out = {}
    for episode, r, live, q, g in log:
        for i in range(len(episode)):
            if live[i]:
                out[(int(episode[i]), int(r[i]))] = q[i].tobytes() + g[i].tobytes()
    return out


def test_streamed_episodes_execute_the_lockstep_commands():
    """11. 4 episodes streamed through 2 slots against the same episodes in lockstep with 4 envs, all
    four keys non-zero: per (episode, r) the executed command state is the same, bit for bit -- the
    ring needs no reset at recycle, and the host's is_skip is every slot's."""
    tail = ["--world_idx_list", "0", "1", "2", "--skip", "3", "--max_duration", "0.4", "--actuation", *ALL]
    st = _compose("Mlp")(argv=BASE + ["--num_envs", "2", "--num_episodes", "4", *tail])
    _script(st)
    slog = []
    _log_commands(st, slog)
    st.run()
    assert st.episode_records["episode"].tolist() == [0, 1, 2, 3] and len(set(st.episode_records["slot"].tolist())) == 2
    streamed = _by_key(slog)
    lk = _compose("Mlp")(argv=BASE + ["--num_envs", "4", *tail])
    action = _script(lk)
    llog = []
    _log_commands(lk, llog)
    lk.run()
    lock = _by_key(llog)
    steps = {e: 1 + max(r for ee, r in streamed if ee == e) for e in range(4)}
    assert all(s >= 9 for s in steps.values()), steps
    assert all((e, r) in streamed for e in range(4) for r in range(steps[e]))
    common = sorted(set(streamed) & set(lock))
    assert all((e, r) in lock for e in range(4) for r in range(steps[e] - 1)), (steps, len(lock))
    differ = [k for k in common if streamed[k] != lock[k]]
    assert not differ, differ[:8]
    # and both are the restatement's: where a command arrives, q_cmd is it
    want, mask = _expected(lk, action, [0, 1, 2, 3], min(steps.values()))
    assert 0 < mask.sum() < mask.size
    for e in range(4):
        for t in range(min(steps.values())):
            if mask[t, e]:
                assert streamed[(e, t)][:48] == want[t, e, :6].tobytes(), (e, t)
            elif t > 0:
                assert streamed[(e, t)] == streamed[(e, t - 1)], (e, t)


def test_shards_execute_the_same_rows():
    """12. One lockstep run of 4 envs against two of 2 at --env_offset 0 and 2: the same executed
    commands, bit for bit."""
    argv = BASE + ["--world_idx_list", "0", "1", "2", "3", "--skip", "3", "--actuation", *ALL]
    whole, wlog = _compose("Mlp")(argv=argv + ["--num_envs", "4"]), []
    _script(whole)
    _log_commands(whole, wlog)
    _lockstep(whole, wlog, 10)
    half = _compose("Mlp")(argv=argv + ["--num_envs", "2"])
    _script(half)
    hlog = []
    _log_commands(half, hlog)
    for off in (0, 2):
        half.args.env_offset = half.env.env_offset = off
        hlog.clear()
        _lockstep(half, hlog, 10)
        for t in range(10):
            assert hlog[t][0].tolist() == [off, off + 1] and int(hlog[t][1][0]) == t
            assert hlog[t][3].tobytes() == wlog[t][3][off:off + 2].tobytes(), (off, t)
            assert hlog[t][4].tobytes() == wlog[t][4][off:off + 2].tobytes(), (off, t)
    assert wlog[9][3][0].tobytes() != wlog[9][3][1].tobytes()


def test_line_result_yaml_and_header_exactly_with_the_flag(tmp_path, capsys):
    """13. The printed line, result["actuation"], the YAML on disk and the trace header are
    spec.as_dict() with the flag, and absent without it."""
    argv = BASE + ["--num_envs", "2", "--world_idx_list", "0", "1", "--max_duration", "0.1", "--trace_stride", "6"]
    off = _compose("Mlp")(argv=argv + ["--trace_dir", str(tmp_path / "off"), "--result_filename", str(tmp_path / "off.yaml")])
    off.run()
    assert "Actuation:" not in capsys.readouterr().out and "actuation" not in off.result
    with open(tmp_path / "off" / "header.json") as f:
        assert "actuation" not in json.load(f)
    with open(tmp_path / "off.yaml") as f:
        assert "actuation" not in yaml.safe_load(f)
    on = _compose("Mlp")(argv=argv + ["--trace_dir", str(tmp_path / "on"), "--result_filename", str(tmp_path / "on.yaml"),
                                      "--actuation", *ALL])
    on.run()
    text = capsys.readouterr().out
    line = "[Rollout] Actuation: noise=0.05 bias=0.1 delay=2 hold=0.3"
    assert text.count(line) == 1 and text.count("Actuation:") == 1
    want = on.actuation_spec.as_dict()
    assert set(want) == {"noise", "bias", "delay", "hold"} and want["delay"] == 2 and want["hold"] == AC.f32(0.3)
    assert on.result["actuation"] == want and "perturb" not in on.result
    with open(tmp_path / "on" / "header.json") as f:
        assert json.load(f)["actuation"] == want
    with open(tmp_path / "on.yaml") as f:
        assert yaml.safe_load(f)["actuation"] == want
    assert len(on.result["success"]) == 2
