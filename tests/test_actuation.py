"""--actuation on the host: the spec parser, the numpy restatement of the rule of include/rmbx.h
(rmbx_action_perturb) in common/actuation.py against the loop-written oracle of
tests/actuation_cases.py, its independence of the batch, the is_skip congruence the streaming call
site relies on, and the loss rate of the hold draw.  No GPU."""

import dataclasses
import math

import numpy as np
import pytest

import actuation_cases as AC
import philox_cases as PC
from robomanipbaselines_amd.common import actuation as A


# -- the parser -----------------------------------------------------------------------------------------
def test_defaults_keys_and_round_trip():
    zero = A.parse_spec([])
    assert zero == A.ActuationSpec() and zero.as_dict() == {"noise": 0.0, "bias": 0.0, "delay": 0, "hold": 0.0}
    s = A.parse_spec(["noise=0.05", "bias=0.1", "delay=2", "hold=0.25"])
    d = s.as_dict()
    assert list(d) == ["noise", "bias", "delay", "hold"]
    assert d == {"noise": AC.f32(0.05), "bias": AC.f32(0.1), "delay": 2, "hold": 0.25}
    assert isinstance(d["delay"], int) and all(isinstance(d[k], float) for k in ("noise", "bias", "hold"))
    assert str(s) == "noise=0.05 bias=0.1 delay=2 hold=0.25"
    assert A.spec_from_dict(d) == s and A.parse_spec(str(s).split()) == s
    assert A.parse_spec("delay=3") == A.ActuationSpec(delay=3)  # one string is one item
    assert A.parse_spec(["hold=0.5", "noise=1e-3"]) == A.ActuationSpec(noise=AC.f32(1e-3), hold=0.5)  # any order
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.delay = 1


def test_values_are_the_f32_the_kernel_reads():
    s = A.parse_spec(["noise=0.1", "bias=0.3", "hold=0.7"])
    for v, text in ((s.noise, 0.1), (s.bias, 0.3), (s.hold, 0.7)):
        assert v == float(np.float32(text)) and v != text


def test_range_edges():
    assert A.parse_spec(["delay=0"]).delay == 0 and A.parse_spec(["delay=64"]).delay == 64
    assert A.parse_spec(["noise=0", "bias=0", "hold=0"]) == A.ActuationSpec()
    assert A.parse_spec(["noise=1e30", "bias=1e30"]).noise == AC.f32(1e30)
    assert A.parse_spec(["hold=0.9999999"]).hold == AC.f32(0.9999999) < 1.0
    for bad in ("delay=65", "delay=-1", "hold=1", "hold=1.0", "hold=-0.1", "noise=-1", "bias=-1e-9", "noise=inf",
                "bias=nan", "noise=1e39", "hold=0.99999999", "noise=-0.0001"):
        with pytest.raises(ValueError, match=r"--actuation: \w+=.* outside \["):
            A.parse_spec([bad])


@pytest.mark.parametrize("items, match", [
    (["gain=0.1"], "unknown key 'gain'; the keys are noise, bias, delay, hold"),
    (["state_noise=0.1"], "unknown key"),
    (["noise=0.1", "noise=0.2"], "noise is given twice"),
    (["delay=1", "hold=0.1", "delay=1"], "delay is given twice"),
    (["noise"], "takes KEY=VALUE, not 'noise'"),
    (["=3"], "takes KEY=VALUE"),
    (["bias="], "takes KEY=VALUE"),
    (["noise=abc"], "noise='abc' is not a number"),
    (["delay=1.5"], "delay='1.5' is not an integer"),
    (["delay=two"], "is not an integer"),
])
def test_error_classes(items, match):
    with pytest.raises(ValueError, match="--actuation.*" + match):
        A.parse_spec(items)


def test_setup_args_refuses_a_bad_spec_before_any_device_work():
    """setup_args raises for a bad --actuation: no env, policy or device has been touched by then."""
    from robomanipbaselines_amd.common.rollout_base import BatchedRolloutBase

    class Bare(BatchedRolloutBase):
        def setup_env(self):
            raise AssertionError("setup_env was reached")

    for bad in (["delay=65"], ["hold=1"], ["speed=2"], ["noise=0.1", "noise=0.1"], ["noise"]):
        with pytest.raises(ValueError, match="--actuation"):
            Bare(argv=["--actuation", *bad])
    with pytest.raises(AssertionError, match="setup_env"):
        Bare(argv=["--actuation", "delay=2"])


# -- the restatement against the loop-written oracle -------------------------------------------------
def _spec(comp, D):
    kw = {k: AC.f32(v) for k, v in AC.COMPONENTS[comp].items()}
    return A.ActuationSpec(delay=D, **kw)


def _both(n, Adim, D, skip, comp, seed=AC.SEED):
    spec = _spec(comp, D)
    acts = AC.actions(n, Adim)
    scale, bs, ns = AC.scale_arrays(Adim, spec.noise, spec.bias)
    ep, r0 = AC.EPISODES[:n], AC.R0[:n]
    r = r0[None, :] + np.arange(AC.T)[:, None]
    ring = np.full((n, D + 1, Adim), AC.RING_FILL)
    got = A.restate(spec, seed, skip, bs, ns, ep, r, acts, ring=ring)
    want = AC.oracle(seed, skip, bs, ns, ep, r0, acts, noise=spec.noise, bias=spec.bias, delay=D, hold=spec.hold)
    return spec, acts, got, want


def test_the_scale_arrays_are_strength_times_scale_in_f64():
    spec = A.parse_spec(["noise=0.1", "bias=0.3"])
    stats = {"mean": [0.0, 1.0, 2.0], "std": [0.5, 2.0, 1e-3]}
    bs, ns = A.scales(spec, stats)
    assert bs.dtype == ns.dtype == np.float64
    assert bs.tolist() == [float(np.float32(0.3)) * s for s in stats["std"]]
    assert ns.tolist() == [float(np.float32(0.1)) * s for s in stats["std"]]
    limits = {"min": [0.0, -1.0], "range": [4.0, 3.0], "norm_config": {"type": "limits", "out_min": -1.0, "out_max": 1.0}}
    bs, ns = A.scales(spec, limits)
    assert bs.tolist() == [float(np.float32(0.3)) * (4.0 / 2.0), float(np.float32(0.3)) * (3.0 / 2.0)]


def test_host_normals_are_the_f64_box_muller_normals_rounded():
    for Adim in AC.AS:
        ep, dr = AC.EPISODES, AC.R0 * 3
        got = A.host_normals(AC.SEED, ep, dr, Adim)
        want = np.stack([PC.normals(AC.SEED, int(e), int(d), AC.PLANE_NOISE, Adim) for e, d in zip(ep, dr)])
        assert got.dtype == np.float32 and got.tobytes() == want.astype(np.float32).tobytes()


@pytest.mark.parametrize("comp", list(AC.COMPONENTS))
@pytest.mark.parametrize("Adim", AC.AS)
@pytest.mark.parametrize("n", AC.NS)
def test_restatement_equals_the_oracle_element_by_element(n, Adim, comp):
    for D in AC.DS:
        for skip in AC.SKIPS:
            spec, acts, (out, mask), (want, wmask) = _both(n, Adim, D, skip, comp)
            assert mask.tolist() == wmask.tolist(), (D, skip)
            for t in range(AC.T):
                for i in range(n):
                    if mask[t, i]:
                        for k in range(Adim):
                            assert out[t, i, k] == want[t, i, k], (D, skip, t, i, k)
                    else:
                        assert np.isnan(out[t, i]).all()
            # what the case is meant to show does happen
            r = AC.R0[None, :n] + np.arange(AC.T)[:, None]
            assert mask[:, 0].tolist()[:D] == [0] * D  # r < D: nothing arrives
            if spec.hold == 0:
                assert (mask != 0).tolist() == (r >= D).tolist()
            elif n == 5:
                assert 0 < mask.sum() < (r >= D).sum() and not mask[r < D].any()
            sel = mask != 0
            sel[:D] = False  # the steps whose command was made inside the case
            delayed = np.full_like(acts, np.nan)
            delayed[D:] = acts[:AC.T - D]
            if comp in ("delay", "hold"):  # no arithmetic: the input bytes, D steps late
                assert out[sel].tobytes() == delayed[sel].tobytes()
            elif sel.any():
                assert (out[sel] != delayed[sel]).all()


def test_zero_spec_is_the_identity_and_keeps_the_mask():
    acts = AC.actions(5, 7)
    scale, bs, ns = AC.scale_arrays(7)
    mask_in = (np.random.default_rng(3).random((AC.T, 5)) < 0.6).astype(np.uint8)
    out, mask = A.restate(A.ActuationSpec(), AC.SEED, 3, bs, ns, AC.EPISODES, AC.R0, acts, mask_in=mask_in)
    assert mask.tobytes() == mask_in.tobytes()
    assert out[mask != 0].tobytes() == acts[mask != 0].tobytes() and np.isnan(out[mask == 0]).all()


def test_noise_is_held_over_the_skip_steps_and_bias_over_the_episode():
    skip, Adim = 3, 5
    acts = np.zeros((AC.T, 5, Adim))
    scale, bs, ns = AC.scale_arrays(Adim, noise=0.3, bias=0.2)
    r = AC.R0[None, :] + np.arange(AC.T)[:, None]
    noise, _ = A.restate(A.ActuationSpec(noise=AC.f32(0.3)), AC.SEED, skip, bs, ns, AC.EPISODES, r, acts)
    for i in range(5):
        for t in range(1, AC.T):
            same = r[t, i] // skip == r[t - 1, i] // skip
            assert np.array_equal(noise[t, i], noise[t - 1, i]) == same, (i, t)
    bias, _ = A.restate(A.ActuationSpec(bias=AC.f32(0.2)), AC.SEED, skip, bs, ns, AC.EPISODES, r, acts)
    assert (bias == bias[:1]).all() and (np.abs(bias[0]) <= bs).all()
    assert len(np.unique(bias[0])) == 5 * Adim  # every episode and dimension its own offset


# -- independence of the batch ---------------------------------------------------------------------------
def test_an_episode_does_not_depend_on_the_batch():
    Adim, D, skip = 7, 3, 3
    spec = _spec("all", D)
    acts = AC.actions(5, Adim)
    scale, bs, ns = AC.scale_arrays(Adim, spec.noise, spec.bias)
    R = AC.R0[None, :] + np.arange(AC.T, dtype=np.int32)[:, None]
    full, fmask = A.restate(spec, AC.SEED, skip, bs, ns, AC.EPISODES, R, acts)
    perm = np.array([3, 0, 4, 2, 1])
    out, mask = A.restate(spec, AC.SEED, skip, bs, ns, AC.EPISODES[perm], R[:, perm], acts[:, perm])
    assert out.tobytes() == full[:, perm].tobytes() and mask.tobytes() == fmask[:, perm].tobytes()
    for i in (0, 3):
        out, mask = A.restate(spec, AC.SEED, skip, bs, ns, AC.EPISODES[i:i + 1], R[:, i:i + 1], acts[:, i:i + 1])
        assert out.tobytes() == full[:, i:i + 1].tobytes() and mask.tobytes() == fmask[:, i:i + 1].tobytes()
    # another episode or seed: another result
    other, _ = A.restate(spec, AC.SEED, skip, bs, ns, AC.EPISODES + 1, R, acts)
    assert not np.array_equal(other, full, equal_nan=True)
    other, _ = A.restate(spec, AC.SEED + 1, skip, bs, ns, AC.EPISODES, R, acts)
    assert not np.array_equal(other, full, equal_nan=True)


# -- is_skip of the arriving command ----------------------------------------------------------------------
@pytest.mark.parametrize("skip", [1, 3])
@pytest.mark.parametrize("D", [0, 1, 2, 3, 4])
def test_is_skip_congruence_of_streaming_slots(skip, D):
    """A slot whose episode started at host rollout step s, a multiple of P = skip x the inference
    period, is at r_e = hr - s when the host is at hr.  The host scalar (hr - D) % skip != 0 is then the
    is_skip of the step every slot's arriving command was made for, whatever its start."""
    for period_calls in (1, 2, 8):
        P = skip * period_calls
        for s in range(0, 6 * P, P):
            for hr in range(s, s + 4 * P + D + 2):
                r_e = hr - s
                assert (r_e - D) % skip == (hr - D) % skip
                host = A.is_skip(hr, D, skip)
                assert isinstance(host, bool) and host == ((hr - D) % skip != 0)
                if r_e >= D:  # a command arrives: the one made at step r_e - D of the episode
                    made_at = r_e - D
                    assert host == (made_at % skip != 0)  # set_command_data's is_skip at that step
    # a start off the grid would break it: the congruence is a property of the aligned recycle
    if skip > 1:
        assert any(((hr - 1) - D) % skip != (hr - D) % skip for hr in range(1, 8))


# -- the hold draw ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, stated", [(7, 0.2566), (0, 0.2605)])
def test_loss_rate(seed, stated):
    """hold = 0.25 over episodes 0..63 x steps 0..63: the lost fraction lies within 5 sigma =
    5 * sqrt(0.25 * 0.75 / 4096) = 0.034 of P (derived, not measured)."""
    ep, r = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    lost = A.lost(seed, ep, r, np.float32(0.25))
    assert lost.shape == (64, 64) and lost.dtype == bool
    frac = float(lost.mean())
    bound = 5 * math.sqrt(0.25 * 0.75 / 4096)
    print(f"\nseed {seed}: lost fraction {frac:.4f} (bound 0.25 +- {bound:.4f})")
    assert abs(bound - 0.034) < 5e-4 and abs(frac - 0.25) <= bound
    assert round(frac, 4) == stated
    # the oracle's draw, element by element
    for e, s in ((0, 0), (5, 17), (63, 63), (31, 2)):
        assert bool(lost[e, s]) == AC.packet_lost(seed, e, s, 0.25)
    # per episode and per step, not per batch: rows and columns differ
    assert len({tuple(row) for row in lost.tolist()}) == 64
