"""The per-episode sampler noise without a GPU: the Random123 known answers of Philox4x32-10 and the
moments of the rule's normals on the numpy restatement (tests/philox_cases.py), the
--sampler_noise flag, and the rejections of kernels.philox_normal that happen before the device."""

import numpy as np
import pytest
import torch

import philox_cases as PC

# (counter, key, output): the Philox4x32-10 vectors of Random123's kat_vectors
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = " ".join(f"{int(w):08x}" for w in PC.philox4x32_10(counter, key))
    assert got == want


def test_words_follow_the_counter_layout():
    """words() is Philox at counter (j, plane, draw, episode), key (seed lo, seed hi); a negative
    episode enters as its bit pattern; the batch form agrees with the row form."""
    seed, ep, dr, pl, L = 2**40 + 7, -1, 2**31 - 1, 9, 21
    w = PC.words(seed, ep, dr, pl, L)
    assert w.shape == (24,) and w.dtype == np.uint32
    for j in (0, 3, 5):
        want = PC.philox4x32_10((j, pl, dr, 0xFFFFFFFF), (7, 2**8))
        assert [int(x) for x in want] == w[4 * j: 4 * j + 4].tolist()
    b = PC.words_batch(seed, [5, ep, 0], [0, dr, 1], pl - 1, 3, L)
    assert b.shape == (3, 3, 24) and np.array_equal(b[1, 1], w)
    assert np.array_equal(b[0, 0], PC.words(seed, 5, 0, pl - 1, L))
    assert np.array_equal(b[2, 2], PC.words(seed, 0, 1, pl + 1, L))


@pytest.fixture(scope="module")
def stream():
    return PC.normals(3, 5, 2, 7, 2**20)


def test_normals_are_bounded_and_exact_at_the_extremes():
    # u1 smallest (word 0) with u2 -> angle near 0: |z| = sqrt(-2 ln 2^-24) = 5.768
    z = PC.normals_from_words(np.array([0, 0, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32))
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.77
    assert abs(np.hypot(z[0], z[1]) - np.sqrt(-2 * np.log(2.0**-24))) < 1e-12
    # u1 largest: r = sqrt(-2 ln(1 - 2^-24)) > 0, so no value is exactly lost to log(1)
    assert np.hypot(z[2], z[3]) > 3e-4


def test_moments(stream):
    """5-sigma bounds for N = 2^20 standard normals.  Measured on the restatement: mean -6.4e-4,
    var - 1 2.5e-3, E z^4 - 3 2.1e-2."""
    z, N = stream, 2**20
    assert z.shape == (N,)
    assert abs(z.mean()) <= 5 / np.sqrt(N)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / N)
    assert abs((z**4).mean() - 3) <= 5 * np.sqrt(96 / N)
    assert np.abs(z).max() <= 5.77


@pytest.mark.parametrize("what,args", [("episode", (3, 6, 2, 7)), ("plane", (3, 5, 2, 8)), ("draw", (3, 5, 3, 7)),
                                       ("seed", (4, 5, 2, 7))])
def test_neighbouring_streams_are_uncorrelated(stream, what, args):
    """Correlation with the stream of the neighbouring episode / plane / draw / seed <= 5 / sqrt(N)
    (measured: at most 1.6e-3)."""
    N = 2**20
    other = PC.normals(*args, N)
    c = np.corrcoef(stream, other)[0, 1]
    assert abs(c) <= 5 / np.sqrt(N), (what, c)


# -- the flag --------------------------------------------------------------------------------------
def _parse(argv):
    from robomanipbaselines_amd.common.rollout_base import BatchedRolloutBase
    from robomanipbaselines_amd.policy.diffusion_policy.rollout_diffusion_policy import RolloutDiffusionPolicy
    from robomanipbaselines_amd.policy.diffusion_policy_3d.rollout_diffusion_policy_3d import RolloutDiffusionPolicy3d

    out = []
    for cls in (RolloutDiffusionPolicy, RolloutDiffusionPolicy3d):
        ro = cls.__new__(cls)  # the parser alone: no env, no device
        BatchedRolloutBase.setup_args(ro, argv=argv)
        out.append(ro.args)
    return out


def test_sampler_noise_flag():
    for a in _parse([]):
        assert a.sampler_noise == "batch"  # the default stays today's behaviour
    for a in _parse(["--sampler_noise", "episode", "--seed", "3"]):
        assert a.sampler_noise == "episode" and a.seed == 3
    with pytest.raises(SystemExit):
        _parse(["--sampler_noise", "slot"])


def test_other_policies_do_not_take_the_flag():
    from robomanipbaselines_amd.common.rollout_base import BatchedRolloutBase
    from robomanipbaselines_amd.policy.mlp.rollout_mlp import RolloutMlp

    ro = RolloutMlp.__new__(RolloutMlp)
    with pytest.raises(SystemExit):
        BatchedRolloutBase.setup_args(ro, argv=["--sampler_noise", "episode"])


def test_bench_policy_passes_the_flag_through(monkeypatch, capsys):
    """scripts/bench_policy.py: --sampler_noise reaches the Rollout command line of the diffusion
    policies, is absent when not given, and is refused for the other policies."""
    import importlib.util
    import os

    from conftest import ROOT

    # (the script sets a MIOpen variable when it is imported: keep it out of this process)
    monkeypatch.delenv("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", raising=False)
    monkeypatch.setattr("sys.path", list(__import__("sys").path))
    spec = importlib.util.spec_from_file_location("bench_policy_under_test",
                                                  os.path.join(ROOT, "scripts", "bench_policy.py"))
    bp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bp)
    for policy in ("DiffusionPolicy", "DiffusionPolicy3d"):
        for mode in ("batch", "episode"):
            argv = bp.rollout_argv(bp.parse_args([policy, "--sampler_noise", mode]))
            assert argv[argv.index("--sampler_noise") + 1] == mode
            # and the rollout's own parser takes that command line
            assert [a.sampler_noise for a in _parse(argv)] == [mode, mode]
        assert "--sampler_noise" not in bp.rollout_argv(bp.parse_args([policy]))
    assert "--sampler_noise" not in bp.rollout_argv(bp.parse_args(["Mlp"]))
    for policy in ("Mlp", "Act", "Sarnn"):
        with pytest.raises(SystemExit):
            bp.parse_args([policy, "--sampler_noise", "episode"])
        assert "flag of the diffusion policies" in capsys.readouterr().err


# -- the wrapper's rejections before the device -------------------------------------------------------
def _args(n=3, L=8, nplane=2):
    ep = torch.arange(n, dtype=torch.int32)
    return ep, torch.zeros(n, dtype=torch.int32), torch.zeros(nplane, n, L)


def test_wrapper_rejects_wrong_calls_before_the_device():
    from robomanipbaselines_amd import kernels as K

    ep, dr, out = _args()
    bad = [
        (dict(seed=-1), "seed"), (dict(seed=2**64), "seed"), (dict(plane0=-1), "plane0"),
        (dict(episode=ep.long()), "episode must be torch.int32"), (dict(draw=dr.float()), "draw must be torch.int32"),
        (dict(out=out.double()), "out must be torch.float32"), (dict(out=out.int()), "out must be torch.float32"),
        (dict(episode=ep[:2]), "draw must have shape"), (dict(episode=ep.view(3, 1)), "episode must have shape"),
        (dict(episode=ep[:0], draw=dr[:0], out=out[:, :0]), "episode must have shape"),
        (dict(out=out[0]), r"out must have shape \[nplane, 3"), (dict(out=out[:, :2].contiguous()), r"out must have shape \[nplane, 3"),
        (dict(out=out[:0]), "out must have shape"), (dict(out=out[:, :, ::2]), "out must be contiguous"),
        (dict(out=out[:, :, :0]), "rows must not be empty"), (dict(L=7), "L = 7 does not match"),
        (dict(out=out.int(), words=True), "needs the row length"),
        (dict(out=out.int(), words=True, L=3), "out must have shape"),
        (dict(out=out, words=True, L=8), "out must be torch.int32"),
        (dict(out=out, plane0=2**31 - 2), "exceeds"),
        (dict(episode=[0, 1, 2]), "must be a torch.Tensor"),
    ]
    for over, msg in bad:
        kw = dict(seed=3, episode=ep, draw=dr, out=out)
        kw.update(over)
        with pytest.raises(ValueError, match=msg):
            K.philox_normal(**kw)
    # a well-formed call on host tensors reaches the device check: there is no host fallback
    with pytest.raises(ValueError, match="must be a device tensor"):
        K.philox_normal(3, ep, dr, out)
    with pytest.raises(ValueError, match="must be a device tensor"):
        K.philox_normal(3, ep, dr, torch.zeros(2, 3, 8, dtype=torch.int32), L=7, words=True)


def test_native_rejects_bad_arguments_before_any_launch():
    """The C entry point itself: every argument error of include/rmbx.h is RMBX_ERR_ARG (-1), decided
    on the host before a launch (so it is the same answer without a GPU)."""
    import ctypes

    from robomanipbaselines_amd import _native as N

    lib = N.load()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    ok = dict(seed=3, episode=p, draw=p, plane0=0, nplane=1, out=p, n=2, L=5, kind=0)
    for over in (dict(episode=None), dict(draw=None), dict(out=None), dict(n=0), dict(n=-3), dict(L=0),
                 dict(nplane=0), dict(plane0=-1), dict(kind=2), dict(kind=-1), dict(plane0=2**31 - 1, nplane=1),
                 dict(out=p + 2), dict(n=2**31 - 1, L=8)):
        a = dict(ok)
        a.update(over)
        st = lib.rmbx_philox_normal(a["seed"], a["episode"], a["draw"], a["plane0"], a["nplane"], a["out"], a["n"],
                                    a["L"], a["kind"], None)
        assert st == -1, over
        assert b"rmbx_philox_normal" in lib.rmbx_last_error()


def test_sampler_refuses_a_noise_source_beside_explicit_noise():
    from robomanipbaselines_amd.policy.diffusion_policy.dp_model import DiffusionPolicyModel

    m = DiffusionPolicyModel(7, 7, 1, crop_hw=(64, 96), down_dims=(64, 128, 256)).eval()
    gc = torch.zeros(2, m.obs_feature_dim * 2)
    src = (3, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="noise_source"):
        m.conditional_sample(gc, x0=torch.zeros(2, 16, 7), noise_source=src)
    # and without a device there is no fallback to torch.randn
    with pytest.raises(ValueError, match="device tensor"):
        m.conditional_sample(gc, noise_source=src)
