"""rmbx_sarnn_attention and rmbx_sarnn_lstm_step at the sizes tests/test_sarnn_gpu.py does not launch
(the cases of tests/observation_cases.py), to that file's own bars.

Attention, per entry 2 (d_ref / T) MAD + 2^-18 (_attention_case / _check_attention of test_sarnn_gpu):
the 4-wide (K = 3, 4) and 8-wide (K = 7, 8, 13, 16) instantiations of the last convolution, one and two
groups of it, both branches of the weight packing (K % 8 == 0 or not), S = 8 (a 2 x 2 map), odd maps
(S = 9, 23), one to four cameras, K = 16 at the production and the largest image.  A constant image has
the known answer (0.5, 0.5) whatever the weights; a NaN pixel stays in its (env, camera).

LSTM, bar = 4 x the measured max |torch-CPU fp32 - f64| of LSTMCell + decoder over four steps at the
same size (the reference route's own error; the factor is the existing margin for the device's exp /
tanh).  Measured on an MI355X host, (hidden, state_dim, key_dim): torch-CPU fp32 error, kernel error
(the first figure depends on the host's CPU kernels, which is why the test measures it each time):

    (128,   7,  20)   6.929e-08   8.358e-08
    ( 64,   7,  20)   9.944e-08   1.436e-07
    ( 65,   7,  20)   1.141e-07   9.522e-08
    (  1,   1,   0)   2.083e-08   2.083e-08
    ( 50, 130, 120)   3.136e-07   2.838e-07
    (128,   1, 255)   2.170e-07   3.294e-07
"""

import copy

import pytest
import torch

import observation_cases as C
from test_sarnn_gpu import _attention_case, _check_attention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("S,K,ncam", C.ATTENTION_CASES)
def test_attention_kernel_edges_against_f64(S, K, ncam):
    from robomanipbaselines_amd import kernels as Kn

    model, images, want, bar = _attention_case(S, K, ncam)
    packed = copy.deepcopy(model).to(DEV)._packed()
    groups, size = Kn.sarnn_conv_groups(K)
    assert packed[4].shape == (ncam, groups, 32, 9, size)
    x = images.to(DEV)
    got = Kn.sarnn_attention(x, packed, model.temperature)
    assert got.shape == (3, ncam, K, 2)
    _check_attention(got.cpu().numpy(), want, bar, f"attention S={S} K={K} ncam={ncam}")
    # reproducible, and independent of the batch
    assert torch.equal(got, Kn.sarnn_attention(x, packed, model.temperature))
    assert torch.equal(got[1:2], Kn.sarnn_attention(x[1:2].contiguous(), packed, model.temperature))


@pytest.mark.parametrize("S,K", C.KNOWN_ANSWER_CASES)
def test_attention_of_a_constant_image_is_the_centre(S, K):
    """Independent of the restated model: identical logits at every pixel make the softmax uniform, so
    every key is the mean position (0.5, 0.5), to the summation term of the bar."""
    from robomanipbaselines_amd import kernels as Kn

    model, images = C.constant_image_case(S, K)
    got = Kn.sarnn_attention(images.to(DEV), copy.deepcopy(model).to(DEV)._packed(), model.temperature).cpu()
    err = float((got.double() - 0.5).abs().max())
    print(f"\nconstant image S={S} K={K}: max |key - 0.5| {err:.3e}, bar {C.KNOWN_ANSWER_BAR:.3e}")
    assert got.shape == (3, 2, K, 2) and err <= C.KNOWN_ANSWER_BAR


def test_attention_nan_stays_in_its_env_and_camera():
    from robomanipbaselines_amd import kernels as Kn

    model, images, _, _ = _attention_case(20, 7, 2)
    packed = copy.deepcopy(model).to(DEV)._packed()
    clean = Kn.sarnn_attention(images.to(DEV), packed, model.temperature).cpu()
    dirty = images.clone()
    dirty[1, 0, 1, 9, 11] = float("nan")
    got = Kn.sarnn_attention(dirty.to(DEV), packed, model.temperature).cpu()
    assert bool(torch.isnan(got[1, 0]).all())
    keep = torch.ones(3, 2, dtype=torch.bool)
    keep[1, 0] = False
    assert torch.equal(got[keep], clean[keep]) and not bool(torch.isnan(clean).any())


def _random_packed(ncam, K):
    from robomanipbaselines_amd import kernels as Kn

    torch.manual_seed(7)
    convs = [[torch.nn.Conv2d(ci, co, 3) for _ in range(ncam)] for ci, co in ((3, 16), (16, 32), (32, K))]
    return tuple(t.to(DEV) for t in Kn.sarnn_pack_attention(convs))


def test_attention_empty_batch_and_rejections():
    """Each rejection raises before a launch: the sentinel-filled `out` keeps its bits."""
    from robomanipbaselines_amd import kernels as Kn

    empty = torch.empty((0, 2, 3, 20, 20), device=DEV)
    assert Kn.sarnn_attention(empty, _random_packed(2, 5), 1e-4).shape == (0, 2, 5, 2)
    outs = []
    for S, K, ncam, T, word in ((7, 5, 1, 1e-4, "S = 7"), (129, 5, 1, 1e-4, "S = 129"), (20, 17, 1, 1e-4, "K <= 16"),
                                (20, 5, 5, 1e-4, "ncam = 5"), (20, 5, 1, 0.0, "temperature")):
        out = torch.full((1, ncam, K, 2), 7.25, device=DEV)
        outs.append(out)
        with pytest.raises(ValueError, match=word):
            Kn.sarnn_attention(torch.rand((1, ncam, 3, S, S), device=DEV), _random_packed(ncam, K), T, out=out)
    torch.cuda.synchronize()
    assert all(bool((o == 7.25).all()) for o in outs)


def _lstm_params(lstm, dec):
    return [t.to(DEV).contiguous() for t in (lstm.weight_ih, lstm.weight_hh, lstm.bias_ih, lstm.bias_hh, dec.weight,
                                             dec.bias)]


@pytest.mark.parametrize("hd,sd,kd", C.LSTM_CASES)
def test_lstm_kernel_edges_against_f64_recurrence(hd, sd, kd):
    """Four steps, each route feeding its own (h, c) back; the figures per size are in the module docstring."""
    from robomanipbaselines_amd import kernels as Kn

    lstm, dec, xs, want, ref_err = C.lstm_case(hd, sd, kd)
    bar = 4.0 * ref_err
    params = _lstm_params(lstm, dec)
    n = C.LSTM_ENVS
    h, c = torch.zeros(n, hd, device=DEV), torch.zeros(n, hd, device=DEV)
    worst = 0.0
    for x, refs in zip(xs, want):
        xd = x.to(DEV)
        pred = Kn.sarnn_lstm_step(xd[:, :sd].contiguous(), xd[:, sd:].contiguous(), h, c, *params)
        assert pred.shape == (n, sd)
        for got, ref in zip((pred, h, c), refs):
            worst = max(worst, float((got.cpu().double() - ref).abs().max()))
    print(f"\nLSTM hidden {hd} state {sd} keys {kd}: torch-CPU fp32 error {ref_err:.3e}, bar {bar:.3e}, "
          f"kernel error {worst:.3e}")
    assert ref_err > 0.0  # the bar is never vacuous
    assert worst <= bar


def test_lstm_masked_rows_at_a_full_block():
    """hidden = 128, every thread of the block a hidden unit: masked rows of h, c and the output keep their
    bits, active rows equal the unmasked step."""
    from robomanipbaselines_amd import kernels as Kn

    hd, sd, kd = C.LSTM_CASES[0]
    assert hd == 128
    lstm, dec, xs, _, _ = C.lstm_case(hd, sd, kd)
    params = _lstm_params(lstm, dec)
    n = C.LSTM_ENVS
    g = torch.Generator().manual_seed(3)
    h0, c0 = (torch.rand(n, hd, generator=g) - 0.5).to(DEV), (torch.rand(n, hd, generator=g) - 0.5).to(DEV)
    xd = xs[0].to(DEV)
    st, ky = xd[:, :sd].contiguous(), xd[:, sd:].contiguous()
    active = (torch.arange(n, device=DEV) % 2).to(torch.uint8)
    h, c = h0.clone(), c0.clone()
    out = torch.full((n, sd), 7.25, device=DEV)
    Kn.sarnn_lstm_step(st, ky, h, c, *params, active=active, out=out)
    hf, cf = h0.clone(), c0.clone()
    full = Kn.sarnn_lstm_step(st, ky, hf, cf, *params)
    m = active.bool()
    assert torch.equal(h[~m], h0[~m]) and torch.equal(c[~m], c0[~m]) and bool((out[~m] == 7.25).all())
    assert torch.equal(h[m], hf[m]) and torch.equal(c[m], cf[m]) and torch.equal(out[m], full[m])
    assert not torch.equal(hf[m], h0[m])


def _lstm_zeros(n, hd, sd, kd):
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    return (z(n, sd), z(n, kd), z(n, hd), z(n, hd), z(4 * hd, sd + kd), z(4 * hd, hd), z(4 * hd), z(4 * hd), z(sd, hd),
            z(sd))


def test_lstm_empty_batch_and_rejections():
    from robomanipbaselines_amd import kernels as Kn

    assert Kn.sarnn_lstm_step(*_lstm_zeros(0, 50, 7, 20)).shape == (0, 7)
    outs = []
    for hd, sd, kd, word in ((129, 7, 20, "hidden = 129"), (50, 7, 250, "257 exceeds 256"),
                             (50, 257, 0, "257 exceeds 256")):
        args = _lstm_zeros(2, hd, sd, kd)
        h, c = args[2].fill_(7.25), args[3].fill_(7.25)
        out = torch.full((2, sd), 7.25, device=DEV)
        outs += [h, c, out]
        with pytest.raises(ValueError, match=word):
            Kn.sarnn_lstm_step(*args, out=out)
    torch.cuda.synchronize()
    assert all(bool((o == 7.25).all()) for o in outs)
