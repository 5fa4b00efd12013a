"""rmbx_add_layernorm (+ its _pos / _split forms) and rmbx_groupnorm_act against f64 at every
instantiation, tail and path switch, within the derived bar of tests/test_norm_edges.py
(err <= bar element-wise; the bar has about 2x over correct f32 arithmetic and none for a one-pass
variance, a wrong divisor or a tail lane counted twice), plus the bitwise invariants: a row / batch
element does not depend on its neighbours, the fused forms equal the plain one, in place equals out
of place, non-finite rows stay in their rows.

Worst err / bar per instantiation, first measured on an MI355X (the host test has torch's CPU f32
kernels at 0.48 / 0.51 of the same bars):

    add_layernorm f32  PER=1 (D 4, 36, 256)   0.423 (D 36, mean1e3, eps 1e-3)
    add_layernorm f32  PER=2 (D 260, 512)     0.302 (D 512, r_none)
    add_layernorm f32  PER=4 (D 516, 1024)    0.402 (D 516, r_none, 1 row)
    add_layernorm f32  PER=8 (D 1028, 2048)   0.362 (D 2048, spike, eps 1e-3)
    add_layernorm bf16 PER=1 (D 8, 72, 512)   0.992 (D 512, spike)
    add_layernorm bf16 PER=2 (D 520, 1024)    0.996 (D 520, huge)
    add_layernorm bf16 PER=4 (D 1032, 2048)   0.995 (D 2048, r_none)
    groupnorm_act register path (E <= 2048)   0.498 (E 300, mean1e3, time-major)
    groupnorm_act three-pass path (E = 2049)  0.279 (unit, time-major)

The bf16 figures are the output's own rounding: 2^-8 |ref| is exactly half a bf16 ulp at the bottom
of a binade, so an element just short of a tie sits just under the bar.
"""

import pytest
import torch
from test_norm_edges import (GN_CASES, GN_SHAPES, LN_CASES, LN_EPS3_WIDTHS, LN_WIDTHS, gn_inputs, gn_reference,
                             ln_inputs, ln_per, ln_reference, worst_ratio)
from test_presplit_gpu import _check_pieces

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_NAME = {torch.float32: "f32", torch.bfloat16: "bf16"}
LN_PARAMS = [pytest.param(dt, D, id=f"{_NAME[dt]}-PER{ln_per(dt, D)}-D{D}") for dt, ws in LN_WIDTHS.items() for D in ws]


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.mark.parametrize("dtype,D", LN_PARAMS)
def test_add_layernorm_vs_f64(dtype, D):
    """Every data case, 7 rows (a 4-row block, then a block with one dead wave) and 1 row, eps 1e-5
    (and 1e-3 at one width per instantiation): within the bar element-wise; a constant row gives
    exactly b (var = 0: eps alone sets rstd, and s - mean is exactly 0)."""
    from robomanipbaselines_amd import kernels as K

    results, exact = [], []
    for eps in (1e-5, 1e-3) if D in LN_EPS3_WIDTHS[dtype] else (1e-5,):
        for rows in (7, 1):
            for case in LN_CASES:
                x, r, w, b = ln_inputs(rows, D, dtype, case)
                ref, bar = ln_reference(x, r, w, b, eps)
                got = K.add_layernorm(*_dev(x, r, w, b), eps).cpu()
                assert got.dtype == dtype and got.shape == (rows, D)
                results.append((worst_ratio(got, ref, bar), case, rows, eps))
                if case == "const":
                    exact.append(torch.equal(got, b.to(dtype).expand(rows, D)))
    top = max(results)
    print(f"add_layernorm {_NAME[dtype]} PER={ln_per(dtype, D)} D={D}: worst err / bar {top[0]:.3f} at {top[1:]}")
    assert all(ratio <= 1.0 for ratio, *_ in results), [t for t in results if not t[0] <= 1.0]
    assert all(exact), "a constant row must give exactly b"


@pytest.mark.parametrize("dtype,D", LN_PARAMS)
def test_add_layernorm_invariants_bitwise(dtype, D):
    """A row equals the same row run alone; add_layernorm_pos's y is add_layernorm's and its y_pos is
    y + pos[row % 3] as torch adds in the storage dtype; in place equals out of place; (f32)
    add_layernorm_split writes the same y and y_pos, pieces that rebuild them, and a norm bound
    within [1, 1 + 2^-11] of the f64 norm."""
    from robomanipbaselines_amd import kernels as K

    for case in ("unit", "mean1e3", "spike", "r_none"):
        x, r, w, b = _dev(*ln_inputs(12, D, dtype, case))
        pos = _dev(ln_inputs(3, D, dtype, "unit")[0])[0]
        y = K.add_layernorm(x, r, w, b, 1e-5)
        for i in range(12):
            alone = K.add_layernorm(x[i:i + 1].clone(), None if r is None else r[i:i + 1].clone(), w, b, 1e-5)
            assert torch.equal(alone[0], y[i]), (case, i)
        x3, r3 = x.view(2, 6, D), None if r is None else r.view(2, 6, D)
        y3, yp3 = K.add_layernorm_pos(x3, r3, w, b, pos, 1e-5)
        assert torch.equal(y3, y.view(2, 6, D)), case
        assert torch.equal(yp3, y3 + pos.repeat(2, 1)), case  # row b 6 + t takes pos[t % 3]
        if dtype == torch.float32:
            ys, yps = K.add_layernorm_split(x3, r3, w, b, 1e-5, pos=pos, y_norm=True)
            assert torch.equal(ys, y3) and torch.equal(yps, yp3), case
            _check_pieces(ys.rmbx_split, ys)
            _check_pieces(yps.rmbx_split, yps)
            norm = ys.rmbx_split.norm.double()
            true = y.double().norm(dim=1)
            assert ((norm >= true) & (norm <= true * (1 + 2.0 ** -11))).all(), case
        xin = x.clone()
        out = K.add_layernorm(xin, r, w, b, 1e-5, out=xin)
        assert out.data_ptr() == xin.data_ptr() and torch.equal(out, y), case


@pytest.mark.parametrize("dtype,D", LN_PARAMS)
def test_add_layernorm_nonfinite_rows_stay_in_their_rows(dtype, D):
    """8 rows (two blocks), a NaN in row 2 and an inf in row 5: those rows come out non-finite, as
    torch's do; the other six (same-block neighbours included) are bitwise the clean run's."""
    from robomanipbaselines_amd import kernels as K

    x, r, w, b = _dev(*ln_inputs(8, D, dtype, "unit"))
    clean = K.add_layernorm(x, r, w, b, 1e-5)
    bad = x.clone()
    bad[2, D // 2] = float("nan")
    bad[5, D - 1] = float("inf")
    y = K.add_layernorm(bad, r, w, b, 1e-5)
    assert not torch.isfinite(y[[2, 5]]).any()
    keep = [0, 1, 3, 4, 6, 7]
    assert torch.isfinite(y[keep]).all() and torch.equal(y[keep], clean[keep])
    y, yp = K.add_layernorm_pos(bad.view(1, 8, D), r.view(1, 8, D), w, b, x[:4].contiguous(), 1e-5)
    assert not torch.isfinite(y[0, [2, 5]]).any() and not torch.isfinite(yp[0, [2, 5]]).any()
    assert torch.equal(y[0, keep], clean[keep])


def test_add_layernorm_guards():
    """A bad `out`, a D that is no multiple of the vector width or above 2048: ValueError before
    any launch."""
    from robomanipbaselines_amd import kernels as K

    x = torch.randn(7, 512, device=DEV)
    r = torch.randn(7, 512, device=DEV)
    w = torch.ones(512, device=DEV)
    b = torch.zeros(512, device=DEV)
    for bad in (torch.empty(7, 256, device=DEV), torch.empty(8, 512, device=DEV), torch.empty(7 * 512, device=DEV),
                torch.empty(7, 512, device=DEV, dtype=torch.bfloat16),
                torch.empty(7, 512, device=DEV, dtype=torch.float64), torch.empty(7, 512),
                torch.empty(512, 7, device=DEV).t(), torch.empty(7, 1024, device=DEV)[:, ::2]):
        with pytest.raises(ValueError):
            K.add_layernorm(x, r, w, b, out=bad)
    with pytest.raises(ValueError):
        K.add_layernorm(x.bfloat16(), r.bfloat16(), w, b, out=torch.empty(7, 512, device=DEV))
    assert torch.equal(K.add_layernorm(x, r, w, b, out=torch.empty(7, 512, device=DEV)), K.add_layernorm(x, r, w, b))
    for dtype, D in ((torch.float32, 6), (torch.float32, 510), (torch.bfloat16, 12), (torch.bfloat16, 516),
                     (torch.float32, 2052), (torch.bfloat16, 2056)):
        xd = torch.zeros(3, 2, D, device=DEV, dtype=dtype)
        wd = torch.ones(D, device=DEV)
        with pytest.raises(ValueError):
            K.add_layernorm(xd, xd, wd, wd)
        with pytest.raises(ValueError):
            K.add_layernorm(xd, None, wd, wd)
        with pytest.raises(ValueError):
            K.add_layernorm_pos(xd, xd, wd, wd, xd[0])
        if dtype == torch.float32:
            with pytest.raises(ValueError):
                K.add_layernorm_split(xd, xd, wd, wd, pos=xd[0], y_norm=True)


@pytest.mark.parametrize("B,C,T,G", GN_SHAPES, ids=[f"E{c // g * t}-B{b}C{c}T{t}G{g}" for b, c, t, g in GN_SHAPES])
def test_groupnorm_act_vs_f64(B, C, T, G):
    """Both layouts, Mish on and off, every data case: within the bar element-wise.  A constant
    span (and any span of one element) gives exactly b without Mish, and with it one value per
    channel whatever the constant."""
    from robomanipbaselines_amd import kernels as K

    E = C // G * T
    results = []
    for case in GN_CASES:
        x, w, b = gn_inputs(B, C, T, G, case)
        xd, wd, bd = _dev(x, w, b)
        xt = xd.transpose(1, 2).contiguous()
        for mish in (False, True):
            ref, bar = gn_reference(x, w, b, G, 1e-5, mish)
            for time_major in (False, True):
                got = K.groupnorm_act(xt if time_major else xd, wd, bd, G, 1e-5, mish=mish, time_major=time_major)
                assert got.shape == (B, C, T)
                got = got.cpu()
                results.append((worst_ratio(got, ref, bar), case, mish, time_major))
                if case == "const" or E == 1:
                    if not mish:
                        assert torch.equal(got, b[None, :, None].expand(B, C, T)), (case, time_major)
                    else:
                        assert torch.equal(got, got[:1, :, :1].expand(B, C, T)), (case, time_major)
    top = max(results)
    path = "register" if E <= 2048 else "three-pass"
    print(f"groupnorm_act {path} path E={E} {(B, C, T, G)}: worst err / bar {top[0]:.3f} at {top[1:]}")
    assert all(ratio <= 1.0 for ratio, *_ in results), [t for t in results if not t[0] <= 1.0]


@pytest.mark.parametrize("B,C,T,G", GN_SHAPES, ids=[f"E{c // g * t}-B{b}C{c}T{t}G{g}" for b, c, t, g in GN_SHAPES])
def test_groupnorm_act_invariants_bitwise(B, C, T, G):
    """In place (channel-major) equals out of place; a batch element equals the same element run
    alone, in each layout (the two layouts walk a span in different orders, so they agree with each
    other only to rounding: test_groupnorm_act_vs_f64 holds both to the bar)."""
    from robomanipbaselines_amd import kernels as K

    for case in ("unit", "mean1e3"):
        x, w, b = _dev(*gn_inputs(B, C, T, G, case))
        xt = x.transpose(1, 2).contiguous()
        for mish in (False, True):
            y = K.groupnorm_act(x, w, b, G, 1e-5, mish=mish)
            yt = K.groupnorm_act(xt, w, b, G, 1e-5, mish=mish, time_major=True)
            xin = x.clone()
            out = K.groupnorm_act(xin, w, b, G, 1e-5, mish=mish, out=xin)
            assert out.data_ptr() == xin.data_ptr() and torch.equal(out, y)
            for i in range(B):
                assert torch.equal(K.groupnorm_act(x[i:i + 1].clone(), w, b, G, 1e-5, mish=mish)[0], y[i])
                alone = K.groupnorm_act(xt[i:i + 1].clone(), w, b, G, 1e-5, mish=mish, time_major=True)
                assert torch.equal(alone[0], yt[i])
