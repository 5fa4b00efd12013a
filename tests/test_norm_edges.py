"""Inputs, f64 references and the derived error bar of the normalisation-kernel edge tests
(tests/test_norm_edges_gpu.py), and the host test that keeps the inputs and the bar honest.

The reference is LayerNorm / GroupNorm (+ Mish) in f64 on the f32 or bf16 values exactly as the kernel
sees them (for LayerNorm s = x + r rounded to the storage dtype first).  With y^ = (s - mu) rstd in
f64, the per-element bar of an f32 output is

    bar = 2^-22 ( |w_c| ( max|s| rstd + |y^| ) + |b_c| )

max|s| over the normalised span (the row, or the (b, g) group).  max|s| rstd is the span's condition:
the error of s - mean when mean carries one f32 rounding of a value of size max|s|.  After Mish the
bar is 1.1 bar + 2^-22 |ref| (|mish'| <= 1.09), and a bf16 output adds 2^-8 |ref| (its own rounding).

The bar leaves about 2x over f32 arithmetic done in the right order and nothing for a one-pass
variance or a wrong divisor: test_torch_cpu_f32_stays_within_the_bar holds torch's CPU f32 kernels
to 0.6 of it on every case the GPU tests use.
"""

import pytest
import torch
import torch.nn.functional as F

U22 = 2.0 ** -22

# D of rmbx_add_layernorm, named for what each hits (a lane holds one vector of 4 f32 / 8 bf16 per
# pass, 64 lanes, PER passes):
LN_WIDTHS = {
    # 4 one live lane, 36 a partial wave, 256 / 512 / 1024 / 2048 full PER = 1 / 2 / 4 / 8,
    # 260 / 516 / 1028 the first widths of PER = 2 / 4 / 8 (the last pass holds one live lane)
    torch.float32: (4, 36, 256, 260, 512, 516, 1024, 1028, 2048),
    # 8 one live lane, 72 a partial wave, 512 / 1024 / 2048 full PER = 1 / 2 / 4, 520 / 1032 the
    # first widths of PER = 2 / 4
    torch.bfloat16: (8, 72, 512, 520, 1024, 1032, 2048),
}
LN_CASES = ("unit", "mean1e3", "const", "tiny", "huge", "spike", "r_none")
# one width per instantiation, also run with eps = 1e-3
LN_EPS3_WIDTHS = {torch.float32: (36, 260, 1024, 2048), torch.bfloat16: (72, 1024, 1032)}

# (B, C, T, G) of rmbx_groupnorm_act; the span E = (C / G) T switches paths at E <= 2048
GN_SHAPES = (
    (3, 46, 89, 2),  # E = 2047: the register path's last partial pass
    (3, 64, 64, 2),  # E = 2048: the register path, full
    (3, 6, 683, 2),  # E = 2049: the three-pass path's first span
    (2, 8, 1, 8),  # E = 1 (T = 1, cg = 1): the output is exactly b, or mish(b)
    (2, 6, 85, 2),  # E = 255: under one block
    (2, 8, 64, 2),  # E = 256: one block exactly
    (2, 2, 257, 2),  # E = 257, cg = 1: one element in the second pass
    (5, 4, 300, 4),  # E = 300, cg = 1
)
GN_CASES = ("unit", "mean1e3", "const", "tiny")


def ln_per(dtype, D):
    """The PER of the add_layernorm_kernel instantiation that D dispatches to."""
    nvec = D // (8 if dtype == torch.bfloat16 else 4)
    return next(p for p in (1, 2, 4, 8) if nvec <= 64 * p)


def ln_inputs(rows, D, dtype, case):
    """(x, r, w, b) on the host: x, r [rows, D] in `dtype` (r None for `r_none`), w, b f32 [D]."""
    g = torch.Generator().manual_seed(1000 * LN_CASES.index(case) + 8 * D + rows)
    x = 3.0 * torch.randn(rows, D, generator=g)
    r = torch.randn(rows, D, generator=g)
    w = 1.5 * torch.randn(D, generator=g)
    b = torch.randn(D, generator=g)
    if case == "mean1e3":
        x = x + 1000.0
    elif case == "const":  # every element of a row equal; D s and its partial sums are exact in f32
        x = (0.75 * torch.arange(1, rows + 1, dtype=torch.float32))[:, None].expand(rows, D).clone()
        r = torch.full((rows, D), 0.5)
    elif case == "tiny":  # var << eps
        x, r = x * 1e-6, r * 1e-6
    elif case == "huge":
        x, r = x * 1e6, r * 1e6
    elif case == "spike":  # one element 1e4 per row; row 0's is the row's last element (a tail lane)
        i = torch.arange(rows)
        x[i, (D - 1 + 37 * i) % D] = 1e4
    elif case == "r_none":
        x, r = x + 1.0, None
    return x.to(dtype), None if r is None else r.to(dtype), w, b


def ln_reference(x, r, w, b, eps):
    """(ref, bar) in f64 for the kernel's output dtype x.dtype."""
    s = x if r is None else x + r  # rounded to the storage dtype, as the kernel and the unfused add do
    sd, wd, bd = s.double(), w.double(), b.double()
    mu = sd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((sd - mu) ** 2).mean(-1, keepdim=True) + eps)
    yh = (sd - mu) * rstd
    ref = yh * wd + bd
    bar = U22 * (wd.abs() * (sd.abs().amax(-1, keepdim=True) * rstd + yh.abs()) + bd.abs())
    if x.dtype == torch.bfloat16:
        bar = bar + 2.0 ** -8 * ref.abs()
    return ref, bar


def gn_inputs(B, C, T, G, case):
    """(x [B, C, T], w [C], b [C]) f32 on the host."""
    g = torch.Generator().manual_seed(1000 * GN_CASES.index(case) + 64 * C + T)
    x = 3.0 * torch.randn(B, C, T, generator=g) + torch.randn(B, C, T, generator=g)
    w = 1.5 * torch.randn(C, generator=g)
    b = torch.randn(C, generator=g)
    if case == "mean1e3":
        x = x + 1000.0
    elif case == "const":  # one value per batch element
        x = (0.75 * torch.arange(1, B + 1, dtype=torch.float32) + 0.5)[:, None, None].expand(B, C, T).clone()
    elif case == "tiny":
        x = x * 1e-6
    return x, w, b


def gn_reference(x, w, b, G, eps, mish):
    """(ref, bar) in f64 of GroupNorm(G) (+ Mish) on x [B, C, T]."""
    B, C, T = x.shape
    xd = x.double().reshape(B, G, -1)
    wd, bd = w.double()[None, :, None], b.double()[None, :, None]
    mu = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + eps)
    yh = ((xd - mu) * rstd).reshape(B, C, T)
    cond = (xd.abs().amax(-1, keepdim=True) * rstd).expand(B, G, C // G * T).reshape(B, C, T)
    ref = yh * wd + bd
    bar = U22 * (wd.abs() * (cond + yh.abs()) + bd.abs())
    if mish:
        ref = F.mish(ref)
        bar = 1.1 * bar + U22 * ref.abs()
    return ref, bar


def worst_ratio(got, ref, bar):
    """max err / bar; inf where an element misses a zero bar or is not finite."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err <= bar, err / bar.clamp_min(1e-300), torch.full_like(err, float("inf")))
    return ratio.max().item()


def test_torch_cpu_f32_stays_within_the_bar():
    """torch's CPU f32 layer_norm / group_norm (+ mish) stay within 0.6 of the f32 bar on every
    (D, case) and (B, C, T, G, case) of the GPU tests: the inputs are fair and the bar is one that
    correct f32 arithmetic meets with room.  Worst measured: layer_norm 0.48 (f32 D = 36, spike, 1 row,
    eps 1e-3), group_norm 0.51 and group_norm + mish 0.48 (both (3, 46, 89, 2), mean1e3)."""
    worst = {}

    def note(kind, ratio, what):
        if ratio > worst.get(kind, (-1.0, None))[0]:
            worst[kind] = (ratio, what)

    for dtype, widths in LN_WIDTHS.items():
        for D in widths:
            for case in LN_CASES:
                for rows in (7, 1):
                    for eps in (1e-5, 1e-3) if D in LN_EPS3_WIDTHS[dtype] else (1e-5,):
                        x, r, w, b = ln_inputs(rows, D, dtype, case)
                        s = (x if r is None else x + r).float()
                        ref, bar = ln_reference(s, None, w, b, eps)  # the f32 bar on the rounded sum
                        note("layer_norm", worst_ratio(F.layer_norm(s, (D,), w, b, eps), ref, bar),
                             (str(dtype), D, case, rows, eps))
    for B, C, T, G in GN_SHAPES:
        for case in GN_CASES:
            x, w, b = gn_inputs(B, C, T, G, case)
            y = F.group_norm(x, G, w, b, 1e-5)
            note("group_norm", worst_ratio(y, *gn_reference(x, w, b, G, 1e-5, False)), (B, C, T, G, case))
            note("group_norm+mish", worst_ratio(F.mish(y), *gn_reference(x, w, b, G, 1e-5, True)), (B, C, T, G, case))
    for kind, (ratio, what) in worst.items():
        print(f"torch CPU f32 {kind}: worst err / bar {ratio:.3f} at {what}")
    for kind, (ratio, what) in worst.items():
        assert ratio <= 0.6, (kind, ratio, what)


@pytest.mark.parametrize("case", LN_CASES)
def test_layernorm_cases_are_what_they_claim(case):
    """The data cases keep the property each is named for after the rounding to the storage dtype."""
    for dtype in LN_WIDTHS:
        x, r, _, _ = ln_inputs(7, 260 if dtype == torch.float32 else 520, dtype, case)
        s = (x if r is None else x + r).double()
        mean, var = s.mean(-1), s.var(-1, unbiased=False)
        if case == "mean1e3":
            assert (mean > 990).all() and (var < 40).all()
        elif case == "const":
            assert (var == 0).all() and mean.unique().numel() == 7
        elif case == "tiny":
            assert (var < 1e-3 * 1e-5).all()
        elif case == "huge":
            assert (var > 1e12).all()
        elif case == "spike":
            assert (s.abs().amax(-1) > 9e3).all() and s[0].abs().argmax() == s.shape[1] - 1
        elif case == "r_none":
            assert r is None
