"""rmbx_resize_crop_u8 / rmbx_resize_f32 at their edges, bitwise against oracle/image.py on the
geometries of tests/observation_cases.py: up-scaling (both border clamps), identity, shrinking one axis
while growing the other, a one-row source, C = 1 and 4, the 2x area path and 2x in x alone (bilinear),
a 1x1 target; full, far-corner and ragged crops into every output dtype; depth frames with +inf, 0 and
NaN (NaN positions compared as such, every other element bit for bit); 600 frames, whose 4 233 600 output
pixels take a second pass of the grid-stride loop; an empty batch; rejections before any launch."""

import numpy as np
import pytest
import torch

import observation_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("dtype", list(C.RESIZE_DTYPES))
@pytest.mark.parametrize("name", list(C.RESIZE_GEOMETRY))
def test_resize_crop_u8_edges(name, dtype):
    from robomanipbaselines_amd import kernels as K

    size = C.RESIZE_GEOMETRY[name][1]
    src = torch.from_numpy(C.u8_sources(name)).to(DEV)
    for crop in C.crops(*size):
        y0, x0, ch, cw = crop
        got = K.resize_crop_u8(src, size, crop, *C.AFFINE, dtype=C.RESIZE_DTYPES[dtype]).cpu()
        if dtype == "u8":  # the resized frame itself, HWC, unscaled
            assert np.array_equal(got.numpy(), C.resized_u8(name)[:, y0:y0 + ch, x0:x0 + cw]), crop
            continue
        want = C.policy_u8(name, crop)
        if dtype == "f32":
            assert C.same_bits(got.numpy(), want), crop
        else:
            assert torch.equal(got, torch.from_numpy(want).to(torch.bfloat16)), crop
    if name == "identity_c1" and dtype == "u8":
        assert torch.equal(K.resize_crop_u8(src, size, dtype=torch.uint8), src)


@pytest.mark.parametrize("special", [False, True], ids=["finite", "inf_zero_nan"])
@pytest.mark.parametrize("name", list(C.RESIZE_GEOMETRY))
def test_resize_f32_edges(name, special):
    from robomanipbaselines_amd import kernels as K

    src = C.depth_sources(name, special)
    got = K.resize_f32(torch.from_numpy(src).to(DEV), C.RESIZE_GEOMETRY[name][1]).cpu().numpy()
    want = C.resized_depth(name, special)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert C.same_bits(got, want)


def test_resize_past_the_grid_cap():
    from robomanipbaselines_amd import kernels as K

    size = C.BIG[3]
    src, want = C.big_u8()
    got = K.resize_crop_u8(torch.from_numpy(src).to(DEV), size, None, *C.AFFINE).cpu().numpy()
    assert got.size // 3 > C.GRID_CAP
    bad = np.flatnonzero((got != want).any(axis=(1, 2, 3)))
    assert bad.size == 0, f"u8 -> f32: {bad.size} of {len(src)} frames differ, first {bad[0]}"
    src, want = C.big_depth()
    got = K.resize_f32(torch.from_numpy(src).to(DEV), size).cpu().numpy()
    assert got.size > C.GRID_CAP
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert bad.size == 0, f"f32: {bad.size} of {len(src)} frames differ, first {bad[0]}"


def test_resize_empty_batch():
    from robomanipbaselines_amd import kernels as K

    for dtype, shape in ((torch.float32, (0, 3, 84, 84)), (torch.bfloat16, (0, 3, 84, 84)),
                         (torch.uint8, (0, 84, 84, 3))):
        out = K.resize_crop_u8(torch.empty((0, 24, 32, 3), dtype=torch.uint8, device=DEV), (84, 84), dtype=dtype)
        assert out.shape == shape and out.dtype == dtype
    assert K.resize_f32(torch.empty((0, 24, 32), device=DEV), (84, 84)).shape == (0, 84, 84)


def test_resize_rejections():
    """Each raises before a launch: the sentinel-filled `out` keeps its bits."""
    from robomanipbaselines_amd import kernels as K

    src = torch.zeros((1, 24, 32, 3), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, 8, 8), 7.25, device=DEV)
    for crop in ((77, 0, 8, 8), (0, 77, 8, 8), (-1, 0, 8, 8), (0, -1, 8, 8)):  # 77 + 8 = 85 > 84
        with pytest.raises(ValueError, match="outside 84x84"):
            K.resize_crop_u8(src, (84, 84), crop, out=out)
    with pytest.raises(ValueError, match="bad sizes"):
        K.resize_crop_u8(torch.zeros((1, 24, 32, 5), dtype=torch.uint8, device=DEV), (84, 84), (0, 0, 8, 8),
                         out=torch.full((1, 5, 8, 8), 7.25, device=DEV))
    for dtype in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="dtype must be"):
            K.resize_crop_u8(src, (84, 84), dtype=dtype)
    with pytest.raises(ValueError, match="out must have shape"):
        K.resize_crop_u8(src, (84, 84), (0, 0, 8, 9), out=out)
    with pytest.raises(ValueError, match="out must be"):
        K.resize_crop_u8(src, (84, 84), (0, 0, 8, 8), dtype=torch.bfloat16, out=out)
    dsrc = torch.zeros((1, 24, 32), device=DEV)
    dout = torch.full((1, 84, 83), 7.25, device=DEV)
    with pytest.raises(ValueError, match="out must have shape"):
        K.resize_f32(dsrc, (84, 84), out=dout)
    with pytest.raises(ValueError, match="src must be"):
        K.resize_f32(dsrc.double(), (84, 84))
    with pytest.raises(ValueError, match="bad sizes"):
        K.resize_f32(dsrc, (0, 84))
    torch.cuda.synchronize()
    assert bool((out == 7.25).all()) and bool((dout == 7.25).all())
