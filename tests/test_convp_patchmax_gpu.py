"""The patch-staged conv picks each (tile, chunk) scale from the max |x| of the staged patch, reduced
per wave across its 64 lanes before one LDS atomic: a single large value must be found whichever
lane (and wave) stages it.  Missed, the scale comes from the small values around it, the large one
overflows its f16 piece and the outputs under it turn to inf / nan."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@torch.no_grad()
@pytest.mark.parametrize("Cout,H,W", [(64, 16, 32), (128, 16, 16)], ids=["tile_16x32_bn64", "tile_16x16_bn128"])
def test_patch_max_found_in_every_lane(Cout, H, W):
    """One tile, one 32-channel chunk; the staging item of pixel p (patch coordinates, one halo
    pixel around the tile) and channel quad c / 4 is p * 8 + c / 4, its lane that value mod 64."""
    from robomanipbaselines_amd import kernels as K

    g = torch.Generator(device="cpu").manual_seed(Cout)
    C, pw = 32, W + 2
    w = (torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    p = K.pack_conv_f32x6(w)
    base = torch.randn(1, C, H, W, generator=g).clamp_min(0)
    xs = []
    for lane in range(64):
        # a pixel whose item falls on this lane, starting the search at a row that varies with the
        # lane (so the items are spread over the waves too)
        y, x = next((yy % H, xx) for yy in range(5 * lane, 5 * lane + H) for xx in range(W)
                    if ((yy % H + 1) * pw + xx + 1) % 8 == lane >> 3)
        assert (((y + 1) * pw + x + 1) * 8 + (lane & 7)) % 64 == lane
        xi = base.clone()
        xi[0, 4 * (lane & 7), y, x] = 3.0e4
        xs.append(xi)
    x = torch.cat(xs).to(DEV).contiguous(memory_format=torch.channels_last)
    got = K.conv3x3_f16x3_patch(x, p, b, relu=False, res=None)
    ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
    for lane in range(64):
        e = ((got[lane].double() - ref[lane]).abs().max() / ref[lane].abs().max()).item()
        assert e <= 2e-6, (lane, e)  # the bound of test_convp_gpu.py
