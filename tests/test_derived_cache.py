"""policy.derived.derived (the one cache of parameter-derived operands) and the route table of the
fused f32 ResNet-18 trunk (policy.backbone.block_routes), on the CPU."""

import pytest
import torch
import torch.nn as nn

from robomanipbaselines_amd import kernels as K
from robomanipbaselines_amd.policy.backbone import FusedResNet18Trunk, ResNet18Trunk, _FusedBlock, _FusedConv
from robomanipbaselines_amd.policy.derived import derived


class _Counted:
    """build() of a doubled weight (+ bias), counting its calls."""

    def __init__(self, lin):
        self.lin, self.calls = lin, 0

    def __call__(self):
        self.calls += 1
        w, b = self.lin.weight, self.lin.bias
        return w.detach().float() * 2 if b is None else (w.detach().float() * 2, b.detach().float() * 2)


def _get(lin, build, **kw):
    return derived(lin, "twice", (lin.weight, lin.bias), build, **kw)


def test_hit_returns_the_same_object_without_building():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    a = _get(lin, build)
    b = _get(lin, build)
    assert a is b and build.calls == 1


@torch.no_grad()
def test_rebuilds_after_copy_into_a_source():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    _get(lin, build)
    lin.bias.copy_(torch.arange(4.0))
    w2, b2 = _get(lin, build)
    assert build.calls == 2 and torch.equal(b2, 2 * torch.arange(4.0))
    lin.weight.copy_(torch.ones(4, 3))
    w2, b2 = _get(lin, build)
    assert build.calls == 3 and torch.equal(w2, torch.full((4, 3), 2.0))


def test_rebuilds_after_load_state_dict():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    _get(lin, build)
    ptr = lin.weight.data_ptr()
    lin.load_state_dict({"weight": torch.full((4, 3), 3.0), "bias": torch.zeros(4)})
    assert lin.weight.data_ptr() == ptr  # in place: only the version tells
    w2, _ = _get(lin, build)
    assert build.calls == 2 and torch.equal(w2, torch.full((4, 3), 6.0))


def test_rebuilds_after_to_dtype():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    _get(lin, build)
    lin.to(torch.bfloat16)
    w2, _ = _get(lin, build)
    assert build.calls == 2 and torch.equal(w2, lin.weight.detach().float() * 2)


def test_rebuilds_when_extra_changes():
    lin = nn.Linear(3, 4)
    build = _Counted(lin)
    _get(lin, build, extra=("f4",))
    _get(lin, build, extra=("f4",))
    assert build.calls == 1
    _get(lin, build, extra=("f2",))
    assert build.calls == 2


def test_rebuilds_when_a_none_source_becomes_a_tensor():
    lin = nn.Linear(3, 4, bias=False)
    build = _Counted(lin)
    assert isinstance(_get(lin, build), torch.Tensor)
    assert isinstance(_get(lin, build), torch.Tensor) and build.calls == 1
    lin.bias = nn.Parameter(torch.ones(4))
    _, b2 = _get(lin, build)
    assert build.calls == 2 and torch.equal(b2, torch.full((4,), 2.0))


def test_two_slots_on_one_owner_do_not_collide():
    lin = nn.Linear(3, 4)
    a = derived(lin, "a", (lin.weight,), lambda: "A")
    b = derived(lin, "b", (lin.weight,), lambda: "B")
    assert (a, b) == ("A", "B")
    assert derived(lin, "a", (lin.weight,), lambda: "A2") == "A" and derived(lin, "b", (lin.weight,), lambda: "B2") == "B"


# ---- the stale values a reload used to leave behind ---------------------------------------------

def _random_state(module, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g).to(v.dtype) for k, v in module.state_dict().items()}


@torch.no_grad()
def test_bias_sum_follows_load_state_dict():
    fused = FusedResNet18Trunk(ResNet18Trunk())
    blk = fused.blocks[2]
    blk._bias_sum()
    fused.load_state_dict(_random_state(fused, 1))
    assert torch.equal(blk._bias_sum(), blk.c2.conv.bias + blk.down.conv.bias)


@torch.no_grad()
def test_bf16_bias_f32_follows_load_state_dict():
    fused = FusedResNet18Trunk(ResNet18Trunk()).to(torch.bfloat16)
    conv = fused.blocks[0].c1
    conv.bias_f32()
    fused.load_state_dict(_random_state(fused, 2))
    got = conv.bias_f32()
    assert got.dtype == torch.float32 and torch.equal(got, conv.conv.bias.float())
    assert conv.conv.bias.abs().max() > 0


@torch.no_grad()
def test_bf16_norm_f32_follows_load_state_dict():
    from robomanipbaselines_amd.policy.act.act_model import _LayerOps

    norm = nn.LayerNorm(16).to(torch.bfloat16)
    _LayerOps._norm_f32(norm)
    norm.load_state_dict(_random_state(norm, 3))
    w, b = _LayerOps._norm_f32(norm)
    assert w.dtype == b.dtype == torch.float32
    assert torch.equal(w, norm.weight.float()) and torch.equal(b, norm.bias.float())
    assert not torch.equal(w, torch.ones(16))


# ---- the route table ----------------------------------------------------------------------------
# Expected tables: the parent commit's predicates (wino_ok, x6_ok, s1_patch_ok, s1_gemm_ok,
# rmbx_f32_ok and the branches of _FusedBlock.forward) evaluated by hand for ResNet-18's convs.

_S1 = {64: ["layer1.0.conv1", "layer1.0.conv2", "layer1.1.conv1", "layer1.1.conv2"],
       128: ["layer2.0.conv2", "layer2.1.conv1", "layer2.1.conv2"],
       256: ["layer3.0.conv2", "layer3.1.conv1", "layer3.1.conv2"],
       512: ["layer4.0.conv2", "layer4.1.conv1", "layer4.1.conv2"]}
_S2 = ["layer2.0.conv1", "layer2.0.downsample", "layer3.0.conv1", "layer3.0.downsample",
       "layer4.0.conv1", "layer4.0.downsample"]


def _table(c64, c128, c256, c512, s2):
    t = {n: s2 for n in _S2}
    for c, r in ((64, c64), (128, c128), (256, c256), (512, c512)):
        t.update({n: r for n in _S1[c]})
    return t


_DEFAULT = _table("patch", "patch", "wino_x6", "wino_x6", "x6")
_DIRECT = _table("nhwc", "miopen", "miopen", "miopen", "miopen")

_CASES = {
    "default": ({}, _DEFAULT),
    "no_wino_x6": ({"WINO_X6": False}, _table("patch", "patch", "wino_f4", "wino_f4", "x6")),
    "no_patch": ({"S1_PATCH_CHANNELS": ()}, _table("wino_f4", "gemm", "wino_x6", "wino_x6", "x6")),
    "no_patch_no_gemm": ({"S1_PATCH_CHANNELS": (), "S1_GEMM_CHANNELS": ()},
                         _table("wino_f4", "wino_f4", "wino_x6", "wino_x6", "x6")),
    # (behind the default patch / wino_x6 routes no conv is left on the fused Winograd kernel)
    "tile_f2": ({"WINO_TILE": "f2"}, _DEFAULT),
    "tile_f2_alone": ({"WINO_TILE": "f2", "WINO_X6": False, "S1_PATCH_CHANNELS": (), "S1_GEMM_CHANNELS": ()},
                      _table("wino_f2", "wino_f2", "wino_f2", "wino_f2", "x6")),
    "direct": ({"F32_CONV": "direct"}, _DIRECT),
    "s2_miopen": ({"F32_CONV_S2": "miopen"}, _table("patch", "patch", "wino_x6", "wino_x6", "miopen")),
    "bf16x6": ({"F32_PIECES": "bf16x6"}, _table("wino_f4", "wino_f4", "wino_x6", "wino_x6", "x6")),
}


def set_knobs(monkeypatch, knobs):
    for name, value in knobs.items():
        owner = K if name == "F32_PIECES" else _FusedBlock if name.startswith("F32_CONV") else _FusedConv
        monkeypatch.setattr(owner, name, value)


@pytest.mark.parametrize("case", list(_CASES))
def test_f32_route_table(monkeypatch, case):
    knobs, want = _CASES[case]
    set_knobs(monkeypatch, {"WINO_TILE": "f4", "WINO_X6": True, "S1_GEMM_CHANNELS": (128,), "S1_PATCH_CHANNELS": (64, 128),
                            "F32_CONV": "winograd", "F32_CONV_S2": "x6", "F32_PIECES": "f16x3"})  # the defaults
    set_knobs(monkeypatch, knobs)
    got = FusedResNet18Trunk(ResNet18Trunk()).routes(torch.float32)
    assert len(want) == 19 and got == want

