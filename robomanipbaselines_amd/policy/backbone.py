"""ResNet-18 trunk with frozen batch norm (torchvision.models.resnet18 + FrozenBatchNorm2d, the
backbone of ACT's DETR (third_party/act, absent from the reference checkout) and of MlpPolicy
(policy/mlp/MlpPolicy.py:34-39)).  torchvision is not installed here, so the network is
restated; parameter names follow torchvision's (conv1, bn1, layer1.0.conv1, ...) so a reference
state_dict maps onto it.  `fuse()` folds each frozen BN into its conv for the MIOpen/MFMA
inference path (channels_last, bf16); the unfused module is the fp32 reference.

Which kernel a block conv of the fused trunk runs is decided in one place, `block_routes`; every
operand computed from a parameter (widened and summed biases, packed planes, filter transforms,
the stem forms) is held through `derived.derived`, so weights may be reloaded after a run."""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import kernels as K
from .derived import derived


class FrozenBatchNorm2d(nn.Module):
    """torchvision.ops.misc.FrozenBatchNorm2d: y = (x - rm) / sqrt(rv + eps) * w + b."""

    def __init__(self, n, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))

    def scale_shift(self):
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        return scale, self.bias - self.running_mean * scale

    def forward(self, x):
        s, b = self.scale_shift()
        return x * s.reshape(1, -1, 1, 1) + b.reshape(1, -1, 1, 1)


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = FrozenBatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = FrozenBatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), FrozenBatchNorm2d(cout))

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return F.relu(y + idt)


class ResNet18Trunk(nn.Module):
    """conv1..layer4 (no avgpool/fc): [B,3,H,W] -> [B,512,H/32,W/32]."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = FrozenBatchNorm2d(64)
        self.layer1 = nn.Sequential(BasicBlock(64, 64, 1), BasicBlock(64, 64, 1))
        self.layer2 = nn.Sequential(BasicBlock(64, 128, 2), BasicBlock(128, 128, 1))
        self.layer3 = nn.Sequential(BasicBlock(128, 256, 2), BasicBlock(256, 256, 1))
        self.layer4 = nn.Sequential(BasicBlock(256, 512, 2), BasicBlock(512, 512, 1))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.max_pool2d(x, 3, 2, 1)
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))


# ---- the route table of the fused trunk's block convs ------------------------------------------
#
# route      kernel                                                     packed operand
# patch      rmbx_conv3x3_f16x3_patch, epilogue fused                   pack_conv_f32x6
# gemm, x6   rmbx_conv2d_f16x3 / rmbx_conv2d_f32x6 (implicit GEMM)      pack_conv_f32x6
# wino_x6    explicit Winograd F(4x4, 3x3), 36 rmbx_linear_f32x6 GEMMs  pack_wino4_x6
# wino_f4    rmbx_conv3x3_winograd4_f32 (fused F(4x4, 3x3), f32 MFMA)   pack_winograd4_f32
# wino_f2    rmbx_conv3x3_winograd_f32 (fused F(2x2, 3x3), f32 MFMA)    pack_winograd_f32
# nhwc       rmbx_conv2d_nhwc (bf16) / rmbx_conv2d_nhwc_f32             the channels_last weight
# miopen     F.conv2d + one rmbx nhwc_bias_act epilogue pass            none
#
# With the default knobs an f32 ResNet-18 runs: layer 1, layer 2.1 and c2 of 2.0 on `patch`; the
# stride-2 c1 and the 1x1 downsample of 2.0 / 3.0 / 4.0 on `x6`; every stride-1 conv of layers 3
# and 4 on `wino_x6`.  A bf16 one runs layers 1-2 on `nhwc` and layers 3-4 on `miopen`.
#
# The knobs (class attributes below, each read from its RMBX_* variable at import) and the
# measurements behind their defaults, all on MI355X at 1024 frames:
#   _FusedBlock.F32_CONV (RMBX_F32_CONV) "winograd": the rmbx stride-1 routes for every layer;
#     "direct": layer 1 on rmbx_conv2d_nhwc_f32 (the f32 MIOpen solvers need a separate
#     bias/residual/ReLU pass and a split-K zero fill per conv), layers 2-4 on MIOpen.
#   _FusedBlock.F32_CONV_S2 (RMBX_F32_CONV_S2) "x6": the stride-2 c1 and the 1x1 downsample on the
#     fp32-accurate implicit GEMM; "miopen": MIOpen + the epilogue pass.  Either way c2 adds the
#     downsample branch and both biases in its epilogue.
#   _FusedConv.S1_PATCH_CHANNELS (RMBX_S1_PATCH, "" = none) 64,128: the patch-staged f16x3 conv
#     splits each input pixel once per output tile instead of once per tap -- 64 channels at
#     120 x 160: 6.86 ms vs 7.70 for the fused Winograd (and 10x closer to f64); 128 channels at
#     60 x 80: 4.93 vs 5.34 ms for the implicit GEMM (profiles/r4_conv3x3_patch_ab.log).
#   _FusedConv.S1_GEMM_CHANNELS (RMBX_S1_GEMM, "" = none) 128: behind `patch`, the implicit GEMM
#     instead of the fused Winograd: at 128 channels (60 x 80) 5.1 vs 6.3 ms per conv, 18,559 vs
#     18,178 env-steps/s (profiles/r4_bench_s1gemm128_ab.log); 64 channels stay off it: on the
#     GEMM's 64-column tile 9.1 vs 7.7 ms per conv (18,366 vs 18,826 env-steps/s,
#     profiles/r4_conv64_gemm_bn64_vs_winograd.log, r4_bench_s1gemm64_ab.log).
#   _FusedConv.WINO_X6 (RMBX_WINO_X6) on: the 256/512-channel stride-1 convs as the explicit
#     Winograd on rmbx_linear_f32x6 (kernels.conv3x3_wino4_x6); 0 keeps them on the fused kernel.
#   _FusedConv.WINO_TILE (RMBX_WINO_TILE) "f4": 2.25 instead of 4 products per output, ACT call
#     240.5 -> 232.1 ms (profiles/r3_bench_f4b.json.log); "f2": F(2x2, 3x3).
#   kernels.F32_PIECES "f16x3": `patch` and `gemm` exist in that piece form only.
#   _FusedBlock.RMBX_CONV_MAX_COUT 128: bf16 implicit-GEMM convs where they beat MIOpen + epilogue
#     (scripts/prof_conv.py, profiles/r1_prof_conv_v3.log: layer1 2.7 vs 4.0 ms, layer2 2.0 vs
#     2.6 ms per conv); MIOpen's tuned solvers still win for the 256/512-channel layers.


def _wino_ok(c):
    return (c.in_channels == c.out_channels and c.in_channels in K.WINOGRAD_F32_CHANNELS
            and tuple(c.kernel_size) == (3, 3) and c.stride[0] == 1 and c.padding[0] == 1)


def _x6_ok(c, f16x3):
    return (c.stride[0] == c.stride[1] and c.padding[0] == c.padding[1]
            and K.conv2d_f32x6_supported(c.in_channels, c.out_channels, f16x3))


def _s1_route(c, k):
    """The route of a stride-1 3x3 conv that _wino_ok."""
    f16x3 = k["F32_PIECES"] == "f16x3"
    if (c.out_channels in k["S1_PATCH_CHANNELS"] and f16x3 and c.in_channels % 32 == 0 and c.out_channels % 64 == 0
            and tuple(c.stride) == (1, 1) and tuple(c.padding) == (1, 1) and tuple(c.dilation) == (1, 1)
            and c.groups == 1):
        return "patch"
    if c.out_channels in k["S1_GEMM_CHANNELS"] and f16x3 and _x6_ok(c, f16x3):
        return "gemm"
    if k["WINO_X6"] and c.out_channels in K.WINO_X6_CHANNELS:
        return "wino_x6"
    return "wino_f4" if k["WINO_TILE"] == "f4" else "wino_f2"


def block_routes(dtype, c1, c2, down, k):
    """(route of c1, route of c2, route of the downsample or None) of one basic block: a pure function
    of the three nn.Conv2d geometries (down may be None), the activation dtype and the knobs k (see
    knobs()).  Route names: the table above."""
    f16x3 = k["F32_PIECES"] == "f16x3"
    if dtype == torch.float32 and k["F32_CONV"] == "winograd" and _wino_ok(c2):
        if down is None and _wino_ok(c1):
            return _s1_route(c1, k), _s1_route(c2, k), None
        if down is not None:
            s2 = "x6" if k["F32_CONV_S2"] == "x6" and _x6_ok(c1, f16x3) and _x6_ok(down, f16x3) else "miopen"
            return s2, _s1_route(c2, k), s2
    if dtype == torch.bfloat16 and c2.out_channels <= k["RMBX_CONV_MAX_COUT"]:
        return "nhwc", "nhwc", None if down is None else "nhwc"
    if dtype == torch.float32 and down is None and all(
            K.conv2d_nhwc_f32_supported(c.in_channels, c.out_channels, c.kernel_size, c.stride[0], c.padding[0])
            for c in (c1, c2)):
        return "nhwc", "nhwc", None
    return "miopen", "miopen", None if down is None else "miopen"


def knobs():
    """The current value of every knob block_routes reads."""
    k = {n: getattr(_FusedConv, n) for n in ("WINO_TILE", "WINO_X6", "S1_GEMM_CHANNELS", "S1_PATCH_CHANNELS")}
    k.update({n: getattr(_FusedBlock, n) for n in ("F32_CONV", "F32_CONV_S2", "RMBX_CONV_MAX_COUT")})
    k["F32_PIECES"] = K.F32_PIECES
    return k


class _FusedConv(nn.Module):
    """conv + folded frozen BN.  The conv runs without bias (MIOpen, MFMA); bias, residual and
    ReLU are applied by the rmbx HIP epilogue in one pass over the output."""

    WINO_TILE = os.environ.get("RMBX_WINO_TILE", "f4")
    WINO_X6 = os.environ.get("RMBX_WINO_X6", "1") != "0"
    S1_GEMM_CHANNELS = tuple(int(c) for c in os.environ.get("RMBX_S1_GEMM", "128").split(",") if c)
    S1_PATCH_CHANNELS = tuple(int(c) for c in os.environ.get("RMBX_S1_PATCH", "64,128").split(",") if c)

    # bench.py's Winograd probe: a list to which s1() appends (shape, tile, HIP events around the
    # launch) for the fused Winograd routes, on the current stream; None = no events
    PROBE = None

    def __init__(self, conv, bn, relu):
        super().__init__()
        s, b = bn.scale_shift()
        w = conv.weight.detach() * s.reshape(-1, 1, 1, 1)
        self.conv = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, bias=True)
        self.conv.weight.data.copy_(w)
        self.conv.bias.data.copy_(b.detach())
        self.relu = relu

    def conv_nobias(self, x):
        c = self.conv
        return F.conv2d(x, c.weight, None, c.stride, c.padding)

    def bias_f32(self):
        """The bias in the storage dtype, widened to f32 for the epilogue."""
        b = self.conv.bias
        return derived(self, "bias_f32", (b,), lambda: b.detach().float().contiguous())

    def forward(self, x):
        y = self.conv_nobias(x)
        return K.nhwc_bias_act(y, self.bias_f32(), relu=self.relu, out=y)

    def rmbx(self, x, relu, res=None):
        """conv + bias (+ res) (+ ReLU) in one rmbx implicit-GEMM launch (bf16, or f32 for the
        layer-1 shape): route `nhwc`."""
        c = self.conv
        w = c.weight
        if not w.is_contiguous(memory_format=torch.channels_last):
            w = w.contiguous(memory_format=torch.channels_last)
        return K.conv2d_nhwc(x, w, self.bias_f32(), c.stride[0], c.padding[0], relu=relu, res=res)

    def _planes(self):
        w = self.conv.weight
        return derived(self, "x6", (w,), lambda: K.pack_conv_f32x6(w))

    def x6(self, x, relu, res=None, bias=True):
        """f32 conv (+ bias) (+ res) (+ ReLU) as one fp32-accurate implicit-GEMM launch
        (rmbx_conv2d_f16x3 / rmbx_conv2d_f32x6 by kernels.F32_PIECES, epilogue fused): routes `x6`
        and `gemm`.  bias=False: no bias, a tensor: that bias."""
        c = self.conv
        if not isinstance(bias, torch.Tensor):
            bias = self.bias_f32() if bias else None
        return K.conv2d_f32x6(x, self._planes(), bias, c.kernel_size, c.stride[0], c.padding[0], relu=relu, res=res)

    def s1(self, route, x, relu, res=None, bias=None):
        """A stride-1 3x3 conv of the f32 trunk + bias (its own, or `bias`) (+ res) (+ ReLU) in one
        launch on its route: patch, gemm, wino_x6, wino_f4 or wino_f2."""
        b = self.bias_f32() if bias is None else bias
        if route == "patch":
            return K.conv3x3_f16x3_patch(x, self._planes(), b, relu=relu, res=res)
        if route == "gemm":
            return self.x6(x, relu, res=res, bias=b)
        w = self.conv.weight
        pack, fn = {"wino_x6": (K.pack_wino4_x6, K.conv3x3_wino4_x6),
                    "wino_f4": (K.pack_winograd4_f32, K.conv3x3_winograd4_f32),
                    "wino_f2": (K.pack_winograd_f32, K.conv3x3_winograd_f32)}[route]
        u = derived(self, "wino", (w,), lambda: pack(w), extra=route)
        probe = _FusedConv.PROBE
        if probe is None or route == "wino_x6":
            return fn(x, u, b, relu=relu, res=res)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(x, u, b, relu=relu, res=res)
        e1.record()
        probe.append((tuple(x.shape), route[-2:], e0, e1))
        return out


class _FusedBlock(nn.Module):
    RMBX_CONV_MAX_COUT = 128
    F32_CONV = os.environ.get("RMBX_F32_CONV", "winograd")
    F32_CONV_S2 = os.environ.get("RMBX_F32_CONV_S2", "x6")

    def __init__(self, blk):
        super().__init__()
        self.c1 = _FusedConv(blk.conv1, blk.bn1, True)
        self.c2 = _FusedConv(blk.conv2, blk.bn2, False)
        self.down = None if blk.downsample is None else _FusedConv(blk.downsample[0], blk.downsample[1], False)

    def routes(self, dtype):
        return block_routes(dtype, self.c1.conv, self.c2.conv, None if self.down is None else self.down.conv, knobs())

    def _bias_sum(self):
        """c2's bias + the downsample's (the residual's bias folded into c2's epilogue)."""
        return derived(self, "bias_sum", (self.c2.conv.bias, self.down.conv.bias),
                       lambda: (self.c2.bias_f32() + self.down.bias_f32()).contiguous())

    def forward(self, x):
        c1, c2, down = self.c1, self.c2, self.down
        r1, r2, _ = self.routes(x.dtype)
        if r2 == "nhwc":
            y = c1.rmbx(x, relu=True)
            idt = x if down is None else down.rmbx(x, relu=False)
            return c2.rmbx(y, relu=True, res=idt)
        if r2 == "miopen":
            y = c1(x)
            z = c2.conv_nobias(y)
            if down is None:
                return K.nhwc_bias_act(z, c2.bias_f32(), res=x, relu=True, out=z)
            d = down.conv_nobias(x)
            return K.nhwc_bias_act(z, c2.bias_f32(), res=d, res_bias=down.bias_f32(), relu=True, out=z)
        # the f32 rmbx stride-1 routes
        if down is None:
            return c2.s1(r2, c1.s1(r1, x, relu=True), relu=True, res=x)
        # c2 adds the downsample branch and both biases in its epilogue
        if r1 == "x6":
            y = c1.x6(x, relu=True)
            d = down.x6(x, relu=False, bias=False)
        else:
            y = c1(x)
            d = down.conv_nobias(x)
        return c2.s1(r2, y, relu=True, res=d, bias=self._bias_sum())


class FusedResNet18Trunk(nn.Module):
    """Inference form on the device: BN folded into conv weights/bias, channels_last activations;
    the same function as ResNet18Trunk.  Each block conv runs the route block_routes names for it
    (the table above it; `routes(dtype)` lists them), bias / residual / ReLU in the kernel's
    epilogue on every rmbx route and in one rmbx pass behind MIOpen.  By default, bf16: layers 1-2
    on the rmbx MFMA implicit GEMM (rmbx_conv2d_nhwc), layers 3-4 on MIOpen; f32: the stride-1 3x3
    convs on the patch-staged f16x3 conv (64 and 128 channels) and the explicit Winograd F(4x4, 3x3)
    over fp32-accurate GEMMs (256 and 512), the stride-2 convs and 1x1 downsamples on the
    fp32-accurate implicit GEMM.  The 3-channel 7x7 stem is MIOpen + the rmbx bias/ReLU/max-pool
    epilogue, or one rmbx kernel on the renderer's space-to-depth images (forward_s2d,
    forward_s2d_u8).  The epilogues are bit-identical to the unfused storage-dtype sequence on the
    same conv outputs (tests/test_nn_gpu.py)."""

    def __init__(self, trunk):
        super().__init__()
        self.stem = _FusedConv(trunk.conv1, trunk.bn1, True)
        blocks = []
        for layer in (trunk.layer1, trunk.layer2, trunk.layer3, trunk.layer4):
            blocks += [_FusedBlock(b) for b in layer]
        self.blocks = nn.Sequential(*blocks)

    def routes(self, dtype):
        """{"layer1.0.conv1": route, ..., "layer2.0.downsample": route, ...} (ResNet18Trunk's names)."""
        out = {}
        for i, blk in enumerate(self.blocks):
            for name, r in zip(("conv1", "conv2", "downsample"), blk.routes(dtype)):
                if r is not None:
                    out[f"layer{i // 2 + 1}.{i % 2}.{name}"] = r
        return out

    def forward(self, x):
        s = self.stem.conv_nobias(x)
        return self.blocks(K.nhwc_bias_relu_maxpool(s, self.stem.bias_f32()))

    def forward_s2d_u8(self, x_u8, mean, std):
        """The f32 trunk on the renderer's 8-bit space-to-depth image [n, H/2, W/2, 16] u8
        (policy_dtype 4): the image normalisation x = (u / 255 - mean) / std is folded into the stem
        (rmbx_stem_s2d_conv_maxpool_u8: exact bf16 integer pixels x three exact bf16 pieces of
        W / (255 std), f32 accumulation, the mean term in the bias and the border edge table)."""
        w, b = self.stem.conv.weight, self.stem.conv.bias
        if w.dtype != torch.float32 or w.shape[0] != 64 or x_u8.shape[2] > K.STEM_POOL_MAX_WS:
            raise ValueError("forward_s2d_u8: needs the f32 64-channel stem and Ws <= STEM_POOL_MAX_WS")
        ops = derived(self, "stem_u8", (w, b), lambda: K.pack_stem_u8(w, b, mean, std), extra=(tuple(mean), tuple(std)))
        return self.blocks(K.stem_s2d_conv_maxpool_u8(x_u8, *ops))

    def forward_s2d(self, x_s2d):
        """Same function on the renderer's 2x2 space-to-depth image [B, H/2, W/2, 16] (bf16 or
        f32): conv + bias + ReLU + max-pool in one rmbx MFMA kernel (rmbx_stem_s2d_conv_maxpool
        / _f32); wider bf16 images: rmbx_stem_s2d_conv then the max-pool."""
        w = self.stem.conv.weight
        w_s2d, zero = derived(self, "stem_s2d", (w,), lambda: (
            K.pack_stem_s2d(w.detach()), torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)))
        if w.shape[0] == 64 and x_s2d.shape[2] <= K.STEM_POOL_MAX_WS:
            # conv + bias + ReLU + max-pool in one kernel: the full-resolution stem map stays on chip
            return self.blocks(K.stem_s2d_conv_maxpool(x_s2d, w_s2d, self.stem.bias_f32()))
        if x_s2d.dtype != torch.bfloat16:
            raise ValueError(f"forward_s2d: f32 images wider than {2 * K.STEM_POOL_MAX_WS} pixels are not supported")
        s = K.stem_s2d_conv(x_s2d, w_s2d, self.stem.bias_f32(), relu=True)
        return self.blocks(K.nhwc_bias_relu_maxpool(s, zero))
