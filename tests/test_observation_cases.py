"""The inputs of tests/observation_cases.py reach the edges they are built for, shown on the oracles
alone (no device): the FPS tie scenes tie, in every stage of the kernel's reduction; the count,
bound and depth-value frames keep exactly the pixels they name; the resize geometries take the
branch they name; the SARNN cases cover every last-convolution group size and both packing
branches; every LSTM size has a reference-route error above zero to build its bar on."""

import copy

import numpy as np
import pytest
import torch

import observation_cases as C
from oracle import image as OI
from oracle import pointcloud as OP

THREADS, WAVE = 1024, 64  # rmbx_pointcloud_fps: pixel p is slot p // 1024 of lane p % 1024


def _tie_kinds(pix, ties):
    """Per stage of the kernel's argmax, the number of steps whose winner (the lowest tied index) ties
    with a pixel of the same lane / of another lane of its wave / of another wave."""
    kinds = {"lane": 0, "wave": 0, "block": 0}
    for t in ties:
        if len(t) < 2:
            continue
        p = pix[t]
        lane, others = p[0] % THREADS, p[1:] % THREADS
        kinds["lane"] += bool((others == lane).any())
        kinds["wave"] += bool(((others // WAVE == lane // WAVE) & (others != lane)).any())
        kinds["block"] += bool((others // WAVE != lane // WAVE).any())
    return kinds


def test_tie_scenes_tie_in_every_stage_of_the_reduction():
    lane_ties = 0
    for H, W, K in C.FPS_SIZES:
        for name in C.TIE_SCENES:
            d, rgb = C.tie_scene(name, H, W)
            pc, pix = C.cropped_cloud(d, rgb), C.kept_pixels(d, rgb)
            assert len(pix) == len(pc) > K
            idx, ties = C.fps_trace(pc, K)
            assert np.array_equal(idx, OP.fps_indices(pc, K))  # the trace is the oracle's loop
            steps = sum(len(t) >= 2 for t in ties)
            kinds = _tie_kinds(pix, ties)
            print(f"{H}x{W} {name}: {len(pc)} points, {steps} of {K} steps tied, {kinds}")
            assert steps >= C.MIN_TIE_STEPS, (H, W, name, steps)
            assert kinds["wave"] >= 5 and kinds["block"] >= 5, (H, W, name, kinds)
            lane_ties += kinds["lane"]
    assert lane_ties >= 3  # two slots of one lane tie only on the frames with more than 1024 pixels


def test_tie_scene_sizes_reach_the_slot_edges():
    assert [H * W for H, W, _ in C.FPS_SIZES] == [1024, 8192, 8190, 391]
    first = {}
    for H, W, _ in C.FPS_SIZES:
        d, rgb = C.tie_scene("late_start", H, W)
        p = int(C.kept_pixels(d, rgb)[0])
        first[H, W] = (p // THREADS, p % THREADS)
    # (slot, lane) of the first kept pixel: a later slot of a later lane on the two large frames
    assert first == {(32, 32): (0, 640), (64, 128): (2, 515), (90, 91): (1, 796), (17, 23): (0, 115)}


def test_count_cases_keep_what_they_name():
    cases = C.count_cases()
    for name, (d, rgb, K, kept) in cases.items():
        assert d.shape == (64, 128)
        norm, raw, count = C.observation(name, d, rgb, K)
        assert count == kept == len(C.kept_pixels(d, rgb)), name
        assert norm.shape == raw.shape == (K, 6)
    d, rgb, K, _ = cases["one_kept_last_pixel"]
    assert C.kept_pixels(d, rgb).tolist() == [64 * 128 - 1]  # slot 7 of lane 1023
    raw = C.observation("one_kept_last_pixel", d, rgb, K)[1]
    assert (raw == raw[0]).all()
    assert cases["exactly_K"][2] == cases["exactly_K"][3] and cases["K_plus_1"][2] + 1 == cases["K_plus_1"][3]
    d, rgb, K, kept = cases["K_9000_tail"]
    raw = C.observation("K_9000_tail", d, rgb, K)[1]
    assert K - kept > 8 * THREADS  # the tail loop wraps its 1024 threads
    assert (raw[kept:] == C.cropped_cloud(d, rgb)[-1]).all() and len(np.unique(raw[:kept], axis=0)) == kept
    # two kept pixels: both selected, then an all-zero round
    d, rgb, K, _ = cases["two_kept_K_8"]
    idx, ties = C.fps_trace(C.cropped_cloud(d, rgb), K)
    assert idx.tolist() == [0, 1] + [-1] * 6 and len(ties[1]) == 0
    # every round all-zero: point 0 again and again until the cloud's size is reached, then the last point
    d, rgb, K, kept = cases["zero_rounds"]
    pc = C.cropped_cloud(d, rgb)
    idx, ties = C.fps_trace(pc, K)
    assert idx.tolist() == [0] * 5 + [-1] * 3 and all(len(t) == 0 for t in ties)
    raw = C.observation("zero_rounds", d, rgb, K)[1]
    assert (raw[:5] == pc[0]).all() and (raw[5:] == pc[-1]).all() and not (pc[0] == pc[-1]).all()


def test_bound_cases_bind():
    d, rgb = C.bounds_frame()
    counts = {name: C.observation("bounds", d, rgb, 128, lo, hi)[2] for name, (lo, hi) in C.bound_cases().items()}
    counts["both"] = C.observation("bounds", d, rgb, 128)[2]
    valid = int(((0 < d) & (d < np.inf)).sum())
    assert counts["both"] < counts["max_only"] < counts["neither"] == valid
    assert counts["both"] < counts["min_only"] < counts["neither"]
    # strictness: z exactly on a bound is dropped, its f32 neighbour inside the bound is kept
    d, rgb = C.strict_frame()
    norm, raw, count = C.observation("strict", d, rgb, 8, C.Z_LO, C.HI)
    assert count == C.STRICT_KEPT
    assert sorted(set(raw[:, 2])) == sorted(float(z) for z in C.STRICT_DEPTHS[[3, 4, 5, 1]])
    assert float(C.STRICT_DEPTHS[1]) < 1.0 == float(C.STRICT_DEPTHS[0])
    assert float(C.STRICT_DEPTHS[3]) > 0.25 == float(C.STRICT_DEPTHS[2])


def test_odd_depth_values_only_the_subnormal_is_kept():
    d, rgb, ordinary = C.odd_depth_frame()
    flat = d.reshape(-1)
    assert np.isnan(flat).sum() == 1 and np.isposinf(flat).sum() == 1 and np.isneginf(flat).sum() == 1
    assert (np.signbit(flat) & (flat == 0)).sum() == 1 and (flat == np.float32(-0.7)).sum() == 1
    assert 0 < C.SUBNORMAL < np.finfo(np.float32).tiny
    norm, raw, count = C.observation("odd", d, rgb, 64)
    assert count == ordinary + 1
    assert (raw[:, 2] == float(C.SUBNORMAL)).sum() == 1 and np.isfinite(raw).all() and (raw[:, 2] > 0).all()


def test_mixed_batch_counts():
    d, rgb, K = C.mixed_batch()
    counts = [len(C.kept_pixels(d[e], rgb[e])) for e in range(4)]
    assert counts[0] == 1024 and K < counts[1] < 1024 and counts[2:] == [0, 1]


def test_resize_geometries_take_the_branch_they_name():
    area = [n for n, ((H, W, _), (rw, rh)) in C.RESIZE_GEOMETRY.items() if W == 2 * rw and H == 2 * rh]
    assert area == ["area"]
    (H, W, _), (rw, rh) = C.RESIZE_GEOMETRY["half_x_only"]
    assert W == 2 * rw and H != 2 * rh
    # identity: the oracle returns the source, u8 and f32
    assert np.array_equal(C.resized_u8("identity_c1"), C.u8_sources("identity_c1"))
    assert C.same_bits(C.resized_depth("identity_c1", False), C.depth_sources("identity_c1", False))
    # up-scaling clamps at both borders: weight 0 on the neighbour at either end
    s0, s1, fx, c0, c1 = OI._coords(84, 32)
    assert s0[0] == 0 and c0[0] == 2048 and s0[-1] == s1[-1] == 31 and c1[-1] == 0 and (c1[1:-2] > 0).any()
    assert sorted({C.RESIZE_GEOMETRY[n][0][2] for n in C.RESIZE_GEOMETRY}) == [1, 3, 4]
    for name, (_, (rw, rh)) in C.RESIZE_GEOMETRY.items():
        assert C.resized_u8(name).shape[1:3] == (rh, rw)
        assert (rh - 1, rw - 1, 1, 1) in C.crops(rw, rh) or (rw, rh) == (1, 1)


def test_special_depth_frames_carry_inf_zero_and_nan_through():
    for name in C.RESIZE_GEOMETRY:
        src, out = C.depth_sources(name, True), C.resized_depth(name, True)
        assert np.isposinf(src).any() and np.isnan(src).sum() == len(src)
        assert np.isnan(out).any() or name == "one_pixel", name  # its one sample lies in the inf patch
        if src.shape[1] > 2 and name != "one_pixel":  # one source row: inf * (1 - fy) + inf * 0 is NaN
            assert np.isposinf(out).any() and (out == 0).any(), name
        assert np.isfinite(C.resized_depth(name, False)).all()


def test_big_case_is_past_the_grid_cap():
    n, H, W, (rw, rh) = C.BIG
    assert n * rh * rw > C.GRID_CAP >= (n - 6) * rh * rw  # a second pass of the grid-stride loop, just


def test_sarnn_cases_cover_every_group_size_and_packing_branch():
    from robomanipbaselines_amd import kernels as Kn

    existing = [1, 5, 11]  # tests/test_sarnn_gpu.py
    assert {Kn.sarnn_conv_groups(K)[1] for K in existing} == {2, 6}
    new = sorted({K for _, K, _ in C.ATTENTION_CASES})
    assert {Kn.sarnn_conv_groups(K)[1] for K in new} == {4, 8}
    assert {K % 8 == 0 for K in new} == {True, False}
    assert {Kn.sarnn_conv_groups(K)[0] for K in new} == {1, 2}
    assert {n for _, _, n in C.ATTENTION_CASES} == {1, 2, 3, 4}
    assert min(S for S, _, _ in C.ATTENTION_CASES) == 8 and max(S for S, _, _ in C.ATTENTION_CASES) == 128


@pytest.mark.parametrize("K", sorted({K for _, K, _ in C.ATTENTION_CASES} | {1, 5, 11, 17}))
def test_sarnn_pack_attention_layout(K):
    """w3 [ncam][G][32][9][g]: channel G * g + j of the Conv2d weight at [cam, G, ci, tap, j], zero beyond
    K, at every group size and on both branches of sarnn_conv_groups."""
    from robomanipbaselines_amd import kernels as Kn

    torch.manual_seed(K)
    ncam = 2
    convs = [[torch.nn.Conv2d(ci, co, 3) for _ in range(ncam)] for ci, co in ((3, 16), (16, 32), (32, K))]
    packed = Kn.sarnn_pack_attention(convs)
    for layer, (w, b) in zip(convs, zip(packed[0::2], packed[1::2])):
        cout = layer[0].out_channels
        G, g = Kn.sarnn_conv_groups(cout)
        assert G * g >= cout and g % 2 == 0 and G == (cout + 7) // 8
        assert w.shape == (ncam, G, layer[0].in_channels, 9, g) and b.shape == (ncam, cout)
        for cam, m in enumerate(layer):
            flat = w[cam].permute(0, 3, 1, 2).reshape(G * g, -1, 3, 3)  # [channel][cin][3][3]
            assert torch.equal(flat[:cout], m.weight.detach()) and not flat[cout:].any()
            assert torch.equal(b[cam], m.bias.detach())


@pytest.mark.parametrize("S,K", C.KNOWN_ANSWER_CASES)
def test_constant_image_attends_to_the_centre(S, K):
    """Identical logits at every pixel: the softmax is uniform and every key the mean position,
    (0.5, 0.5), whatever the weights; the f32 positions col / (S - 7) are each within 2^-25 of the exact
    ones, so their mean is too."""
    model, images = C.constant_image_case(S, K)
    with torch.no_grad():
        keys = copy.deepcopy(model).double().attention_points(images.double())
    assert keys.shape == (3, 2, K, 2)
    assert float((keys - 0.5).abs().max()) <= 2.0 ** -25


@pytest.mark.parametrize("hd,sd,kd", C.LSTM_CASES)
def test_lstm_reference_route_error_is_measurable(hd, sd, kd):
    lstm, dec, xs, want, ref_err = C.lstm_case(hd, sd, kd)
    print(f"LSTM hidden {hd} state {sd} keys {kd}: torch-CPU fp32 error {ref_err:.3e}")
    assert lstm.weight_ih.shape == (4 * hd, sd + kd) and sd + kd <= 256 and hd <= 128
    assert len(xs) == len(want) == C.LSTM_STEPS and xs[0].shape == (C.LSTM_ENVS, sd + kd)
    assert 0.0 < ref_err < 1e-6
