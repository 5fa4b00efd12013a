"""Replay CLI: render recorded steps of one traced episode as camera images.

  python -m robomanipbaselines_amd.bin.Replay TRACE_DIR --episode 4117 [--steps last | all | k1 k2 ...]
      [--cameras front side ...] [--shadows off|scene] [--offsamples 1|4|scene] [--output_image_dir D]
      [--as_seen]

A trace row (--trace_dir of bin/Rollout.py, common/episode_trace.py) holds the four per-env arrays
the renderer reads.  The renderer's output does not depend on the batch, so the chosen rows are
drawn in one call per camera with the steps as the batch dimension, and every image is bit for bit
the frame of the live step.  The cameras go side by side, as --save_last_image writes them, to
Rollout<Policy>_<Env>_world<idx>_<success|failure>_ep<episode>_step<k>.png.

--as_seen (a run recorded with --perturb): the header's perturbation is applied to the re-rendered
frame with the row's episode and rollout_time_idx, the keys the live run used, so the image of a step
the policy read is the frame it read (the trace itself holds the clean scene).

A run recorded with --camera_jitter: the header's spec and seed give every recorded episode's camera
rows again (keyed by the episode, not by the slot it ran in); they are drawn and bound before
rendering, so the frames stay the live step's.  --as_seen composes with it.
"""

import argparse
import os
import sys
import types

import numpy as np

from ..common.episode_trace import TraceReader

# device bytes one replay batch may take (images, the renderer's per-pixel workspaces): a long
# episode is drawn in several batches of steps
BATCH_BYTES = 256 * 2**20


def select_rows(rows, steps):
    """Indices into the episode's rows for --steps: ["last"], ["all"] or step numbers.  ValueError
    naming the recorded steps for a step that has no row (dropped by the stride, or past the end)."""
    have = rows["step"]
    steps = [str(s) for s in steps]
    if steps == ["all"]:
        return np.arange(len(have))
    try:
        want = [int(have[-1]) if s == "last" else int(s) for s in steps]
    except ValueError:
        raise ValueError(f"--steps takes `last`, `all` or step numbers, not {steps}") from None
    where = {int(k): i for i, k in enumerate(have)}
    missing = [k for k in want if k not in where]
    if missing:
        raise ValueError(f"step(s) {missing} of episode {int(rows['episode'][0])} were not recorded; "
                         f"recorded steps: {_ranges(have)}")
    return np.array([where[k] for k in want])


def _ranges(steps):
    """1, 2, 3, 6, 9 -> '1-3, 6, 9'"""
    out, steps = [], [int(s) for s in steps]
    i = 0
    while i < len(steps):
        j = i
        while j + 1 < len(steps) and steps[j + 1] == steps[j] + 1:
            j += 1
        out.append(str(steps[i]) if i == j else f"{steps[i]}-{steps[j]}")
        i = j + 1
    return ", ".join(out)


def make_renderer(header, device, shadows=None, offsamples=None):
    """The Renderer of the recording run: the header's model and image size, and its shadows and
    offsamples settings unless given (resolved against the scene as the env does)."""
    from .. import model as MD
    from ..render import Renderer, samples_of, scene_casts_shadows, scene_offsamples

    arrays = MD.load(header["model_name"])
    shadows = header["shadows"] if shadows is None else shadows
    offsamples = header["offsamples"] if offsamples is None else offsamples
    samples = samples_of(scene_offsamples(arrays)) if offsamples == "scene" else int(offsamples)
    H, W = header["image_size"]
    return Renderer(arrays, device, width=W, height=H, shadows=shadows == "scene" and scene_casts_shadows(arrays),
                    samples=samples)


def as_seen_of(header):
    """The (spec, seed, camera list) --as_seen applies: the recording run's --perturb.  ValueError for
    a trace recorded without it."""
    from ..common.perturb import spec_from_dict

    if header.get("perturb") is None:
        raise ValueError("--as_seen needs a trace recorded with --perturb: this trace's header has no `perturb` key "
                         "(the policy read the clean frames, which Replay draws without --as_seen)")
    return spec_from_dict(header["perturb"]), int(header["seed"]) & (2**64 - 1), list(header["camera_names"])


def camera_jitter_of(header):
    """The (spec, seed) of the recording run's --camera_jitter, or None for a trace recorded without it."""
    from ..common.camera_jitter import spec_from_dict

    if header.get("camera_jitter") is None:
        return None
    return spec_from_dict(header["camera_jitter"]), int(header["seed"]) & (2**64 - 1)


def render_rows(renderer, rows, idx, cameras, device, batch_bytes=BATCH_BYTES, as_seen=None, camera_jitter=None):
    """u8 [len(idx), H, W * len(cameras), 3] host array: the rows `idx` of the episode drawn by every
    camera, the cameras side by side.  The steps are the renderer's batch, in batches that fit.
    as_seen: as_seen_of(header), to perturb every frame as the policy of the recording run saw it.
    camera_jitter: camera_jitter_of(header), to render every step with its episode's camera rows."""
    import torch

    from .. import kernels as K

    H, W = renderer.height, renderer.width
    ngeom, nbody = rows["gxpos"].shape[1], rows["xpos"].shape[1]
    # per step: one rgb frame in flight, and per pixel the visibility keys (8 B), a camera's static
    # cache (8 B) and the sample sums (4 B)
    per_step = H * W * (3 + 8 + 8 * len(cameras) + 4) + 8 * (12 * ngeom + 7 * nbody)
    batch = int(max(1, min(len(idx), batch_bytes // per_step)))
    out = np.empty((len(idx), H, W * len(cameras), 3), np.uint8)
    for b0 in range(0, len(idx), batch):
        sel = idx[b0:b0 + batch]
        t = len(sel)
        dev = {k: torch.from_numpy(np.ascontiguousarray(rows[k][sel])).to(device) for k in ("gxpos", "gxmat", "xpos", "xquat")}
        eng = types.SimpleNamespace(n_env=t, ngeom=ngeom, nbody=nbody, **dev)
        rgb = torch.empty((t, H, W, 3), dtype=torch.uint8, device=device)
        if camera_jitter is not None:
            # the batch's steps are the renderer's envs: each gets the rows of its episode
            spec, seed = camera_jitter
            episode = torch.from_numpy(np.ascontiguousarray(rows["episode"][sel], dtype=np.int32)).to(device)
            cam_rows = torch.empty((len(renderer.cam_names), t, 8), dtype=torch.float64, device=device)
            P, T, F = spec.strengths()
            K.camera_jitter_draw(seed, episode, cam_rows, pos=float(P), tan_half_rot=float(T), fovy=float(F))
            renderer.bind_camera_rows(cam_rows)
        for c, cam in enumerate(cameras):
            renderer.render(eng, cam, rgb=rgb)
            if as_seen is not None and as_seen[0].touches_images:
                spec, seed, scene_cameras = as_seen
                episode = torch.from_numpy(np.ascontiguousarray(rows["episode"][sel], dtype=np.int32)).to(device)
                draw = torch.from_numpy(np.ascontiguousarray(rows["rollout_time_idx"][sel], dtype=np.int32)).to(device)
                occ_h, occ_w = spec.occ_size(H, W)
                K.image_perturb(rgb, seed, episode, draw, scene_cameras.index(cam), brightness=spec.brightness,
                                contrast=spec.contrast, gain=spec.gain, noise=spec.noise, occ_h=occ_h, occ_w=occ_w,
                                rgb_out=rgb)
            out[b0:b0 + t, :, c * W:(c + 1) * W] = rgb.cpu().numpy()
    if camera_jitter is not None:
        renderer.bind_camera_rows(None)
    return out


def image_name(header, record, step):
    outcome = "success" if record["success"] else "failure"
    return (f"Rollout{header['policy']}_{header['env']}_world{int(record['world_idx']):0>1}_{outcome}_"
            f"ep{int(record['episode'])}_step{int(step)}.png")


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("trace_dir", type=str, help="the --trace_dir of the recording run")
    parser.add_argument("--episode", type=int, required=True, help="global episode index")
    parser.add_argument("--steps", type=str, nargs="+", default=["last"],
                        help="`last`, `all` or the env-step numbers (1 = the episode's first step)")
    parser.add_argument("--cameras", type=str, nargs="+", default=None, help="default: every camera of the scene")
    parser.add_argument("--shadows", choices=["off", "scene"], default=None, help="default: the recording run's")
    parser.add_argument("--offsamples", choices=["1", "4", "scene"], default=None, help="default: the recording run's")
    parser.add_argument("--output_image_dir", type=str, default=".")
    parser.add_argument("--device", type=str, default="cuda:0")
    parser.add_argument("--as_seen", action="store_true",
                        help="apply the recording run's --perturb to the frames: what the policy read")
    args = parser.parse_args(argv)
    # everything that can be wrong with the request is found before the device is touched
    reader = TraceReader(args.trace_dir)
    record = reader.record(args.episode)
    rows = reader.episode(args.episode)
    idx = select_rows(rows, args.steps)
    header = reader.header
    cameras = list(args.cameras) if args.cameras else list(header["camera_names"])
    unknown = [c for c in cameras if c not in header["camera_names"]]
    if unknown:
        raise ValueError(f"unknown camera(s) {unknown}; the scene has {header['camera_names']}")
    as_seen = as_seen_of(header) if args.as_seen else None
    camera_jitter = camera_jitter_of(header)
    from ..common.image_io import write_png

    renderer = make_renderer(header, args.device, args.shadows, args.offsamples)
    os.makedirs(args.output_image_dir, exist_ok=True)
    paths = []
    H, W = renderer.height, renderer.width
    # (one batch of images on the host at a time as well)
    per_image = H * W * len(cameras) * 3
    group = int(max(1, BATCH_BYTES // per_image))
    for g0 in range(0, len(idx), group):
        part = idx[g0:g0 + group]
        images = render_rows(renderer, rows, part, cameras, args.device, as_seen=as_seen, camera_jitter=camera_jitter)
        for i, image in zip(part, images):
            path = os.path.abspath(os.path.join(args.output_image_dir, image_name(header, record, rows["step"][i])))
            write_png(path, image)
            print(f"[Replay] Save the observation image of step {int(rows['step'][i])}: {path}")
            paths.append(path)
    return paths


if __name__ == "__main__":
    main(sys.argv[1:])
