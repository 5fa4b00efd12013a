"""Batched rollout plugin base: n_env environments step in lockstep on one GPU.

Mirrors common/base/RolloutBase.py of the reference (hook names, argparse flags, phase
semantics, results schema) for a batch of envs:

* phases: InitialRolloutPhase (1.0 s), the Operation's pre-motion phases (timed reach/grasp),
  RolloutPhase (policy every `skip` steps, success latch, +1.0 s after success or max_duration,
  --auto_exit), EndRolloutPhase — RolloutBase.py:28-132, PhaseBase.py:41-106.  All phase
  transitions are driven by the simulation clock, so the pre-rollout schedule is identical for
  every env and is tracked on the host; per-env termination/results live in the device
  schedule (rmbx_sched_update).
* the step loop (RolloutBase.py:387-426): pre_update -> env action -> env.step ->
  post_update -> check_transition, with cv2.waitKey / plotting removed (headless).
* results: {"success": [...], "reward": [...], "duration": [...]} per env in env order, the
  `Rollout result: success|failure` stdout contract (RolloutBase.py:96-107) and the optional
  YAML file (RolloutBase.py:417-422); inference-duration statistics (RolloutBase.py:528-539).
* streaming (--num_episodes M, run_streaming / step_stream): the n envs are slots that work through
  a queue of M >= n episodes; a finished slot is recorded, given the next episode and re-armed on
  the device (rmbx_episode_recycle) at the end of steps aligned to P = skip x the policy's
  inference period, so every slot keeps the host's skip / inference phase and the policy runs on
  all n rows at the lockstep shapes ("Streaming").  Results: M entries in episode
  order.  The lockstep entry points (run, step_once, reset) are untouched by it.
"""

import argparse
import datetime
import os
import sys
import time

import numpy as np
import torch
import yaml

from .. import kernels as K
from ..common import episode_metrics as EM
from ..common.data_key import DataKey, action_key_codes, state_key_codes
from ..common.data_utils import make_meta_info
from ..common.episode_trace import TraceWriter, parse_episodes, row_bytes, select_mask
from ..common import actuation as ACT
from ..common import camera_jitter as CJ
from ..common import dynamics as DYN
from ..common.perturb import Perturber, parse_spec


class PhaseSpec:
    """Timed phase of the pre-rollout motion (PhaseBase.ReachPhaseBase / GraspPhaseBase)."""

    def __init__(self, name, duration, kind, pos_z=None, grip=None, target=None):
        # grip: gripper command of a grasp phase (None = action_space.high, set_target_close;
        # "low" = action_space.low, set_target_open; or a value)
        # target: reach phases of tasks other than the cable: callable(rollout) -> (R [n, 9],
        # p [n, 3]) f64 device tensors, the phase's set_target (evaluated when the phase starts)
        self.name, self.duration, self.kind, self.pos_z, self.grip = name, duration, kind, pos_z, grip
        self.target = target


class BatchedRolloutBase:
    require_task_desc = False
    policy_name = "Policy"

    def __init__(self, argv=None, **overrides):
        self.setup_args(argv=argv)
        for k, v in overrides.items():
            setattr(self.args, k, v)
        # the parsed --perturb spec (None: off); ValueError for a bad key or value
        self.perturb_spec = None if getattr(self.args, "perturb", None) is None else parse_spec(self.args.perturb)
        # the parsed --actuation spec (None: off); ValueError for a bad key or value
        self.actuation_spec = (None if getattr(self.args, "actuation", None) is None
                               else ACT.parse_spec(self.args.actuation))
        # the parsed --dynamics spec (None: off); ValueError for a bad key or value
        self.dynamics_spec = (None if getattr(self.args, "dynamics", None) is None
                              else DYN.parse_spec(self.args.dynamics))
        # the parsed --camera_jitter spec (None: off); ValueError for a bad key or value
        self.camera_jitter_spec = (None if getattr(self.args, "camera_jitter", None) is None
                                   else CJ.parse_spec(self.args.camera_jitter))
        torch.manual_seed(self.args.seed)
        np.random.seed(self.args.seed)
        self.device = torch.device(self.args.device)
        self.setup_env()
        self.setup_model_meta_info()
        self.setup_policy()
        self.n = self.env.num_envs
        self.pre_phases = self.get_pre_motion_phases()
        self.pre_durations = [1.0] + [p.duration for p in self.pre_phases]  # Initial phase: 1.0 s
        self.result = {key: [] for key in ("success", "reward", "duration")}
        self.inference_duration_list = []
        self._infer_events = []
        self.datetime_now = datetime.datetime.now()
        self._active = None  # optional caller override of the per-env step mask
        self.phase_timer = None  # optional PhaseTimer (common/phase_timer.py): bench.py's per-phase split
        self._trace = None  # the TraceWriter of a run with --trace_dir
        self._metrics = None  # the kernels.EpisodeMetrics accumulator of a run with --episode_metrics
        self._perturb = None  # the common.perturb.Perturber of a run with --perturb
        self._actuation = None  # the common.actuation.Actuator of a run with --actuation
        self._dynamics = None  # the common.dynamics.Dynamics of a run with --dynamics
        self._camera_jitter = None  # the common.camera_jitter.CameraJitter of a run with --camera_jitter

    def attach_phase_timer(self, timer):
        """Record HIP events at the policy / render / physics / glue boundaries of every env-step
        (None detaches)."""
        self.phase_timer = timer
        self.env.phase_timer = timer

    def _mark(self, label):
        if self.phase_timer is not None:
            self.phase_timer.mark(label)

    # -- arguments (RolloutBase.setup_args :165-284 + batching flags) --------------------------
    def setup_args(self, parser=None, argv=None):
        if parser is None:
            parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
        parser.add_argument("--checkpoint", type=str, default=None, help="checkpoint file (random init if omitted)")
        parser.add_argument("--world_idx", type=int, default=0)
        parser.add_argument("--world_idx_list", type=int, nargs="*", default=None)
        parser.add_argument("--world_random_scale", nargs="+", type=float, default=None)
        parser.add_argument("--skip", type=int, default=None)
        parser.add_argument("--skip_draw", type=int, default=None)
        parser.add_argument("--seed", type=int, default=0)
        parser.add_argument("--no_render", action="store_true")
        parser.add_argument("--no_plot", action="store_true")
        parser.add_argument("--win_xy_plot", type=int, nargs=2)
        parser.add_argument("--wait_before_start", action="store_true")
        parser.add_argument("--auto_exit", action="store_true")
        parser.add_argument("--max_duration", type=float, default=30.0)
        parser.add_argument("--result_filename", type=str, default=None)
        parser.add_argument("--save_last_image", action="store_true")
        parser.add_argument("--output_image_dir", type=str, default=".")
        parser.add_argument("--shadows", choices=["off", "scene"], default="off",
                            help="scene: the camera images carry the hard shadows of the scene's light where its "
                                 "<light> casts them (the Cable, Ring and Pick scenes), as the reference's renders "
                                 "do; off (default): no shadows")
        parser.add_argument("--offsamples", choices=["1", "4", "scene"], default="1",
                            help="samples per pixel of the camera images: 4 averages the 4x rotated-grid samples "
                                 "(anti-aliased edges, as the reference's multisampled offscreen renders); scene: "
                                 "the scene's <visual><quality offsamples> (MuJoCo's default 4; a value other than "
                                 "0, 1 or 4 is refused); 1 (default): one ray through each pixel centre")
        # batching (this engine)
        parser.add_argument("--num_envs", type=int, default=None,
                            help="environments stepped in lockstep (default: one per --world_idx_list entry, "
                                 "the episodes the reference runs one after another)")
        parser.add_argument("--device", type=str, default="cuda:0")
        parser.add_argument("--precision", choices=["fp32", "bf16"], default="fp32",
                            help="policy arithmetic: fp32 (the reference's precision, the default) or bf16 "
                                 "(opt-in throughput mode, ~1e-3 action error)")
        parser.add_argument("--max_steps", type=int, default=None, help="hard cap on env-steps")
        parser.add_argument("--num_gpus", type=int, default=1,
                            help="shard the envs over this many GPUs of the node (bin/Rollout.py launches one "
                                 "process per GPU; results all-gathered over RCCL)")
        parser.add_argument("--tactile", action="store_true",
                            help="scenes with tactile pads: info['intensity_tactile'] every env-step")
        parser.add_argument("--state_keys", type=str, nargs="*", default=None,
                            help="synthetic runs (no --checkpoint) only: state keys of the synthetic model meta "
                                 "info (TrainBase --state_keys; default measured_joint_pos)")
        parser.add_argument("--action_keys", type=str, nargs="+", default=None,
                            help="synthetic runs (no --checkpoint) only: action keys of the synthetic model meta "
                                 "info (TrainBase --action_keys; default command_joint_pos)")
        parser.add_argument("--env_offset", type=int, default=0,
                            help="global index of local env 0 (this rank's shard start under --num_gpus): world "
                                 "indices and noise streams follow the global env index")
        parser.add_argument("--num_episodes", type=int, default=None,
                            help="streaming mode: evaluate this many episodes on min(--num_envs, M) env slots; a "
                                 "finished slot is recorded, reset and given the next episode on the device. "
                                 "Episode i uses world_idx_list[i %% len] and the noise stream (seed, i), as env i "
                                 "of a lockstep run does. Not with --save_last_image: a recycled slot no longer "
                                 "holds its episode's last frame")
        parser.add_argument("--episode_offset", type=int, default=0,
                            help="global index of this process's first episode (its shard start under --num_gpus), "
                                 "the role --env_offset plays for envs")
        parser.add_argument("--trace_dir", type=str, default=None,
                            help="record the trajectory of every traced episode on the device and write it "
                                 "here (common/episode_trace.py); bin/Replay.py renders any recorded step, the "
                                 "last frame of a streamed episode included. Under --num_gpus each rank writes "
                                 "rank<r>/ below it")
        parser.add_argument("--trace_episodes", type=str, nargs="+", default=["all"],
                            help="with --trace_dir: `all` or the global indices of the episodes to record")
        parser.add_argument("--trace_stride", type=int, default=1,
                            help="with --trace_dir: keep every K-th env-step of an episode and its last step; "
                                 "K = --skip keeps the steps whose frames the policy read")
        parser.add_argument("--episode_metrics", action="store_true",
                            help="accumulate per-episode metrics of the RolloutPhase on the device (steps to first "
                                 "success, peak wrist force / torque, peak joint speed and tracking error, gripper and "
                                 "joint path lengths, command roughness): a `metrics` key in the result file and a "
                                 "summary with the success rate's Wilson interval after the statistics")
        parser.add_argument("--perturb", type=str, nargs="+", default=None, metavar="KEY=VALUE",
                            help="perturb what the policy observes, per episode and on the device (the rule: "
                                 "include/rmbx.h, rmbx_image_perturb): brightness=LEVELS contrast=C gain=G (C, G in "
                                 "[0, 1)), noise=LEVELS (sensor noise), occluder=F (a rectangle of F x each image "
                                 "side), state_noise=S (normalised units). An episode sees the same perturbation in "
                                 "any slot, shard or re-run; info['rgb_images'], saved images and the trace stay clean")
        parser.add_argument("--actuation", type=str, nargs="+", default=None, metavar="KEY=VALUE",
                            help="perturb the command the robot executes, per episode and on the device (the rule: "
                                 "include/rmbx.h, rmbx_action_perturb): noise=S bias=B (normalised action units: "
                                 "per-inference Gaussian noise, episode-constant offset uniform in +-B), delay=D "
                                 "(env-steps of control latency, 0..64), hold=P (probability that a step's command "
                                 "is lost and the last one stays). An episode is actuated the same way in any slot, "
                                 "shard or re-run; ctrl, the trace and the metrics show the executed command")
        parser.add_argument("--dynamics", type=str, nargs="+", default=None, metavar="KEY=VALUE",
                            help="randomise the world's physical constants per episode, on the device (the rule: "
                                 "include/rmbx.h, rmbx_dynamics_draw): friction=F damping=D mass=M gain=G, each in "
                                 "[0, 1): the contact friction, the objects' joint damping, the objects' mass and "
                                 "inertia, and the servo gains (kp, kv) are multiplied by a factor uniform in "
                                 "(1 - S, 1 + S). An episode meets the same world in any slot, shard or re-run; "
                                 "common.dynamics.scales(seed, episodes, spec) gives the factors on the host")
        parser.add_argument("--camera_jitter", type=str, nargs="+", default=None, metavar="KEY=VALUE",
                            help="jitter every camera's pose and field of view per episode, in the renderer (the "
                                 "rule: include/rmbx.h, rmbx_camera_jitter_draw): pos=P (metres, [0, 0.5]: each "
                                 "component of the mount's displacement uniform in +-P), rot=R (degrees, [0, 30]: a "
                                 "rotation about the camera's own axes, below R per axis), fovy=F ([0, 0.5): fovy "
                                 "times a factor uniform in (1 - F, 1 + F)). An episode sees the same cameras in any "
                                 "slot, shard or re-run; common.camera_jitter.rows(seed, episodes, spec, ncam) gives "
                                 "the rows on the host. The point cloud of DiffusionPolicy3d is still unprojected "
                                 "with the nominal fovy: the policy believes the calibrated intrinsics")
        if self.require_task_desc:
            parser.add_argument("--task_desc", type=str, required=True)
        self.set_additional_args(parser)
        if argv is None:
            argv = sys.argv[1:]
        self.args = parser.parse_args(argv)
        if self.args.world_idx_list is None:
            self.args.world_idx_list = [self.args.world_idx]
        if self.args.num_envs is None:
            self.args.num_envs = len(self.args.world_idx_list)
        if self.args.world_random_scale is not None:
            self.args.world_random_scale = np.array(self.args.world_random_scale)
        self.args.auto_exit = True  # headless batched evaluation always auto-exits
        if self.args.trace_stride < 1:
            raise ValueError("--trace_stride must be at least 1")
        parse_episodes(self.args.trace_episodes)  # ValueError for anything but `all` or indices
        if self.args.perturb is not None:
            parse_spec(self.args.perturb)  # ValueError for a bad key or value
        if self.args.actuation is not None:
            ACT.parse_spec(self.args.actuation)  # ValueError for a bad key or value
        if self.args.dynamics is not None:
            DYN.parse_spec(self.args.dynamics)  # ValueError for a bad key or value
        if self.args.camera_jitter is not None:
            CJ.parse_spec(self.args.camera_jitter)  # ValueError for a bad key or value
        if self.args.num_episodes is not None:
            if self.args.num_episodes < 1:
                raise ValueError("--num_episodes must be at least 1")
            if self.args.save_last_image:
                raise ValueError("--save_last_image cannot be combined with --num_episodes: a recycled env slot no "
                                 "longer holds the last frame of the episodes it ran")
            # the slots: never more than the episodes; slot e starts with episode episode_offset + e,
            # which is what a lockstep reset gives env e at this env_offset
            self.args.num_envs = min(self.args.num_envs, self.args.num_episodes)
            self.args.env_offset = self.args.episode_offset

    def set_additional_args(self, parser):
        pass

    def setup_model_meta_info(self):
        self.model_meta_info = make_meta_info(self)
        self.state_keys = self.model_meta_info["state"]["keys"]
        self.action_keys = self.model_meta_info["action"]["keys"]
        self.camera_names = self.model_meta_info["image"]["camera_names"]
        self.state_dim = len(self.model_meta_info["state"]["example"])
        self.action_dim = len(self.model_meta_info["action"]["example"])
        # device routing codes; unsupported keys raise ValueError as MotionManager does
        self._state_codes = state_key_codes(self.state_keys)
        self._action_codes = action_key_codes(self.action_keys)
        for what, keys, dim in (("state", self.state_keys, self.state_dim), ("action", self.action_keys, self.action_dim)):
            kd = sum(DataKey.get_dim(k, self.env) for k in keys)
            if kd != dim:
                raise ValueError(f"{what} keys {keys} have dimension {kd}, the model meta info {dim}")
        if self.args.skip is None:
            self.args.skip = self.model_meta_info["data"]["skip"]
        if self.args.skip_draw is None:
            self.args.skip_draw = self.args.skip

    def setup_env(self):
        raise NotImplementedError("defined by the Operation mixin")

    def setup_policy(self):
        raise NotImplementedError

    def get_pre_motion_phases(self):
        return []

    def reset_variables(self):
        pass

    def infer_policy(self):
        raise NotImplementedError

    def draw_plot(self):
        pass

    # -- state / images (RolloutBase.get_state :463-477, get_images :479-490) -----------------
    def _bind_state_stats(self):
        """The state normalisation statistics as f64 device tensors (read once per episode)."""
        st, dev = self.model_meta_info["state"], self.device
        if "mean" in st:
            self._st_mean = torch.tensor(st["mean"], dtype=torch.float64, device=dev)
            self._st_std = torch.tensor(st["std"], dtype=torch.float64, device=dev)
        if "min" in st:
            self._st_min = torch.tensor(st["min"], dtype=torch.float64, device=dev)
            self._st_range = torch.tensor(st["range"], dtype=torch.float64, device=dev)

    def get_raw_state(self):
        """RolloutBase.get_state's key concatenation (:463-473): MotionManager.get_data of every
        state key in order, f64 [n, state_dim], on the device (rmbx_motion_state)."""
        if not self.state_keys:
            return torch.zeros((self.n, 0), dtype=torch.float64, device=self.device)
        return K.motion_state(self._placement, self.obs, self.q_cmd, self.grip_cmd, self._tgt_R, self._tgt_p,
                              self._state_codes, self.state_dim)

    def get_state(self):
        """RolloutBase.get_state (:463-477): the routed state, normalised, as f32 [n, state_dim]
        (--perturb state_noise: plus the episode's state noise of this observation)."""
        s = self.normalize_state(self.get_raw_state())
        if getattr(self, "_perturb", None) is not None:
            s = self._perturb_rows().state(s)
        return s

    def normalize_state(self, x):
        """normalize_data (DataUtils.py:9-24) in f64 (same operations and order as numpy), then the
        f32 cast of RolloutBase.get_state (:475)."""
        if x.shape[-1] == 0:
            return x.to(torch.float32)
        st = self.model_meta_info["state"]
        if st.get("norm_config", {}).get("type", "gaussian") == "gaussian":
            return ((x - self._st_mean) / self._st_std).to(torch.float32)
        scale = (st["norm_config"]["out_max"] - st["norm_config"]["out_min"]) / self._st_range
        return (scale * (x - self._st_min) + st["norm_config"]["out_min"]).to(torch.float32)

    # per-channel (mean, std) the renderer applies to [0, 1] pixels for the policy tensor:
    # identity = RolloutBase.image_transforms (v2.ToDtype(float32, scale=True), :353); the ACT
    # policy overrides it with its ImageNet normalisation
    image_norm = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))

    def get_images(self, dtype):
        """RolloutBase.get_images (:479-490): stack info["rgb_images"][camera] of every policy
        camera -> CHW -> ToDtype(scale) (and the policy's image normalisation).  Fused: every
        policy camera of the current state is rendered straight into the normalised policy tensor
        [n,ncam,3,H,W] (or, for a device policy that accepts it, the bf16 / f32 / 8-bit
        space-to-depth form [n,ncam,H/2,W/2,16] its fused stem kernel reads) -- the same values as
        normalising info["rgb_images"] (tests/test_env_info_gpu.py), without the u8 frame round
        trip through HBM."""
        H, W = self.env.renderer.height, self.env.renderer.width
        mean, std = self.image_norm
        # (the fused f32 stem kernel takes space-to-depth rows of at most STEM_POOL_MAX_WS: wider
        # f32 images go through the NCHW path)
        s2d = (dtype in (torch.bfloat16, torch.float32) and self.device.type == "cuda"
               and getattr(self.policy, "accepts_s2d", False) and H % 2 == 0 and W % 2 == 0
               and (dtype == torch.bfloat16 or W // 2 <= K.STEM_POOL_MAX_WS))
        shape = (H // 2, W // 2, 16) if s2d else (3, H, W)
        if s2d and dtype == torch.float32 and getattr(self.policy, "accepts_u8_s2d", False):
            # the f32 policy folds mean / std into its stem: the renderer hands over the 8-bit values
            dtype = torch.uint8
        if getattr(self, "_img", None) is None or self._img.dtype != dtype or tuple(self._img.shape[2:]) != shape:
            self._img = torch.empty((self.n, len(self.camera_names)) + shape, dtype=dtype, device=self.device)
            self._img_cam = [torch.empty((self.n,) + shape, dtype=dtype, device=self.device) for _ in self.camera_names]
        self._mark("render")
        if getattr(self, "_perturb", None) is not None and self.perturb_spec.touches_images:
            # the clean u8 frame is rendered, and the kernel writes the policy form of the perturbed one
            pt = self._perturb_rows()
            for i, cam in enumerate(self.camera_names):
                rgb = self.info["rgb_images"][cam]
                if len(self.camera_names) == 1:
                    pt.policy(cam, rgb, self._img.view((self.n,) + shape), mean, std)
                else:
                    pt.policy(cam, rgb, self._img_cam[i], mean, std)
                    self._img[:, i].copy_(self._img_cam[i])
        elif len(self.camera_names) == 1:
            self.env.render_images(self.camera_names[0], policy=self._img.view((self.n,) + shape), mean=mean, std=std)
        else:
            for i, cam in enumerate(self.camera_names):
                self.env.render_images(cam, policy=self._img_cam[i], mean=mean, std=std)
                self._img[:, i].copy_(self._img_cam[i])
        self._mark("policy")
        return self._img

    # -- observation perturbation (--perturb) ------------------------------------------------------
    def _perturb_begin(self):
        """The Perturber of this run, and its one printed line."""
        r = self.env.renderer
        self._perturb = Perturber(self.perturb_spec, self.args.seed, self.n, r.height, r.width, self.env.camera_names,
                                  self.device)
        self._lockstep_rows_begin()
        print(f"[{self.__class__.__name__}] Perturb: {self.perturb_spec}", flush=True)

    def _lockstep_rows_begin(self):
        """The episodes of a lockstep run's rows: env e is episode env_offset + e."""
        self._lockstep_rows = torch.arange(self.args.env_offset, self.args.env_offset + self.n, dtype=torch.int32,
                                           device=self.device)

    def _episode_rows(self):
        """(episode, rollout_time_idx) of the rows at this point of the step, as set_rows of the
        Perturber and the Actuator takes them.  Lockstep: env e is episode env_offset + e and every
        row is at the host's rollout_time_idx (an int); streaming: the stream's slot -> episode map
        and each slot's own rollout_time_idx, read from the schedule on the device."""
        if self.args.num_episodes is not None and getattr(self, "stream", None) is not None:
            return self.stream.slot_episode, self.sched.view(torch.int32)[:, 1]
        return self._lockstep_rows, int(self.rollout_time_idx)

    def _perturb_rows(self):
        """The Perturber with the rows' (episode, draw) of the observation being made (_episode_rows)."""
        pt = self._perturb
        pt.set_rows(*self._episode_rows())
        return pt

    def policy_rgb(self, cam):
        """The 8-bit frame of camera `cam` the policy reads: info["rgb_images"][cam], or with --perturb
        the perturbed scratch frame (info["rgb_images"] itself stays clean)."""
        rgb = self.info["rgb_images"][cam]
        if getattr(self, "_perturb", None) is None or not self.perturb_spec.touches_images:
            return rgb
        return self._perturb_rows().frame(cam, rgb)

    # -- command routing (MotionManager / ArmManager) ------------------------------------------
    def _reset_motion(self):
        """ArmManager.reset (:75-86): arm / gripper command = the initial pose, IK target = its FK."""
        env, dev = self.env, self.device
        self.q_cmd = torch.tensor(np.tile(env.init_qpos[:6], (self.n, 1)), dtype=torch.float64, device=dev)
        self.grip_cmd = torch.zeros((self.n, 1), dtype=torch.float64, device=dev)
        self._placement = torch.tensor(env.arrays["arm_placement"], dtype=torch.float64, device=dev).contiguous()
        self._glo, self._ghi = float(env.action_low[6]), float(env.action_high[6])
        self._tgt_R = torch.empty((self.n, 9), dtype=torch.float64, device=dev)
        self._tgt_p = torch.empty((self.n, 3), dtype=torch.float64, device=dev)
        from .. import _native as N

        N.call("rmbx_arm_fk", N.ptr(self._placement), N.ptr(self.q_cmd), N.ptr(self._tgt_R), N.ptr(self._tgt_p),
               self.n, N.stream_ptr())

    def set_command_data(self):
        """RolloutBase.set_command_data (:496-509): the policy action routed key by key through
        MotionManager / ArmManager (joint / relative joint / gripper / eef pose / relative eef
        pose commands, rmbx_motion_command), with is_skip = rollout_time_idx % skip != 0.
        --actuation: the command that arrives at this step, under the mask of the rows it arrives for."""
        action, is_skip, mask = self._executed_action(self.rollout_time_idx, None)
        K.motion_command(self._placement, action, self._action_codes, is_skip, self._glo, self._ghi,
                         self.q_cmd, self.grip_cmd, self._tgt_R, self._tgt_p, mask=mask)

    # -- actuation perturbation (--actuation) ------------------------------------------------------
    def _actuation_begin(self):
        """The Actuator of this run, and its one printed line."""
        self._actuation = ACT.Actuator(self.actuation_spec, self.args.seed, self.n, self.action_dim, self.args.skip,
                                       self.action_stats(), self.device)
        self._lockstep_rows_begin()
        print(f"[{self.__class__.__name__}] Actuation: {self.actuation_spec}", flush=True)

    # -- dynamics randomisation (--dynamics) ---------------------------------------------------------
    def _dynamics_begin(self):
        """The Dynamics of this run (made once: it binds its scale rows to the engine), the draw of
        the lockstep rows' episodes -- before env.reset runs its forward pass -- and its one printed
        line."""
        from ..envs.ur5e_base import ARM_JOINTS

        if self._dynamics is None:
            eng = self.env.engine
            self._dynamics = DYN.Dynamics(self.dynamics_spec, self.args.seed, eng,
                                          DYN.object_bodies(eng.arrays, ARM_JOINTS[0]), self.device)
        self._lockstep_rows_begin()
        self._dynamics.draw(self._lockstep_rows)
        print(f"[{self.__class__.__name__}] Dynamics: {self.dynamics_spec}", flush=True)

    # -- camera jitter (--camera_jitter) --------------------------------------------------------------
    def _camera_jitter_begin(self):
        """The CameraJitter of this run (made once: it binds its rows to the env's renderer), the draw
        of the lockstep rows' episodes -- before env.reset renders the first observation -- and its one
        printed line."""
        if self._camera_jitter is None:
            self._camera_jitter = CJ.CameraJitter(self.camera_jitter_spec, self.args.seed, self.env.renderer, self.n,
                                                  self.device)
        self._lockstep_rows_begin()
        self._camera_jitter.draw(self._lockstep_rows)
        print(f"[{self.__class__.__name__}] Camera jitter: {self.camera_jitter_spec}", flush=True)

    def action_stats(self):
        """The statistics denormalize_data turns the policy's output into the action with."""
        return self.model_meta_info["action"]

    def _executed_action(self, r, mask):
        """(action, is_skip, mask) rmbx_motion_command gets at the host's rollout step r for the rows of
        `mask` (None: all): the policy action itself, or with --actuation the command that arrives at
        this step (rmbx_action_perturb), the is_skip of the step it was made for and the rows it
        arrives for."""
        act = getattr(self, "_actuation", None)
        if act is None:
            return self.policy_action, r % self.args.skip != 0, mask
        act.set_rows(*self._episode_rows())
        action, arrived = act(self.policy_action, mask_in=mask)
        return action, act.is_skip(r), arrived

    def env_action(self):
        return torch.cat([self.q_cmd, self.grip_cmd], dim=1)

    def _set_reach_target(self, pos_z):
        """OperationMujocoUR5eCable.get_target_se3 (:8-11): cable_end xy, fixed z, R=diag(-1,1,-1)."""
        end = self.env.get_body_pose("cable_end")[:, :3].clone()
        end[:, 2] = pos_z
        self._tgt_p.copy_(end)
        R = torch.tensor([-1.0, 0, 0, 0, 1.0, 0, 0, 0, -1.0], dtype=torch.float64, device=self.device)
        self._tgt_R.copy_(R.expand(self.n, 9))

    def _ik_step(self):
        from .. import _native as N

        N.call("rmbx_arm_ik", N.ptr(self._placement), N.ptr(self.q_cmd), N.ptr(self._tgt_R), N.ptr(self._tgt_p),
               None, self.n, 1, N.stream_ptr())

    # -- episode --------------------------------------------------------------------------------
    def reset(self):
        self._reset_motion()
        g0, wl = self.args.env_offset, self.args.world_idx_list
        world = np.array([wl[(g0 + e) % len(wl)] for e in range(self.n)])
        self.env.world_random_scale = self.args.world_random_scale
        self.world_idx = self.env.modify_world(world_idx=world)
        if getattr(self, "dynamics_spec", None) is not None:
            self._dynamics_begin()
        if getattr(self, "camera_jitter_spec", None) is not None:
            self._camera_jitter_begin()
        self.obs, self.info = self.env.reset(seed=self.args.seed)
        self._bind_state_stats()
        dev = self.device
        self.sched = K.sched_alloc(self.n, dev)
        K.sched_reset(self.sched, self.env.get_time())
        # device-side step mask: an env stops stepping at its RolloutPhase -> EndRolloutPhase
        # transition (rmbx_sched_active), freezing the state its results were recorded from
        self._step_mask = torch.ones(self.n, dtype=torch.uint8, device=dev)
        self._pre = torch.tensor(self.pre_durations, dtype=torch.float64, device=dev)
        # host mirror of the (env-independent) pre-rollout clock
        self.phase_idx = 0
        self.host_time = 0.0
        self.phase_start = 0.0
        self.rollout_time_idx = 0
        self.policy_action = torch.zeros((self.n, self.action_dim), dtype=torch.float64, device=dev)
        self.reset_variables()
        self._perturb = None
        if getattr(self, "perturb_spec", None) is not None:
            self._perturb_begin()
        self._actuation = None
        if getattr(self, "actuation_spec", None) is not None:
            self._actuation_begin()
        if getattr(self.args, "trace_dir", None) and self.args.num_episodes is None:
            self._trace_begin()
        if getattr(self.args, "episode_metrics", False) and self.args.num_episodes is None:
            self._metrics_begin()

    # -- per-episode metrics (--episode_metrics) --------------------------------------------------
    def _metrics_begin(self):
        """Allocate the device metrics table of this run.  Lockstep: env e is episode env_offset + e;
        streaming: one row per episode of the queue, addressed through the stream's slot -> episode
        map."""
        a, env = self.args, self.env
        streaming = a.num_episodes is not None
        self._metrics = K.EpisodeMetrics(
            self.sched, env.engine, len(self.pre_durations), int(a.num_episodes) if streaming else self.n,
            episode_base=int(a.episode_offset) if streaming else int(a.env_offset),
            slot_episode=self.stream.slot_episode if streaming else None, bad_resets=env.bad_resets,
            arm_qadr=env._arm_qadr.tolist(), arm_dof=env._arm_dadr.tolist())

    def _metrics_finish(self, world_idx):
        """Read the table (the one device read) and, under --num_gpus, all-gather the ranks' rows into
        global episode order: self.episode_metrics (_native.METRICS_DTYPE).  Every rank calls it."""
        table, widx = self._metrics.table(), np.asarray(world_idx, np.int64)
        rank, world = self._dist_world()
        if world > 1:
            import torch.distributed as dist

            from ..distributed import gather_table

            dev = self.device if dist.get_backend() == "nccl" else "cpu"
            table, widx = EM.columns_to_table(gather_table(EM.table_to_columns(table, widx), dev))
        self.episode_metrics, self._metrics_world = table, widx

    def _append_metrics_result(self):
        """result["metrics"]: per-episode lists parallel to result["success"] (which a second run of
        the same object extends, so these are extended too)."""
        new = EM.metrics_result(self.episode_metrics, self._step_seconds())
        cur = self.result.setdefault("metrics", {k: [] for k in new})
        for k, v in new.items():
            cur[k].extend(v)

    def _step_seconds(self):
        return self.env.frame_skip * self.env.sim_timestep

    def _print_metrics(self, success):
        for line in EM.summary_lines(EM.summarize(self.episode_metrics, success, self._metrics_world,
                                                  self._step_seconds())):
            print(line, flush=True)

    # -- episode trace (--trace_dir) -------------------------------------------------------------
    def _trace_begin(self):
        """Allocate the device trace of this run and open its directory.  Lockstep: env e is episode
        env_offset + e; streaming: the slot -> episode map of the stream."""
        from .. import kernels as K

        a, env, eng = self.args, self.env, self.env.engine
        old = getattr(self, "_trace", None)
        if old is not None:
            old.abort()
        streaming = a.num_episodes is not None
        base = int(a.episode_offset) if streaming else int(a.env_offset)
        count = int(a.num_episodes) if streaming else self.n
        chosen = parse_episodes(a.trace_episodes)
        mask = select_mask(chosen, base, count)
        select = None if mask is None else torch.tensor(mask, dtype=torch.uint8, device=self.device)
        trace = K.EpisodeTrace(self.sched, eng, count, len(self.pre_durations), episode_base=base,
                               slot_episode=self.stream.slot_episode if streaming else None, select=select,
                               stride=a.trace_stride, bad_resets=env.bad_resets if streaming else None)
        rank, world = self._dist_world()
        directory = os.path.join(a.trace_dir, f"rank{rank}") if world > 1 else a.trace_dir
        scale = a.world_random_scale
        header = {
            "policy": self.policy_name, "env": env.demo_name, "model_name": env.model_name,
            "image_size": [int(env.renderer.height), int(env.renderer.width)], "camera_names": list(env.camera_names),
            "seed": int(a.seed), "world_idx_list": [int(w) for w in a.world_idx_list],
            "world_random_scale": None if scale is None else [float(x) for x in np.asarray(scale).reshape(-1)],
            "skip": int(a.skip), "stride": int(a.trace_stride), "shadows": str(getattr(a, "shadows", "off")),
            "offsamples": str(getattr(a, "offsamples", "1")), "dims": trace.dims, "streaming": streaming, "episode_base": base,
            "num_episodes": count, "num_slots": self.n, "trace_episodes": "all" if chosen is None else chosen,
            "max_duration": float(a.max_duration), "rank": rank, "world_size": world,
        }
        if hasattr(a, "sampler_noise"):  # the diffusion policies: which noise a re-run must ask for
            header["sampler_noise"] = str(a.sampler_noise)
        if getattr(self, "perturb_spec", None) is not None:  # what Replay --as_seen applies
            header["perturb"] = self.perturb_spec.as_dict()
        if getattr(self, "actuation_spec", None) is not None:  # how the recorded ctrl came about
            header["actuation"] = self.actuation_spec.as_dict()
        if getattr(self, "dynamics_spec", None) is not None:  # the world each recorded episode ran in
            header["dynamics"] = self.dynamics_spec.as_dict()
        if getattr(self, "camera_jitter_spec", None) is not None:  # what Replay binds before it renders
            header["camera_jitter"] = self.camera_jitter_spec.as_dict()
        self._trace = TraceWriter(directory, header, trace)
        # the size the run can reach: an episode ends by max_duration + the post-success second
        dt = env.frame_skip * env.sim_timestep
        steps = self._phase_entry_steps()[-1] + int(np.ceil((a.max_duration + 1.0) / dt)) + 1
        if a.max_steps:
            steps = min(steps, int(a.max_steps))
        rows = steps // trace.stride + 1
        traced = count if mask is None else int(mask.sum())
        rb = row_bytes(trace.dims)
        print(f"[{self.__class__.__name__}] Episode trace: {directory}: {rb} bytes per row x up to {rows} rows per "
              f"episode (stride {trace.stride}) x {traced} episodes = up to {rb * rows * traced / 2**20:.1f} MiB",
              flush=True)

    def _trace_finish(self, records):
        tr = getattr(self, "_trace", None)
        if tr is not None:
            self._trace = None
            tr.finish(records)
            self.last_trace = tr  # its counters (rows, flush times) outlive the run

    def _lockstep_records(self, v):
        """The records of a lockstep run in the form a streaming run keeps them (_native.EPISODE_DTYPE)."""
        from .. import _native as N

        rec = np.zeros(self.n, dtype=N.EPISODE_DTYPE)
        rec["episode"] = self.args.env_offset + np.arange(self.n)
        rec["slot"] = np.arange(self.n)
        rec["world_idx"] = np.asarray(self.world_idx)
        rec["rollout_time_idx"], rec["success"] = v["rollout_time_idx"], v["success"]
        rec["bad_state"] = (self.env.bad_resets.cpu().numpy() > 0).astype(np.uint8)
        rec["reward"], rec["duration"] = v["result_reward"], v["duration"]
        return rec

    def _pre_update(self):
        n_pre = len(self.pre_durations)
        if self.phase_idx == 0:
            return
        if self.phase_idx < n_pre:
            ph = self.pre_phases[self.phase_idx - 1]
            if ph.kind == "reach":
                self._ik_step()
            elif ph.kind == "grasp":
                # GraspPhaseBase.pre_update (:66-69): set_target_close / set_target_open
                # (action_space high / low, :78-104) or a fixed value
                g = self._ghi if ph.grip is None else (self._glo if ph.grip == "low" else float(ph.grip))
                self.grip_cmd.fill_(g)
        elif self.phase_idx == n_pre:
            if self.rollout_time_idx % self.args.skip == 0:
                self._timed_infer()
            self.set_command_data()

    def _timed_infer(self):
        """infer_policy timed like the reference's figure (RolloutAct.py:74-76 includes the .cpu()
        sync): device events around the call on the current stream, read in finish() so the
        loop never waits on the device; wall clock on a CPU device."""
        if self.device.type == "cuda":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self._mark("policy")
            e0.record()
            self.infer_policy()
            e1.record()
            self._mark("glue")
            self._infer_events.append((e0, e1))
        else:
            t0 = time.time()
            self.infer_policy()
            self.inference_duration_list.append(time.time() - t0)

    def _collect_inference_durations(self):
        if self._infer_events:
            self._infer_events[-1][1].synchronize()
            self.inference_duration_list.extend(a.elapsed_time(b) / 1e3 for a, b in self._infer_events)
            self._infer_events = []

    def _host_transition(self):
        """Host mirror of the pre-rollout phase clock (PhaseBase.get_elapsed_duration)."""
        n_pre = len(self.pre_durations)
        if self.phase_idx < n_pre:
            if self.host_time - self.phase_start > self.pre_durations[self.phase_idx]:
                self.phase_idx += 1
                self.phase_start = self.host_time
                if self.phase_idx < n_pre:
                    ph = self.pre_phases[self.phase_idx - 1]
                    if ph.kind == "reach":
                        if ph.target is not None:
                            R, p = ph.target(self)
                            self._tgt_R.copy_(R)
                            self._tgt_p.copy_(p)
                        else:
                            self._set_reach_target(ph.pos_z)
                else:
                    self.rollout_time_idx = 0
        elif self.phase_idx == n_pre:
            self.rollout_time_idx += 1

    def step_once(self):
        self._mark("glue")
        self._pre_update()
        active = self._active if self._active is not None else self._step_mask
        self.obs, self.reward, _, _, self.info = self.env.step(self.env_action(), active=active)
        for _ in range(self.env.frame_skip):
            self.host_time += self.env.sim_timestep
        if getattr(self, "_metrics", None) is not None:
            self._metrics.step(active, self.reward)
        K.sched_update(self.sched, self.env.get_time(), self.reward, self._pre, self.args.max_duration)
        if getattr(self, "_trace", None) is not None:
            self._trace.step(active, self.reward)
        K.sched_active(self.sched, len(self.pre_durations), out=self._step_mask)
        self._host_transition()

    # -- streaming mode (--num_episodes): n slots work through a queue of M episodes -----------
    # How many infer_policy() calls apart the policy reads a new observation for its action buffer
    # (1: every call; the policies with an action buffer: its length)
    infer_period_calls = 1

    @property
    def stream_period(self):
        """P = skip x infer_period_calls env-steps: finished slots are recycled only at the end of
        global steps g with (g + 1) % P == 0, so every episode starts on a multiple of P and shares
        the host's skip / inference phase."""
        return int(self.args.skip) * int(self.infer_period_calls)

    def reset_policy_state(self, mask):
        """Forget the episode of the slots of `mask` (u8 [n], device; no host sync): recurrent
        state, ensemble ring, action buffer, observation history.  Defined by the policy."""
        raise NotImplementedError(f"{self.__class__.__name__} does not define reset_policy_state")

    def _fill_first_obs(self, hist, new, dim):
        """Observation histories of the policies that keep n_obs_steps of them: the rows whose
        episode has just begun (reset_policy_state) hold the new observation in every entry of
        `dim`, as the reference's first call of an episode does; the other rows keep `hist`."""
        first = getattr(self, "_first_obs", None)
        if first is None:
            return hist
        return torch.where(first.view((self.n,) + (1,) * (hist.dim() - 1)), new.unsqueeze(dim), hist)

    def _reset_obs_history(self, mask):
        m = mask.bool()
        first = getattr(self, "_first_obs", None)
        self._first_obs = m if first is None else (first | m)

    def _phase_entry_steps(self):
        """N_k for k = 1 .. n_pre: the env-step count an episode has spent when it enters phase k
        (k = n_pre: RolloutPhase), from the host mirror of the phase clock -- the same for every
        episode, since the pre-rollout phases are clock-driven and every clock starts at 0."""
        t, start, out = 0.0, 0.0, []
        steps = 0
        for dur in self.pre_durations:
            while True:
                for _ in range(self.env.frame_skip):
                    t += self.env.sim_timestep
                steps += 1
                if t - start > dur:
                    break
            start = t
            out.append(steps)
        return out

    def reset_streaming(self):
        """Lockstep reset of the n slots as episodes episode_offset .. + n - 1, plus the episode
        queue: the world table of this process's M episodes and the recycle buffers."""
        a = self.args
        self.reset()
        env, eng = self.env, self.env.engine
        M, g0 = int(a.num_episodes), int(a.episode_offset)
        widx, wpos = env.world_table(g0 + np.arange(M), a.world_idx_list)
        self._episode_world = np.asarray(widx, dtype=np.int64)
        world_body, world_qadr = env.world_slot()
        motion0 = torch.cat([self.q_cmd[0], self._tgt_R[0], self._tgt_p[0]]).cpu().numpy()  # constant FK
        self.stream = K.EpisodeStream(
            self.sched, eng, self.q_cmd, self.grip_cmd, self._tgt_R, self._tgt_p, env.bad_resets, env.init_qpos,
            np.concatenate([env.init_qpos[:6], [0.0]])[: eng.nu], motion0, widx, wpos, episode_base=g0,
            world_body=world_body, world_qadr=world_qadr, final_qpos=getattr(self, "record_final_qpos", False))
        self.slot_episode = self.stream.slot_episode
        self.stream.phases()
        self._entry_steps = self._phase_entry_steps()
        self._grip_values = {}
        self._g = 0  # global env-step index
        self.episode_records = None
        if getattr(self.args, "trace_dir", None):
            self._trace_begin()
        if getattr(self.args, "episode_metrics", False):
            self._metrics_begin()

    def _reach_target(self, ph):
        """(R [n, 9], p [n, 3]) a reach phase would set now for every slot."""
        if ph.target is not None:
            return ph.target(self)
        end = self.env.get_body_pose("cable_end")[:, :3].clone()
        end[:, 2] = ph.pos_z
        R = torch.tensor([-1.0, 0, 0, 0, 1.0, 0, 0, 0, -1.0], dtype=torch.float64, device=self.device)
        return R.expand(self.n, 9), end

    def step_stream(self):
        """One env-step of every slot, each in its own phase (the order of step_once); recycles the
        finished slots when the step is aligned.  No host synchronisation."""
        from .. import _native as N

        st, n_pre, P, skip = self.stream, len(self.pre_durations), self.stream_period, self.args.skip
        g, N_pre = self._g, self._entry_steps[-1]
        self._mark("glue")
        # 1. pre-motion phases, each under the mask of the slots that are in it
        for k in range(1, n_pre):
            ph = self.pre_phases[k - 1]
            in_k = st.phase == k
            if ph.kind == "reach":
                N.call("rmbx_arm_ik", N.ptr(self._placement), N.ptr(self.q_cmd), N.ptr(self._tgt_R),
                       N.ptr(self._tgt_p), N.ptr(in_k.to(torch.uint8)), self.n, 1, N.stream_ptr())
            elif ph.kind == "grasp":
                gv = self._ghi if ph.grip is None else (self._glo if ph.grip == "low" else float(ph.grip))
                self.grip_cmd.copy_(torch.where(in_k[:, None], gv, self.grip_cmd))
        # 2. RolloutPhase: the host's global rollout index is every slot's, mod P
        hr = g - N_pre
        if hr >= 0:
            in_rollout = st.phase == n_pre
            if hr % P == 0:
                self.reset_policy_state((in_rollout & (st.entered != 0)).to(torch.uint8))
            self.rollout_time_idx = hr
            if hr % skip == 0:
                self._timed_infer()
            action, is_skip, mask = self._executed_action(hr, in_rollout.to(torch.uint8))
            K.motion_command(self._placement, action, self._action_codes, is_skip, self._glo, self._ghi, self.q_cmd,
                             self.grip_cmd, self._tgt_R, self._tgt_p, mask=mask)
        # 3. step + schedule
        self.obs, self.reward, _, _, self.info = self.env.step(self.env_action(), active=self._step_mask)
        if getattr(self, "_metrics", None) is not None:
            self._metrics.step(self._step_mask, self.reward)
        K.sched_update(self.sched, self.env.get_time(), self.reward, self._pre, self.args.max_duration)
        st.close_bad(n_pre)
        if getattr(self, "_trace", None) is not None:
            self._trace.step(self._step_mask, self.reward)
        K.sched_active(self.sched, n_pre, out=self._step_mask)
        # 4. recycle on aligned steps, then the phase report
        if (g + 1) % P == 0:
            self._mark("recycle")
            st.recycle()
            K.sched_active(self.sched, n_pre, out=self._step_mask)
            if getattr(self, "_dynamics", None) is not None:  # the new episodes' worlds, before their forward pass
                self._dynamics.draw(st.slot_episode, active=st.recycled)
            if getattr(self, "_camera_jitter", None) is not None:  # the new episodes' cameras, before their first render
                self._camera_jitter.draw(st.slot_episode, active=st.recycled)
            self.env.refresh(active=st.recycled)
            self.obs, self.reward, self.info = self.env._get_obs(), self.env.reward, self.env._get_info()
            self._mark("glue")
        st.phases()
        # reach targets of the slots that entered a reach phase with this step (a phase is entered
        # N_k steps after an aligned episode start, so only on steps of one residue mod P)
        for k in range(1, n_pre):
            ph = self.pre_phases[k - 1]
            if ph.kind == "reach" and g + 1 >= self._entry_steps[k - 1] and (g + 1 - self._entry_steps[k - 1]) % P == 0:
                m = ((st.phase == k) & (st.entered != 0))[:, None]
                R, p = self._reach_target(ph)
                self._tgt_R.copy_(torch.where(m, R, self._tgt_R))
                self._tgt_p.copy_(torch.where(m, p, self._tgt_p))
        self._g = g + 1
        self.rollout_time_idx = max(self._g - N_pre, 0)

    def run_streaming(self, max_steps=None):
        self.reset_streaming()
        max_steps = max_steps or self.args.max_steps or 10**9
        M, steps = int(self.args.num_episodes), 0
        while steps < max_steps:
            self.step_stream()
            steps += 1
            # the only host read of the loop: the two device counters, every 16 steps
            if steps % 16 == 0 and int(self.stream.counters.cpu()[1]) >= M:
                break
        self.finish()
        return steps

    def run(self, max_steps=None):
        if self.args.num_episodes is not None:
            return self.run_streaming(max_steps)
        self.reset()
        max_steps = max_steps or self.args.max_steps or 10**9
        steps = 0
        while steps < max_steps:
            self.step_once()
            steps += 1
            # finished envs are frozen on the device (step mask); the host only polls for the end
            if self.phase_idx >= len(self.pre_durations) and steps % 16 == 0:
                if K.sched_view(self.sched)["done"].all():
                    break
        self.finish()
        return steps

    def _dist_world(self):
        """(rank, world) of the torch.distributed group this rollout is a shard of (bin/Rollout.py
        --num_gpus), else (0, 1)."""
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def finish(self):
        """RolloutPhase / EndRolloutPhase result bookkeeping (RolloutBase.py:96-110, 417-422) for
        every env.  Under --num_gpus the per-env records of all shards are all-gathered (one RCCL
        all_gather, distributed.py) and rank 0 prints and writes them in global env order."""
        if getattr(self.args, "num_episodes", None) is not None:
            return self._finish_streaming()
        v = K.sched_view(self.sched)
        succ, rew, dur = v["success"].astype(bool), v["result_reward"].astype(np.float64), v["duration"]
        if getattr(self, "_trace", None) is not None:
            self._trace_finish(self._lockstep_records(v))
        rank, world = self._dist_world()
        if world > 1:
            import torch.distributed as dist

            from ..distributed import gather_results, pack_results

            dev = self.device if dist.get_backend() == "nccl" else "cpu"
            g = gather_results(pack_results(succ, rew, dur, v["rollout_time_idx"]), dev)
            succ, rew, dur = g[:, 0] != 0, g[:, 1], g[:, 2]
        metrics = getattr(self, "_metrics", None) is not None
        if metrics:
            self._metrics_finish(self.world_idx)
        if rank == 0:
            for e in range(len(succ)):
                print(f"Rollout result: {'success' if succ[e] else 'failure'}", flush=True)
                self.result["success"].append(bool(succ[e]))
                self.result["reward"].append(float(rew[e]))
                self.result["duration"].append(float(dur[e]))
            if metrics:
                self._append_metrics_result()
            if getattr(self, "perturb_spec", None) is not None:
                self.result["perturb"] = self.perturb_spec.as_dict()
            if getattr(self, "actuation_spec", None) is not None:
                self.result["actuation"] = self.actuation_spec.as_dict()
            if getattr(self, "dynamics_spec", None) is not None:
                self.result["dynamics"] = self.dynamics_spec.as_dict()
            if getattr(self, "camera_jitter_spec", None) is not None:
                self.result["camera_jitter"] = self.camera_jitter_spec.as_dict()
        if self.args.save_last_image:
            self.save_rgb_images(v)
        if rank == 0 and self.args.result_filename is not None:
            print(f"[{self.__class__.__name__}] Save the rollout results: {self.args.result_filename}")
            with open(self.args.result_filename, "w") as f:
                yaml.dump(self.result, f)
        if rank == 0:
            self.print_statistics()
            if metrics:
                self._print_metrics(succ)

    def _finish_streaming(self):
        """finish() of a streaming run: one record per episode, in episode order.  An episode the
        run was cut off before (--max_steps) is reported as a failure of duration 0 (its record's
        `episode` is -1).  Under --num_gpus the ranks' contiguous episode shards are all-gathered
        and rank 0 reports them in global episode order."""
        rec = self.stream.records()
        self.episode_records = rec
        if getattr(self, "_trace", None) is not None:
            self._trace_finish(rec)
        self.bad_state_episodes = int(rec["bad_state"].sum())
        succ, rew, dur = rec["success"].astype(bool), rec["reward"].copy(), rec["duration"].copy()
        nbad = self.bad_state_episodes
        rank, world = self._dist_world()
        if world > 1:
            import torch.distributed as dist

            from ..distributed import gather_results, pack_results

            dev = self.device if dist.get_backend() == "nccl" else "cpu"
            g = gather_results(pack_results(succ, rew, dur, rec["rollout_time_idx"]), dev)
            h = gather_results(pack_results(rec["episode"], rec["slot"], rec["world_idx"], rec["bad_state"]), dev)
            succ, rew, dur = g[:, 0] != 0, g[:, 1], g[:, 2]
            nbad = int(h[:, 3].sum())
            # every rank's episode_records: all episodes, in global episode order
            from .. import _native as N

            rec = np.zeros(len(g), dtype=N.EPISODE_DTYPE)
            rec["success"], rec["reward"], rec["duration"], rec["rollout_time_idx"] = succ, rew, dur, g[:, 3]
            rec["episode"], rec["slot"], rec["world_idx"], rec["bad_state"] = h[:, 0], h[:, 1], h[:, 2], h[:, 3]
            self.episode_records = rec
        metrics = getattr(self, "_metrics", None) is not None
        if metrics:
            self._metrics_finish(self._episode_world)
        if rank == 0:
            for e in range(len(succ)):
                print(f"Rollout result: {'success' if succ[e] else 'failure'}", flush=True)
                self.result["success"].append(bool(succ[e]))
                self.result["reward"].append(float(rew[e]))
                self.result["duration"].append(float(dur[e]))
            if metrics:
                self._append_metrics_result()
            if getattr(self, "perturb_spec", None) is not None:
                self.result["perturb"] = self.perturb_spec.as_dict()
            if getattr(self, "actuation_spec", None) is not None:
                self.result["actuation"] = self.actuation_spec.as_dict()
            if getattr(self, "dynamics_spec", None) is not None:
                self.result["dynamics"] = self.dynamics_spec.as_dict()
            if getattr(self, "camera_jitter_spec", None) is not None:
                self.result["camera_jitter"] = self.camera_jitter_spec.as_dict()
            if self.args.result_filename is not None:
                print(f"[{self.__class__.__name__}] Save the rollout results: {self.args.result_filename}")
                with open(self.args.result_filename, "w") as f:
                    yaml.dump(self.result, f)
            self.bad_state_episodes = nbad
            self.print_statistics()
            if metrics:
                self._print_metrics(succ)

    def save_rgb_images(self, v=None):
        """RolloutBase.save_rgb_image (:541-561) for every env: the last frame of all cameras side
        by side (cv2.hconcat of info["rgb_images"]), named
        Rollout<Policy>_<Env>_world<idx>_<success|failure>_<datetime>.png in --output_image_dir.
        Each env is frozen at its episode's end, so its frame is the transition step's."""
        from .image_io import write_png

        if v is None:
            v = K.sched_view(self.sched)
        # cv2.hconcat(list(self.info["rgb_images"].values())): the envs are frozen at their last
        # step, whose info this is
        image = torch.cat([self.info["rgb_images"][cam] for cam in self.env.camera_names], dim=2).cpu().numpy()
        demo_name = self.env.demo_name
        os.makedirs(self.args.output_image_dir, exist_ok=True)
        for e in range(self.n):
            success_str = "success" if v["success"][e] else "failure"
            path = os.path.abspath(os.path.join(
                self.args.output_image_dir,
                f"Rollout{self.policy_name}_{demo_name}_world{int(self.world_idx[e]):0>1}_{success_str}_"
                f"{self.datetime_now:%Y%m%d_%H%M%S}_env{self.args.env_offset + e}.png"))
            print(f"[{self.__class__.__name__}] Save the observation image of the last frame: {path}")
            write_png(path, image[e])

    def print_statistics(self):
        self._collect_inference_durations()
        print(f"[{self.__class__.__name__}] Statistics on policy inference")
        if self.inference_duration_list:
            a = np.array(self.inference_duration_list)
            print(f"  - Inference duration [s] | mean: {a.mean():.2e}, std: {a.std():.2e} min: {a.min():.2e}, max: {a.max():.2e}")
            print(f"  - Inference duration per env [us] | mean: {1e6 * a.mean() / self.n:.2f}")
        if getattr(self.args, "num_episodes", None) is not None:
            print(f"  - Episodes closed by a bad-state reset | {getattr(self, 'bad_state_episodes', 0)}")
        if torch.cuda.is_available():
            print(f"  - GPU memory usage [GB] | {torch.cuda.max_memory_reserved() / 1024**3:.3f}")
