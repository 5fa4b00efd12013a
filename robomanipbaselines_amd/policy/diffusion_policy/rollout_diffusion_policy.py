"""Batched RolloutDiffusionPolicy: policy/diffusion_policy/RolloutDiffusionPolicy.py of the
reference for n_env envs.

* get_state (:89-105): normalised state, n_obs_steps history -> [n, To, S].
* get_images (:107-138): renderer u8 frames -> rmbx_resize_crop_u8 (cv2.resize to image_size,
  ToDtype(scale), * 2 - 1, and the obs encoder's eval centre crop to image_crop_size) ->
  n_obs_steps history [n, ncam, To, 3, ch, cw].
* infer_policy (:66-87): when the action buffer is empty, predict_action (obs encoder + 100-step
  DDPM loop, HIP-graph captured) -> n_action_steps actions; each call pops one and
  denormalises it (rmbx_act_ensemble, no-ensemble mode, bit-exact f64).
* --sampler_noise episode (opt-in): the sampler's noise from the Philox stream of (seed, global
  episode index, inference count of the episode) instead of torch.randn draws for the batch, so an
  episode does not depend on the layout it runs in.
Training-side defaults (TrainDiffusionPolicy.py:26-84): limits normalisation to [-1, 1],
horizon 16, n_obs_steps 2, n_action_steps 8, image_size 320x240, crop 288x216.
"""

import numpy as np
import os

import torch

from ... import kernels as K
from ...common.rollout_base import BatchedRolloutBase
from ..diffusion.checkpoint import load_dp_checkpoint
from .dp_model import DiffusionPolicyModel


def _limits_meta(meta, out_min=-1.0, out_max=1.0):
    for key in ("state", "action"):
        meta[key]["norm_config"] = {"type": "limits", "out_min": out_min, "out_max": out_max}


class RolloutDiffusionPolicy(BatchedRolloutBase):
    policy_name = "DiffusionPolicy"

    def set_additional_args(self, parser):
        parser.add_argument("--no_graph", action="store_true", help="run the denoising loop eagerly")
        parser.add_argument("--sampler_noise", choices=["batch", "episode"], default="batch",
                            help="where the sampler's initial trajectory and variance noise come from. batch "
                                 "(default): torch.randn draws for the whole batch, as the reference draws them; a "
                                 "row's noise depends on the batch layout. episode: a Philox stream keyed by "
                                 "(--seed, global episode index, inference count of the episode), the same in every "
                                 "layout (slot count, slot, --env_offset / --episode_offset, --num_gpus)")

    def setup_model_meta_info(self):
        super().setup_model_meta_info()
        meta = self.model_meta_info
        if meta["data"].get("name") == "synthetic":
            _limits_meta(meta)
            meta["data"].update({"horizon": 16, "n_obs_steps": 2, "n_action_steps": 8,
                                 "image_size": [320, 240], "image_crop_size": [288, 216]})

    def setup_policy(self):
        meta = self.model_meta_info
        d = meta["data"]
        self.n_obs_steps, self.n_action_steps = int(d["n_obs_steps"]), int(d["n_action_steps"])
        self.image_size, self.crop_size = list(d["image_size"]), list(d["image_crop_size"])
        self.policy = DiffusionPolicyModel(
            len(meta["state"]["example"]), len(meta["action"]["example"]), len(meta["image"]["camera_names"]),
            horizon=int(d["horizon"]), n_obs_steps=self.n_obs_steps, n_action_steps=self.n_action_steps,
            crop_hw=(self.crop_size[1], self.crop_size[0]), num_inference_steps=100)
        if self.args.checkpoint:
            # the reference's DiffusionUnetHybridImagePolicy checkpoint, strictly (RolloutBase.py:376-385)
            load_dp_checkpoint(self.policy, self.args.checkpoint, self.camera_names)
        self.policy_dtype = torch.bfloat16 if self.args.precision == "bf16" else torch.float32
        # (the UNet's convs are GEMMs in both precisions, so MIOpen serves the image encoder only:
        # Find picks its solvers once per shape, outside the captured denoising loop).  fp32 is the
        # parity mode: deterministic MIOpen solvers only (no atomic split-K), so a seed reproduces
        # its episodes bit for bit, as the reference's TrainDiffusionPolicy/rollout setup intends
        torch.backends.cudnn.benchmark = True
        torch.backends.cudnn.deterministic = (self.policy_dtype == torch.float32
                                              and os.environ.get("RMBX_DP_DETERMINISTIC", "1") != "0")
        self.policy = self.policy.eval().requires_grad_(False).to(device=self.device, dtype=self.policy_dtype)
        self.policy.obs_nets = self.policy.obs_nets.to(memory_format=torch.channels_last)
        self._print_sampler_noise()

    def _print_sampler_noise(self):
        print(f"[{self.__class__.__name__}] Sampler noise: {getattr(self.args, 'sampler_noise', 'batch')}", flush=True)

    @property
    def infer_period_calls(self):
        return self.n_action_steps

    def reset_policy_state(self, mask):
        """--sampler_noise batch: the sampler draws its noise per call for all rows, so a streaming
        run's episodes are reproducible for a fixed slot count, not across slot counts.  episode:
        the rows of `mask` begin a new noise stream (their draw counter returns to 0), so an
        episode's noise is the same in every layout."""
        self.ens.reset(mask)
        self._reset_obs_history(mask)
        if getattr(self, "_draw", None) is not None:
            self._draw.masked_fill_(mask.bool(), 0)

    def reset_variables(self):
        self.ens = K.ActEnsembleState(self.n, self.n_action_steps, self.action_dim, self.model_meta_info["action"],
                                      self.device, temporal_ensemble=False)
        self.state_buf = None
        self.images_buf = None
        self._calls = 0
        self._first_obs = None
        # --sampler_noise episode: the draw counter of every row (sampler calls its episode has made)
        # and, for a lockstep run, the rows' global episode indices (a streaming run reads the
        # stream's slot -> episode map, which the device updates)
        self._draw = self._lockstep_episode = None
        if getattr(self.args, "sampler_noise", "batch") == "episode":
            self._draw = torch.zeros(self.n, dtype=torch.int32, device=self.device)
            self._lockstep_episode = torch.arange(self.args.env_offset, self.args.env_offset + self.n,
                                                  dtype=torch.int32, device=self.device)

    def _noise_source(self):
        """(seed, episode [n] i32, draw [n] i32) of the next sampler call, or None (--sampler_noise batch)."""
        if self._draw is None:
            return None
        streaming = self.args.num_episodes is not None
        episode = self.stream.slot_episode if streaming else self._lockstep_episode
        return int(self.args.seed) & (2**64 - 1), episode, self._draw

    def _predict(self, *obs):
        """predict_action of a push step; afterwards every row has made one more sampler call."""
        chunk = self.policy.predict_action(*obs, use_graph=not self.args.no_graph,
                                           noise_source=self._noise_source()).float().contiguous()
        if self._draw is not None:
            self._draw += 1
        return chunk

    def get_state(self):
        s = super().get_state()
        if self.state_buf is None:
            self.state_buf = s[:, None].repeat(1, self.n_obs_steps, 1)
        else:
            self.state_buf = self._fill_first_obs(torch.cat([self.state_buf[:, 1:], s[:, None]], dim=1), s, 1)
        return self.state_buf

    def get_images(self, dtype):
        """RolloutDiffusionPolicy.get_images (:111-143): info["rgb_images"][camera] of the last
        env-step, resized / scaled / cropped on the device."""
        rw, rh = self.image_size
        cw, ch = self.crop_size
        crop = ((rh - ch) // 2, (rw - cw) // 2, ch, cw)
        imgs = []
        for cam in self.camera_names:
            rgb = self.policy_rgb(cam)
            imgs.append(K.resize_crop_u8(rgb, (rw, rh), crop, a=2.0, b=-1.0, dtype=dtype))
        img = torch.stack(imgs, dim=1)  # [n, ncam, 3, ch, cw]
        if self.images_buf is None:
            self.images_buf = img[:, :, None].repeat(1, 1, self.n_obs_steps, 1, 1, 1)
        else:
            self.images_buf = self._fill_first_obs(torch.cat([self.images_buf[:, :, 1:], img[:, :, None]], dim=2),
                                                   img, 2)
        return self.images_buf

    @torch.no_grad()
    def infer_policy(self):
        push = self._calls % self.n_action_steps == 0
        chunk = None
        if push:
            state = self.get_state()
            images = self.get_images(self.policy_dtype)
            chunk = self._predict(state, images)
            self._first_obs = None
        p = torch.full((self.n,), int(push), dtype=torch.uint8, device=self.device)
        self.policy_action = self.ens(chunk, push=p)
        self._calls += 1
