"""Batched RolloutSarnn: policy/sarnn/RolloutSarnn.py of the reference for n_env envs.

* setup_policy (:18-37): SarnnPolicy(state_dim, ncam, **meta["policy"]["args"]) + the checkpoint.
* reset_variables (:54-64): lstm_state = None, i.e. per-env (h, c) = 0 on the device.
* get_images (:103-122): info["rgb_images"][camera] centre-cropped (crop_and_resize,
  common/utils/VisionUtils.py:5-35), cv2.resize to the image size, / 255 -> [n, ncam, 3, S, S].
* infer_policy (:66-79): the network on every policy step with the recurrent state carried;
  predicted_state -> f64 -> denormalize_data with the STATE statistics (rmbx_act_ensemble in its
  no-ensemble mode with a chunk of one: bit-exact f64).
* set_command_data (:124-126): the model has no action keys; the predicted state is routed as the
  command keys of the state keys.
Training-side defaults (TrainSarnn.py:54-124, TrainBase.py:347-353): state command_joint_pos,
limits normalisation to [0, 1], skip 6, crop 280x280, image 64x64, 5 attention points, LSTM 50.
"""

import numpy as np
import torch

from ... import kernels as K
from ...common.data_key import DataKey, action_key_codes
from ...common.rollout_base import BatchedRolloutBase
from .sarnn_model import SarnnModel


def crop_window(height, width, crop_size):
    """(y0, x0, ch, cw) of crop_and_resize's centre crop of a height x width frame; crop_size is
    (width, height) (VisionUtils.py:16-27)."""
    ch, cw = int(crop_size[1]), int(crop_size[0])
    return height // 2 - ch // 2, width // 2 - cw // 2, ch, cw


def _per_camera(sizes, ncam, what):
    """A flat (w, h) pair for every camera, or one pair per camera (TrainSarnn --image_size_list)."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    if len(sizes) == 1:
        sizes = np.repeat(sizes, ncam, axis=0)
    if len(sizes) != ncam:
        raise ValueError(f"{what} has {len(sizes)} entries for {ncam} cameras")
    return [(int(w), int(h)) for w, h in sizes]


class RolloutSarnn(BatchedRolloutBase):
    policy_name = "Sarnn"

    def setup_model_meta_info(self):
        synthetic = not self.args.checkpoint
        skip_given, skip_draw_given = self.args.skip is not None, self.args.skip_draw is not None
        if synthetic:
            if self.args.action_keys is not None:
                raise ValueError("Sarnn has no action keys: the predicted state is the command")
            if self.args.state_keys is None:
                self.args.state_keys = [DataKey.COMMAND_JOINT_POS]
        super().setup_model_meta_info()
        meta = self.model_meta_info
        if synthetic:
            meta["state"]["norm_config"] = {"type": "limits", "out_min": 0.0, "out_max": 1.0}
            meta["action"] = {"keys": [], "example": np.zeros(0)}
            meta["data"].update({"skip": 6, "image_crop_size_list": [280, 280], "image_size_list": [64, 64]})
            meta["policy"]["args"] = {"image_size_list": [64, 64], "num_attentions": 5, "lstm_hidden_dim": 50}
            if not skip_given:
                self.args.skip = 6
                if not skip_draw_given:
                    self.args.skip_draw = 6
        # RolloutSarnn.set_command_data (:124-126)
        self.action_keys = [DataKey.get_command_key(key) for key in self.state_keys]
        self._action_codes = action_key_codes(self.action_keys)
        self.action_dim = self.state_dim
        kd = sum(DataKey.get_dim(k, self.env) for k in self.action_keys)
        if kd != self.action_dim:
            raise ValueError(f"command keys {self.action_keys} have dimension {kd}, the state {self.state_dim}")

    def setup_policy(self):
        if self.args.precision != "fp32":
            raise ValueError("Sarnn runs in fp32 only: its spatial softmax has a temperature of 1e-4, which "
                             "amplifies the convolutions' rounding by 1e4 (--precision bf16 is not served)")
        meta = self.model_meta_info
        ncam = len(self.camera_names)
        self.crop_size_list = _per_camera(meta["data"]["image_crop_size_list"], ncam, "image_crop_size_list")
        self.image_size_list = _per_camera(meta["data"]["image_size_list"], ncam, "image_size_list")
        if len(set(self.image_size_list)) != 1:
            raise ValueError(f"image sizes {self.image_size_list}: the batched rollout stacks the cameras, so they "
                             "must share one size")
        self.policy = SarnnModel(self.state_dim, ncam, **meta["policy"]["args"])
        if self.policy.image_size_list != self.image_size_list:
            raise ValueError(f"policy image sizes {self.policy.image_size_list} differ from the data's "
                             f"{self.image_size_list}")
        if self.args.checkpoint:
            sd = torch.load(self.args.checkpoint, map_location="cpu", weights_only=True)
            self.policy.load_state_dict(sd)
        self.policy_dtype = torch.float32
        torch.backends.cudnn.allow_tf32 = False
        torch.backends.cuda.matmul.allow_tf32 = False
        self.policy = self.policy.eval().requires_grad_(False).to(device=self.device, dtype=torch.float32)

    def action_stats(self):
        return self.model_meta_info["state"]  # the predicted state is the command

    def reset_variables(self):
        hd = self.policy.lstm_hidden_dim
        self.h = torch.zeros((self.n, hd), dtype=torch.float32, device=self.device)
        self.c = torch.zeros((self.n, hd), dtype=torch.float32, device=self.device)
        self.ens = K.ActEnsembleState(self.n, 1, self.action_dim, self.model_meta_info["state"], self.device,
                                      temporal_ensemble=False)
        self._push = torch.ones(self.n, dtype=torch.uint8, device=self.device)
        self.attention = None
        self.predicted_state = None
        self._img = None

    def reset_lstm_state(self, mask):
        """lstm_state = None for the envs of `mask` (bool / u8 [n]) alone: their (h, c) rows are
        zeroed and their action buffer emptied, every other env's are untouched."""
        self.reset_policy_state(mask.to(device=self.device))

    def reset_policy_state(self, mask):
        m = mask.bool()  # masked fills: no host synchronisation
        self.h.masked_fill_(m[:, None], 0.0)
        self.c.masked_fill_(m[:, None], 0.0)
        self.ens.reset(m)

    def get_images(self, dtype=torch.float32):
        if dtype != torch.float32:
            raise ValueError("Sarnn images are f32")
        S = self.image_size_list[0][0]
        if self._img is None:
            self._img = torch.empty((self.n, len(self.camera_names), 3, S, S), dtype=torch.float32, device=self.device)
            self._img_cam = [torch.empty((self.n, 3, S, S), dtype=torch.float32, device=self.device)
                             for _ in self.camera_names]
        self._mark("render")  # the u8 frames are rendered on first access
        frames = [self.policy_rgb(cam) for cam in self.camera_names]
        self._mark("policy")
        for i, (rgb, crop_size) in enumerate(zip(frames, self.crop_size_list)):
            y0, x0, ch, cw = crop_window(rgb.shape[1], rgb.shape[2], crop_size)
            window = rgb[:, y0:y0 + ch, x0:x0 + cw].contiguous()
            if len(self.camera_names) == 1:
                K.resize_crop_u8(window, (S, S), a=1.0, b=0.0, dtype=torch.float32, out=self._img.view(self.n, 3, S, S))
            else:
                K.resize_crop_u8(window, (S, S), a=1.0, b=0.0, dtype=torch.float32, out=self._img_cam[i])
                self._img[:, i].copy_(self._img_cam[i])
        return self._img

    @torch.no_grad()
    def infer_policy(self):
        state = self.get_state()
        images = self.get_images()
        pred, self.attention = self.policy.step(state, images, self.h, self.c)
        self.predicted_state = pred
        self.policy_action = self.ens(pred.view(self.n, 1, self.action_dim), push=self._push)
