"""SARNN policy network (policy/sarnn/SarnnPolicy.py:15-186 of the reference) with the reference's
parameter names, so its `policy.ckpt` loads with strict=True.

`forward` is the reference forward in plain torch (same inputs, same 5-tuple).  `step` is the
rollout's hot path: only the branch that reaches predicted_state (attention encoders, spatial
softmax, LSTM cell, state decoder) -- the image encoders, attention decoders, inverse spatial
softmax and image decoders feed the reference's plot only -- through the fused HIP kernels
(rmbx_sarnn_attention, rmbx_sarnn_lstm_step) where they apply, else the same torch modules.
RMBX_SARNN_FUSED=0 selects the torch modules on the device too (A/B measurements).

SpatialSoftmax / InverseSpatialSoftmax restate the two layers the reference imports from the `eipl`
package (absent here; unpinned against eipl itself).  Tensors are [B, C, R, Cc]; the reference passes
width = R and height = Cc, which only agrees with its (width, height) image sizes for square
images, so square images only.
"""

import os
from collections.abc import Iterable

import numpy as np
import torch
import torch.nn as nn

from ... import kernels as K
from ..derived import derived


def _grids(width, height):
    """(pos_x, pos_y) f32 [width, height]: pos_x[r, c] = c / (height - 1), pos_y[r, c] = r / (width - 1)."""
    px, py = np.meshgrid(np.linspace(0.0, 1.0, height), np.linspace(0.0, 1.0, width), indexing="xy")
    return torch.from_numpy(px).float(), torch.from_numpy(py).float()


class _GridBuffers(nn.Module):
    """Buffers that are functions of the layer's size: a checkpoint's copy must equal them."""

    _grid_names = ()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        for name in self._grid_names:
            t = state_dict.get(prefix + name)
            own = getattr(self, name)
            if t is not None and tuple(t.shape) == tuple(own.shape) and not torch.equal(
                    t.to(device=own.device, dtype=own.dtype), own):
                error_msgs.append(f"buffer {prefix + name} of the checkpoint differs from the position grid of a "
                                  f"{tuple(own.shape)} map")
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)


class SpatialSoftmax(_GridBuffers):
    _grid_names = ("pos_x", "pos_y")

    def __init__(self, width, height, temperature=1e-4, normalized=True):
        super().__init__()
        if not normalized:
            raise ValueError("SpatialSoftmax: only normalized=True is served")
        if not temperature > 0:
            raise ValueError(f"SpatialSoftmax: temperature {temperature} must be positive")
        self.width, self.height, self.temperature = int(width), int(height), float(temperature)
        px, py = _grids(self.width, self.height)
        self.register_buffer("pos_x", px.reshape(-1))
        self.register_buffer("pos_y", py.reshape(-1))

    def forward(self, x):
        B, C, R, Cc = x.shape
        if (R, Cc) != (self.width, self.height):
            raise ValueError(f"SpatialSoftmax({self.width}, {self.height}) got a {R} x {Cc} map")
        att = torch.softmax(x.reshape(B, C, -1) / self.temperature, dim=-1)
        ex = torch.sum(self.pos_x * att, dim=-1, keepdim=True)
        ey = torch.sum(self.pos_y * att, dim=-1, keepdim=True)
        return torch.cat([ex, ey], dim=-1), att.reshape(B, C, R, Cc)


class InverseSpatialSoftmax(_GridBuffers):
    _grid_names = ("pos_xy",)

    def __init__(self, width, height, heatmap_size=0.1, normalized=True):
        super().__init__()
        if not normalized:
            raise ValueError("InverseSpatialSoftmax: only normalized=True is served")
        self.width, self.height, self.heatmap_size = int(width), int(height), float(heatmap_size)
        self.register_buffer("pos_xy", torch.stack(_grids(self.width, self.height)))

    def forward(self, keys):
        d = self.pos_xy[None, None] - keys[:, :, :, None, None]
        return torch.exp(-torch.sum(d**2, dim=2) / self.heatmap_size)


class SarnnModel(nn.Module):
    def __init__(self, state_dim, num_images, image_size_list, num_attentions, lstm_hidden_dim):
        kernel_size = 3
        softmax_temperature = 1e-4
        inv_softmax_heatmap_size = 0.1
        if isinstance(image_size_list[0], Iterable):
            if num_images != len(image_size_list):
                raise ValueError(f"{len(image_size_list)} image sizes for {num_images} images")
            image_size_list = [tuple(int(v) for v in s) for s in image_size_list]
        else:
            image_size_list = [tuple(int(v) for v in image_size_list)] * num_images
        for size in image_size_list:
            if len(size) != 2 or size[0] != size[1]:
                raise ValueError(f"image size {size} is not square: image_size_list is (width, height) while the "
                                 "tensors are [3, height, width], and the spatial softmax takes its size in that "
                                 "swapped order, so only square images are consistent")
            if size[0] < 8:
                raise ValueError(f"image size {size} leaves no map after three valid 3x3 convolutions")
        super().__init__()
        self.state_dim, self.num_images = int(state_dim), int(num_images)
        self.num_attentions, self.lstm_hidden_dim = int(num_attentions), int(lstm_hidden_dim)
        self.image_size_list = image_size_list
        self.temperature = softmax_temperature
        activation = nn.LeakyReLU(negative_slope=0.3)
        enc_sizes = [(s[0] - 3 * (kernel_size - 1), s[1] - 3 * (kernel_size - 1)) for s in image_size_list]
        K_ = self.num_attentions

        self.attention_encoder_list = nn.ModuleList(
            nn.Sequential(nn.Conv2d(3, 16, kernel_size, 1, 0), activation, nn.Conv2d(16, 32, kernel_size, 1, 0),
                          activation, nn.Conv2d(32, K_, kernel_size, 1, 0), activation,
                          SpatialSoftmax(width=e[0], height=e[1], temperature=softmax_temperature, normalized=True))
            for e in enc_sizes)
        self.image_encoder_list = nn.ModuleList(
            nn.Sequential(nn.Conv2d(3, 16, kernel_size, 1, 0), activation, nn.Conv2d(16, 32, kernel_size, 1, 0),
                          activation, nn.Conv2d(32, K_, kernel_size, 1, 0), activation)
            for _ in range(num_images))
        self.lstm = nn.LSTMCell(state_dim + num_images * K_ * 2, lstm_hidden_dim)
        self.state_decoder = nn.Sequential(nn.Linear(lstm_hidden_dim, state_dim))
        self.attention_decoder_list = nn.ModuleList(
            nn.Sequential(nn.Linear(lstm_hidden_dim, K_ * 2), activation) for _ in range(num_images))
        self.inv_softmax_list = nn.ModuleList(
            InverseSpatialSoftmax(width=e[0], height=e[1], heatmap_size=inv_softmax_heatmap_size, normalized=True)
            for e in enc_sizes)
        self.image_decoder_list = nn.ModuleList(
            nn.Sequential(nn.ConvTranspose2d(K_, 32, kernel_size, 1, 0), activation,
                          nn.ConvTranspose2d(32, 16, kernel_size, 1, 0), activation,
                          nn.ConvTranspose2d(16, 3, kernel_size, 1, 0))
            for _ in range(num_images))
        self.apply(self._initialize_weights)

    @staticmethod
    def _initialize_weights(m):
        """SarnnPolicy._initialize_weights (:119-131)."""
        if isinstance(m, nn.LSTMCell):
            nn.init.xavier_uniform_(m.weight_ih)
            nn.init.orthogonal_(m.weight_hh)
            nn.init.zeros_(m.bias_ih)
            nn.init.zeros_(m.bias_hh)
        elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear)):
            nn.init.xavier_uniform_(m.weight)
            nn.init.zeros_(m.bias)

    def forward(self, state, image_list, lstm_state=None):
        """SarnnPolicy.forward (:133-186), unfused."""
        if len(image_list) != len(self.image_encoder_list):
            raise ValueError(f"{len(image_list)} images for {len(self.image_encoder_list)} cameras")
        encoded_image_list = [enc(image) for image, enc in zip(image_list, self.image_encoder_list)]
        attention_list = [enc(image)[0].reshape(-1, self.num_attentions * 2)
                          for image, enc in zip(image_list, self.attention_encoder_list)]
        lstm_output = self.lstm(torch.cat([state, *attention_list], dim=-1), lstm_state)
        predicted_state = self.state_decoder(lstm_output[0])
        predicted_attention_list = [dec(lstm_output[0]).reshape(-1, self.num_attentions, 2)
                                    for dec in self.attention_decoder_list]
        predicted_image_list = [
            image_decoder(torch.mul(inv_softmax(predicted_attention), encoded_image))
            for encoded_image, predicted_attention, inv_softmax, image_decoder in zip(
                encoded_image_list, predicted_attention_list, self.inv_softmax_list, self.image_decoder_list)]
        attention_list = [a.reshape(-1, self.num_attentions, 2) for a in attention_list]
        return predicted_state, predicted_image_list, attention_list, predicted_attention_list, lstm_output

    # -- rollout hot path ----------------------------------------------------------------------
    def attention_points(self, images):
        """The attention encoders alone, unfused: images [n, ncam, 3, S, S] -> [n, ncam, K, 2]."""
        return torch.stack([enc(images[:, i])[0] for i, enc in enumerate(self.attention_encoder_list)], dim=1)

    def fused(self, images):
        """Whether `step` serves these images with the HIP kernels."""
        if os.environ.get("RMBX_SARNN_FUSED", "1") == "0" or not images.is_cuda:
            return False
        return (len(set(self.image_size_list)) == 1 and images.dtype == torch.float32
                and K.sarnn_supported(self.image_size_list[0][0], self.num_attentions, self.num_images, self.state_dim,
                                      self.lstm_hidden_dim))

    def _packed(self):
        """Per-camera conv weights and biases packed camera-major, as rmbx_sarnn_attention reads them."""
        convs = [[enc[i] for enc in self.attention_encoder_list] for i in (0, 2, 4)]
        src = [p for layer in convs for m in layer for p in (m.weight, m.bias)]
        return derived(self, "sarnn_attention", src, lambda: K.sarnn_pack_attention(convs))

    @torch.no_grad()
    def step(self, state, images, h, c, active=None):
        """One recurrent step for n envs: state f32 [n, S], images f32 [n, ncam, 3, S, S], h / c f32
        [n, Hd] updated in place -> (predicted_state [n, S], attention points [n, ncam, K, 2])."""
        n = state.shape[0]
        if self.fused(images):
            keys = K.sarnn_attention(images, self._packed(), self.temperature)
            lin = self.state_decoder[0]
            pred = K.sarnn_lstm_step(state, keys.view(n, -1), h, c, self.lstm.weight_ih, self.lstm.weight_hh,
                                     self.lstm.bias_ih, self.lstm.bias_hh, lin.weight, lin.bias, active=active)
            return pred, keys
        if active is not None:
            raise ValueError("the unfused step takes no active mask")
        keys = self.attention_points(images)
        hn, cn = self.lstm(torch.cat([state, keys.reshape(n, -1)], dim=-1), (h, c))
        h.copy_(hn)
        c.copy_(cn)
        return self.state_decoder(hn), keys
