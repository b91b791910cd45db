"""awesome/model/cnn_net.py: the convexity benchmark's segmentation network (the `segmentation_model_type` of its CNNNet configs).

Conv(in_chn -> width), LeakyReLU, depth x [Conv(width -> width), ReLU], Conv(width -> out_chn), every convolution k x k with padding
k // 2, under the same `model.*` names and in the same construction order as the reference, so a seeded construction gives its
initial weights.  `forward` is plain torch (the autograd path needs its double backward); the fused joint step runs the supported
shapes through the HIP step of awesome_amd.cnnseg instead."""
from __future__ import annotations

from typing import Literal, Optional

import torch
import torch.nn as nn


def conv_relu(width: int, kernel_size: int) -> nn.Sequential:
    return nn.Sequential(nn.Conv2d(width, width, kernel_size=kernel_size, padding=kernel_size // 2), nn.ReLU())


def concat_input(in_type: Literal["rgb", "xy", "rgbxy"], patch_image: torch.Tensor, patch_grid: torch.Tensor) -> torch.Tensor:
    """The network's input: the image, the spatial / semantic features, or both concatenated along the channels."""
    if in_type == "rgb":
        return patch_image
    if in_type == "xy":
        return patch_grid
    if in_type == "rgbxy":
        return torch.cat((patch_image, patch_grid.float()), dim=1)
    raise ValueError(f"in_type must be one of: rgb, xy, rgbxy but was: {in_type}")


def _batcherize(*args):
    """awesome/util/batcherize.py with keep=True, expected_dim=4: tensors of fewer dimensions get leading ones."""
    return tuple(a[(None,) * (4 - a.dim()) + (Ellipsis,)] if isinstance(a, torch.Tensor) and a.dim() < 4 else a for a in args)


class CNNNet(nn.Module):
    """Convolutional network of variable width and depth (in_type: 'rgb', 'xy' or 'rgbxy'; `input` is the config's name for it)."""

    def __init__(self, in_chn: Optional[int] = None, out_chn: Optional[int] = None, kernel_size: Optional[int] = None,
                 width: Optional[int] = None, depth: Optional[int] = None, in_type: Optional[str] = None, input: Optional[str] = None,
                 decoding: bool = False):
        if decoding:
            return
        super().__init__()
        self.in_chn, self.out_chn, self.in_type = in_chn, out_chn, in_type
        assert (kernel_size % 2) == 1
        self.kernel_size, self.width, self.depth = kernel_size, width, depth
        conv_blocks = [conv_relu(width, kernel_size) for _ in range(depth)]
        self.model = nn.Sequential(nn.Conv2d(in_chn, width, kernel_size=kernel_size, padding=kernel_size // 2), nn.LeakyReLU(),
                                   *conv_blocks, nn.Conv2d(width, out_chn, kernel_size=kernel_size, padding=kernel_size // 2))

    def forward(self, image, grid, *args, no_extend: bool = False, **kwargs):
        if not no_extend:
            image, grid = _batcherize(image, grid)
        return self.model(concat_input(self.in_type, image, grid))

    def conv_layers(self):
        """The convolutions in order (layer 0 .. depth + 1)."""
        return [m for m in self.model.modules() if isinstance(m, nn.Conv2d)]
