"""awesome/model/unet.py: the path-connectedness configs' segmentation backbone (`segmentation_model_type: awesome.model.unet.UNet`).

InConv, four Down blocks (2 x 2 max-pool + two [Conv 3 x 3, BatchNorm, ReLU]), four Up blocks (bilinear x2 upsampling with
align_corners, padded to the skip map's size and concatenated behind it, two [Conv 3 x 3, BatchNorm, ReLU]) and a 1 x 1 OutConv, under
the reference's sub-module names and in its construction order, so a seeded construction gives its state_dict.  Channel widths are
`base_width` (1, 2, 4, 8, 8) going down and `base_width` (4, 2, 1, 1) coming up; the reference is base_width 64.

In evaluation mode under no_grad - what the pre-fit loops and inference do with a frozen checkpoint - an fp32 network on the GPU runs
in HIP (awesome_amd.unet, csrc/unet.h).  With `hip_training=True` a training step on one image - the forward pass with batch statistics
and the whole backward pass - runs in HIP as well (csrc/unet_train.h), as an autograd function over the parameters.  Everything else
(a batch of several images, inputs that require grad, other dtypes) is the plain torch modules."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .cnn_net import _batcherize

MIN_HIP_SIDE = 16     # four max-pools must leave a pixel
MAX_HIP_SIDE = 4096


class DoubleConv(nn.Module):
    """(conv => BN => ReLU) * 2"""

    def __init__(self, in_ch: int, out_ch: int, dtype: torch.dtype = torch.float32):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_ch, out_ch, 3, padding=1, dtype=dtype), nn.BatchNorm2d(out_ch, dtype=dtype), nn.ReLU(inplace=True),
                                  nn.Conv2d(out_ch, out_ch, 3, padding=1, dtype=dtype), nn.BatchNorm2d(out_ch, dtype=dtype), nn.ReLU(inplace=True))

    def forward(self, x):
        return self.conv(x)


class InConv(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, dtype: torch.dtype = torch.float32):
        super().__init__()
        self.conv = DoubleConv(in_ch, out_ch, dtype=dtype)

    def forward(self, x):
        return self.conv(x)


class Down(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, dtype: torch.dtype = torch.float32):
        super().__init__()
        self.mpconv = nn.Sequential(nn.MaxPool2d(2), DoubleConv(in_ch, out_ch, dtype=dtype))

    def forward(self, x):
        return self.mpconv(x)


class Up(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, bilinear: bool = True, dtype: torch.dtype = torch.float32):
        super().__init__()
        if not bilinear:
            raise NotImplementedError("Up(bilinear=False) (a transposed convolution) is not part of this build")
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self.conv = DoubleConv(in_ch, out_ch, dtype=dtype)

    def forward(self, x1, x2):
        x1 = self.up(x1)
        dy, dx = x2.size(2) - x1.size(2), x2.size(3) - x1.size(3)
        x1 = F.pad(x1, (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2))
        return self.conv(torch.cat([x2, x1], dim=1))


class OutConv(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, dtype: torch.dtype = torch.float32):
        super().__init__()
        self.conv = nn.Conv2d(in_ch, out_ch, 1, dtype=dtype)

    def forward(self, x):
        return self.conv(x)


class UNet(nn.Module):
    def __init__(self, in_chn: Optional[int] = None, out_chn: int = 1, dtype: torch.dtype = torch.float32, decoding: bool = False, *,
                 base_width: int = 64, hip_training: bool = False):
        super().__init__()
        self.hip_training = bool(hip_training)     # a switch, not a weight: no part of the state_dict
        if decoding:
            return
        b = int(base_width)
        self.in_chn, self.out_chn, self.base_width = in_chn, out_chn, b
        self.inc = InConv(in_chn, b, dtype=dtype)
        self.down1 = Down(b, 2 * b, dtype=dtype)
        self.down2 = Down(2 * b, 4 * b, dtype=dtype)
        self.down3 = Down(4 * b, 8 * b, dtype=dtype)
        self.down4 = Down(8 * b, 8 * b, dtype=dtype)
        self.up1 = Up(16 * b, 4 * b, dtype=dtype)
        self.up2 = Up(8 * b, 2 * b, dtype=dtype)
        self.up3 = Up(4 * b, b, dtype=dtype)
        self.up4 = Up(2 * b, b, dtype=dtype)
        self.outc = OutConv(b, out_chn, dtype=dtype)

    def blocks(self):
        """The nine DoubleConvs in state_dict order."""
        return [self.inc.conv] + [d.mpconv[1] for d in (self.down1, self.down2, self.down3, self.down4)] + \
               [u.conv for u in (self.up1, self.up2, self.up3, self.up4)]

    def forward_torch(self, image, feature_encoding):
        x1 = self.inc(torch.cat((image, feature_encoding), dim=1))
        x2 = self.down1(x1)
        x3 = self.down2(x2)
        x4 = self.down3(x3)
        x5 = self.down4(x4)
        x = self.up1(x5, x4)
        x = self.up2(x, x3)
        x = self.up3(x, x2)
        x = self.up4(x, x1)
        return self.outc(x)

    def _hip_shape(self, image, feature_encoding) -> bool:
        """fp32 tensors on one GPU, parameters and buffers included, at a shape the library holds kernels for."""
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in (image, feature_encoding)):
            return False
        if image.shape[-2] < MIN_HIP_SIDE or image.shape[-1] < MIN_HIP_SIDE or image.shape[-2:] != feature_encoding.shape[-2:]:
            return False
        if self.base_width % 4 or self.base_width > 64 or self.out_chn > 8 or image.shape[1] + feature_encoding.shape[1] != self.in_chn:
            return False
        return all(t.is_cuda and t.device == image.device and (t.dtype == torch.float32 or not t.is_floating_point())
                   for t in list(self.parameters()) + list(self.buffers()))

    def hip_route(self, image, feature_encoding) -> bool:
        """Evaluation mode, no autograd, fp32 on a GPU, at least 16 x 16 - and a shape the library holds kernels for."""
        if self.training or torch.is_grad_enabled():
            return False
        return self._hip_shape(image, feature_encoding)

    def hip_train_route(self, image, feature_encoding) -> bool:
        """`hip_training`, train() with autograd on, one image whose tensors do not require grad, fp32 on one GPU, BatchNorms with
        affine weights, running statistics, one eps and one float momentum, at least two values per channel at the bottom level."""
        if not getattr(self, "hip_training", False) or not self.training or not torch.is_grad_enabled():
            return False
        if not self._hip_shape(image, feature_encoding) or image.device != feature_encoding.device:
            return False
        if image.requires_grad or feature_encoding.requires_grad or image.dim() != 4 or image.shape[0] != 1 or feature_encoding.shape[0] != 1:
            return False
        h, w = image.shape[-2:]
        if (h >> 4) * (w >> 4) < 2 or h > MAX_HIP_SIDE or w > MAX_HIP_SIDE:
            return False
        if any(not p.is_contiguous() for p in self.parameters()):
            return False
        from ..unet import train_momentum
        return train_momentum(self) is not None

    def forward(self, image, feature_encoding, *args, **kwargs):
        image, feature_encoding = _batcherize(image, feature_encoding)
        if self.hip_route(image, feature_encoding):
            from ..unet import unet_forward
            return unet_forward(self, image, feature_encoding)
        if self.hip_train_route(image, feature_encoding):
            from ..unet import unet_train_forward
            return unet_train_forward(self, image, feature_encoding)
        return self.forward_torch(image, feature_encoding)
