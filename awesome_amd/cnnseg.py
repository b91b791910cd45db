"""The convexity benchmark's segmentation network on the device (include/inrfit.h: inrfit_cnnseg_*, csrc/cnnseg.h).

A CNNNet (awesome_amd.model.CNNNet: 3x3 convolutions, width 16, depth <= 3, one output channel, 'rgbxy' input of at most 8
channels) trained with BCELoss or GradientPenaltyLoss(BCELoss) - the criterion of the benchmark's CNNNet configs - takes its whole
step in HIP: forward, the data term, the gradient penalty's value (the backward of sum(s) to the input) and its gradient with
respect to every weight (a tangent forward and one backward with the masks fixed, DESIGN.md "CNNNet segmentation step").  Every
other network or criterion keeps the torch path; that is routing (`net_supported`, `criterion_form` return False / None)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from . import _segnet as S
from ._segnet import _plain_bce, assign_grads  # noqa: F401 (assign_grads: part of this module's surface)
from .icnn import _check_dev

GROUP_NONE, GROUP_RGB, GROUP_XY, GROUP_FEAT = -1, 0, 1, 2


def net_supported(net) -> bool:
    """A CNNNet of a shape the kernels are compiled for, fp32 on the GPU."""
    from .model.cnn_net import CNNNet
    if type(net) is not CNNNet or not hasattr(net, "model"):
        return False
    convs = net.conv_layers()
    return (net.in_type == "rgbxy" and net.kernel_size == 3 and net.width == 16 and 0 <= int(net.depth) <= 3 and net.out_chn == 1
            and 1 <= int(net.in_chn) <= 8 and len(convs) == net.depth + 2
            and all(c.bias is not None and c.weight.is_cuda and c.weight.dtype == torch.float32 and c.weight.is_contiguous()
                    and c.padding == (1, 1) and c.stride == (1, 1) and c.dilation == (1, 1) and c.groups == 1 for c in convs))


@dataclass
class SegCriterionForm:
    """How `criterion(s, t, **kwargs)` is evaluated: BCE on the pixels whose target is not `noneclass`, plus - `penalty` -
    coef[group] * mean |d sum(s) / d input| over the group's channels (rgb: the image, xy / feat: the features by `xytype`)."""
    noneclass: Optional[float]
    penalty: bool
    coef: Tuple[float, float, float]
    xytype: str

    def channel_groups(self, image_channels: int, in_channels: int):
        out = []
        for c in range(in_channels):
            r = c - image_channels
            if r < 0:
                out.append(GROUP_RGB)
            elif self.xytype == "xy":
                out.append(GROUP_XY)
            elif self.xytype == "feat":
                out.append(GROUP_FEAT)
            elif self.xytype == "featxy":
                out.append(GROUP_XY if r < 2 else GROUP_FEAT)
            else:
                out.append(GROUP_NONE)
        return out


def criterion_form(criterion, kwargs, image_channels: int, in_channels: int) -> Optional[SegCriterionForm]:
    """The form of BCELoss / GradientPenaltyLoss(BCELoss, mean) as measures.losses evaluates it with these kwargs, or None (anything
    else, and every call torch would refuse or answer with NaN by construction: the penalty without `_input`, an empty group)."""
    from .measures.losses import GradientPenaltyLoss
    if _plain_bce(criterion):
        return SegCriterionForm(None, False, (0.0, 0.0, 0.0), "xy")
    if not isinstance(criterion, GradientPenaltyLoss) or not _plain_bce(criterion.criterion):
        return None
    nc = None if criterion.noneclass is None else float(criterion.noneclass)
    if not criterion.apply_gradient_penalty:
        return SegCriterionForm(nc, False, (0.0, 0.0, 0.0), criterion.xytype)
    if kwargs.get("_input") is None:
        return None
    xyg, fg, rg = float(criterion.xygrad), float(criterion.featgrad), float(criterion.rgbgrad)
    c_xy = c_feat = 0.0
    if xyg > 0.0 or fg > 0.0:
        if criterion.xytype in ("xy", "featxy") and xyg > 0.0:
            c_xy = xyg
        if criterion.xytype in ("feat", "featxy") and fg > 0.0:
            c_feat = fg
    form = SegCriterionForm(nc, False, (rg if rg > 0.0 else 0.0, c_xy, c_feat), criterion.xytype)
    groups = form.channel_groups(image_channels, in_channels)
    for grp, coef in enumerate(form.coef):
        if coef > 0.0 and grp not in groups:
            return None       # the mean of an empty group: NaN in torch
    form.penalty = any(c > 0.0 for c in form.coef)
    return form


def make_desc(net, image_channels: int, height: int, width: int, form: SegCriterionForm, inversion: bool = False,
              g: float = 1.0) -> L.InrCnnSegDesc:
    d = L.InrCnnSegDesc()
    d.in_channels, d.image_channels, d.width, d.depth, d.kernel_size = int(net.in_chn), int(image_channels), int(net.width), int(net.depth), 3
    d.height, d.width_px, d.inversion = int(height), int(width), int(bool(inversion))
    d.use_noneclass, d.noneclass = int(form.noneclass is not None), float(form.noneclass if form.noneclass is not None else 0.0)
    d.g, d.penalty = float(g), int(form.penalty)
    for i, c in enumerate(form.coef):
        d.coef[i] = float(c)
    groups = form.channel_groups(image_channels, int(net.in_chn))
    for i in range(8):
        d.channel_group[i] = groups[i] if i < len(groups) else GROUP_NONE
    return d


def _inputs(desc, image: Tensor, features: Optional[Tensor]):
    n = desc.height * desc.width_px
    image = _check_dev(image.detach(), "image")
    assert image.numel() == desc.image_channels * n, (tuple(image.shape), desc.image_channels, n)
    if desc.image_channels < desc.in_channels:
        features = _check_dev(features.detach().float(), "features")
        assert features.numel() == (desc.in_channels - desc.image_channels) * n
    else:
        features = None
    return image, features


CnnSegResult = S.SegResult     # logits / seg [H W], loss [1] g (crit + penalties)

# (against fcseg's driver only two fields change what a call does: the target covers every pixel, and a forward without a target
# still passes a loss cell; the others say where this family keeps the same things)
_DRIVER = S.SegDriver("cnnseg", "CNNNet", layers=lambda net: net.conv_layers(), inputs=_inputs,
                      n_points=lambda d: d.height * d.width_px, n_target=lambda d: d.height * d.width_px,
                      ws_key=lambda d: (d.in_channels, d.width, d.depth, d.height, d.width_px), loss_without_target=True)


def param_count(desc: L.InrCnnSegDesc) -> int:
    return _DRIVER.param_count(desc)


def forward(net, desc: L.InrCnnSegDesc, image: Tensor, features: Optional[Tensor], target: Optional[Tensor] = None) -> CnnSegResult:
    """f and s of the network (and with `target` the loss, kept in the workspace for step(..., reuse_forward=True))."""
    return _DRIVER.forward(net, desc, image, features, target)


def step(net, desc: L.InrCnnSegDesc, image: Tensor, features: Optional[Tensor], target: Tensor, dseg: Optional[Tensor] = None,
         reuse_forward: bool = False, grads: Optional[Tensor] = None) -> CnnSegResult:
    """The network's gradient of loss + sum(dseg * s) into `grads` ([param_count] float32, allocated when None).  reuse_forward:
    forward(..., target) ran with the same arguments just before (the joint step puts the prior's step in between)."""
    return _DRIVER.step(net, desc, image, features, target, dseg, reuse_forward, grads)
