"""The convexity benchmark's fully connected segmentation network on the device (include/inrfit.h: inrfit_fcseg_*, csrc/fcseg.h).

An FCNet (awesome_amd.model.FCNet with an image input: Linear(F, 16), ReLU, depth x [Linear(16, 16), ReLU], Linear(16, 1), depth <= 3,
'rgb' / 'rgbxy' rows of at most 8 channels) trained with a plain mean BCELoss - the criterion of the benchmark's FCNet configs -
takes its whole step in HIP: one launch over the pixel rows (forward, the data term on the first `data_count` rows, the backward
and every weight gradient) and one fixed-order reduction (DESIGN.md "FCNet segmentation step").  Every other network or criterion
keeps the torch path; that is routing (`net_supported`, `criterion_form` return False / None)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from . import _lib as L
from . import _segnet as S
from ._segnet import _plain_bce, assign_grads  # noqa: F401 (assign_grads: part of this module's surface)
from .icnn import _check_dev


def net_supported(net) -> bool:
    """An FCNet of a shape the kernels are compiled for, fp32 on the GPU."""
    from .model.fc_net import FCNet
    if type(net) is not FCNet or not hasattr(net, "model") or net.in_type not in ("rgb", "rgbxy"):
        return False
    lins = net.linear_layers()
    return (net.width == 16 and 0 <= int(net.depth) <= 3 and net.out_chn == 1 and 1 <= int(net.in_chn) <= 8
            and len(lins) == net.depth + 2
            and all(m.bias is not None and m.weight.is_cuda and m.weight.dtype == torch.float32 and m.weight.is_contiguous()
                    and m.bias.is_contiguous() for m in lins))


@dataclass
class SegCriterionForm:
    """How `criterion(s, t)` is evaluated: the mean BCE over the rows the target covers."""
    penalty: bool = False


def criterion_form(criterion, kwargs=None) -> Optional[SegCriterionForm]:
    """The form of a plain mean BCELoss, or of GradientPenaltyLoss(BCELoss, mean) with its penalty off and no noneclass (what
    measures.losses then evaluates is that BCELoss); None for anything else."""
    from .measures.losses import GradientPenaltyLoss
    if _plain_bce(criterion):
        return SegCriterionForm()
    if (isinstance(criterion, GradientPenaltyLoss) and _plain_bce(criterion.criterion) and not criterion.apply_gradient_penalty
            and criterion.noneclass is None):
        return SegCriterionForm()
    return None


def make_desc(net, image_channels: int, n_rows: int, data_count: int = 0, inversion: bool = False, g: float = 1.0) -> L.InrFcSegDesc:
    d = L.InrFcSegDesc()
    d.in_channels, d.image_channels, d.width, d.depth = int(net.in_chn), int(image_channels), int(net.width), int(net.depth)
    d.inversion, d.g, d.n_rows, d.data_count = int(bool(inversion)), float(g), int(n_rows), int(data_count)
    return d


def _inputs(desc, image: Optional[Tensor], features: Optional[Tensor]):
    n, ic, fc = desc.n_rows, desc.image_channels, desc.in_channels - desc.image_channels
    if ic > 0:
        image = _check_dev(image.detach(), "image")
        assert image.numel() == ic * n, (tuple(image.shape), ic, n)
    else:
        image = None
    if fc > 0:
        features = _check_dev(features.detach().float(), "features")
        assert features.numel() == fc * n, (tuple(features.shape), fc, n)
    else:
        features = None
    return image, features


FcSegResult = S.SegResult      # logits / seg [n], loss [1] g mean BCE (None: forward without a target)

# (against cnnseg's driver only two fields change what a call does: the target covers the first `data_count` rows, and a forward
# without a target passes no loss cell; the others say where this family keeps the same things)
_DRIVER = S.SegDriver("fcseg", "FCNet", layers=lambda net: net.linear_layers(), inputs=_inputs,
                      n_points=lambda d: d.n_rows, n_target=lambda d: d.data_count or d.n_rows,
                      ws_key=lambda d: (d.in_channels, d.depth, d.n_rows), loss_without_target=False)


def param_count(desc: L.InrFcSegDesc) -> int:
    return _DRIVER.param_count(desc)


def forward(net, desc: L.InrFcSegDesc, image: Optional[Tensor], features: Optional[Tensor],
            target: Optional[Tensor] = None) -> FcSegResult:
    """f and s of the network on the rows [image | features] (and with `target` the loss); target None: the evaluation forward."""
    return _DRIVER.forward(net, desc, image, features, target)


def step(net, desc: L.InrFcSegDesc, image: Optional[Tensor], features: Optional[Tensor], target: Tensor,
         dseg: Optional[Tensor] = None, reuse_forward: bool = False, grads: Optional[Tensor] = None) -> FcSegResult:
    """The network's gradient of loss + sum(dseg * s) into `grads` ([param_count] float32, allocated when None).  reuse_forward:
    forward(..., target) ran with the same arguments just before (the joint step puts the prior's step in between), so f and s
    are not returned again."""
    assert grads is None or grads.is_cuda
    return _DRIVER.step(net, desc, image, features, target, dseg, reuse_forward, grads)
