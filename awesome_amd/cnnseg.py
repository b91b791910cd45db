"""The convexity benchmark's segmentation network on the device (include/inrfit.h: inrfit_cnnseg_*, csrc/cnnseg.h).

A CNNNet (awesome_amd.model.CNNNet: 3x3 convolutions, width 16, depth <= 3, one output channel, 'rgbxy' input of at most 8
channels) trained with BCELoss or GradientPenaltyLoss(BCELoss) - the criterion of the benchmark's CNNNet configs - takes its whole
step in HIP: forward, the data term, the gradient penalty's value (the backward of sum(s) to the input) and its gradient with
respect to every weight (a tangent forward and one backward with the masks fixed, DESIGN.md "CNNNet segmentation step").  Every
other network or criterion keeps the torch path; that is routing (`net_supported`, `criterion_form` return False / None)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from .icnn import _check_dev, _stream_ptr

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


def _plain_bce(c) -> bool:
    return type(c) is torch.nn.BCELoss and c.weight is None and c.reduction == "mean"


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


def param_count(desc: L.InrCnnSegDesc) -> int:
    n = L.load().inrfit_cnnseg_param_count(C.byref(desc))
    if n < 0:
        raise L.InrfitError("inrfit_cnnseg_param_count: unsupported CNNNet shape")
    return int(n)


_ws_cache = {}


def _workspace(desc: L.InrCnnSegDesc, dev) -> Tensor:
    """One workspace per (shape, device): inrfit_cnnseg_step(reuse_forward=1) reads what inrfit_cnnseg_forward left in it."""
    key = (desc.in_channels, desc.width, desc.depth, desc.height, desc.width_px, str(dev))
    ws = _ws_cache.get(key)
    if ws is None:
        nbytes = int(L.load().inrfit_cnnseg_workspace_bytes(C.byref(desc)))
        if nbytes < 0:
            raise L.InrfitError("inrfit_cnnseg_workspace_bytes: unsupported CNNNet shape")
        ws = _ws_cache[key] = L.scratch(nbytes // 4 + 64, dtype=torch.float32, device=dev)
    return ws


def _layer_ptrs(net):
    convs = net.conv_layers()
    w = (C.c_void_p * len(convs))(*[c.weight.data_ptr() for c in convs])
    b = (C.c_void_p * len(convs))(*[c.bias.data_ptr() for c in convs])
    return C.cast(w, C.c_void_p), C.cast(b, C.c_void_p), (w, b)       # (the arrays stay alive with the caller's reference)


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


@dataclass
class CnnSegResult:
    logits: Optional[Tensor]   # [H W] f
    seg: Optional[Tensor]      # [H W] s
    loss: Tensor               # [1] g (crit + penalties)
    grads: Optional[Tensor] = None    # [P] in parameters() order
    status: Optional[Tensor] = None   # [1] int32: 1 = non-finite loss or gradient (grads zeroed)


def forward(net, desc: L.InrCnnSegDesc, image: Tensor, features: Optional[Tensor], target: Optional[Tensor] = None) -> CnnSegResult:
    """f and s of the network (and with `target` the loss, kept in the workspace for step(..., reuse_forward=True))."""
    dev = image.device
    n = desc.height * desc.width_px
    image, features = _inputs(desc, image, features)
    if target is not None:
        target = _check_dev(target.detach().float(), "target")
        assert target.numel() == n
    w, b, _keep = _layer_ptrs(net)
    logits = L.scratch(n, dtype=torch.float32, device=dev)
    seg = L.scratch(n, dtype=torch.float32, device=dev)
    loss = L.scratch(1, dtype=torch.float32, device=dev)
    ws = _workspace(desc, dev)
    rc = L.load().inrfit_cnnseg_forward(C.byref(desc), w, b, image.data_ptr(), None if features is None else features.data_ptr(),
                                        None if target is None else target.data_ptr(), logits.data_ptr(), seg.data_ptr(),
                                        loss.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream_ptr(dev))
    L.check(rc, "inrfit_cnnseg_forward")
    return CnnSegResult(logits, seg, loss)


def step(net, desc: L.InrCnnSegDesc, image: Tensor, features: Optional[Tensor], target: Tensor, dseg: Optional[Tensor] = None,
         reuse_forward: bool = False, grads: Optional[Tensor] = None) -> CnnSegResult:
    """The network's gradient of loss + sum(dseg * s) into `grads` ([param_count] float32, allocated when None).  reuse_forward:
    forward(..., target) ran with the same arguments just before (the joint step puts the prior's step in between)."""
    dev = image.device
    n = desc.height * desc.width_px
    image, features = _inputs(desc, image, features)
    target = _check_dev(target.detach().float(), "target")
    assert target.numel() == n
    if dseg is not None:
        dseg = _check_dev(dseg.detach(), "dseg")
        assert dseg.numel() == n
    P = param_count(desc)
    if grads is None:
        grads = L.scratch(P, dtype=torch.float32, device=dev)
    assert grads.numel() == P and grads.is_contiguous() and grads.dtype == torch.float32
    w, b, _keep = _layer_ptrs(net)
    logits = seg = None
    if not reuse_forward:
        logits = L.scratch(n, dtype=torch.float32, device=dev)
        seg = L.scratch(n, dtype=torch.float32, device=dev)
    loss = L.scratch(1, dtype=torch.float32, device=dev)
    status = L.scratch(1, dtype=torch.int32, device=dev)      # (always written)
    ws = _workspace(desc, dev)
    rc = L.load().inrfit_cnnseg_step(C.byref(desc), w, b, image.data_ptr(), None if features is None else features.data_ptr(),
                                     target.data_ptr(), None if dseg is None else dseg.data_ptr(), int(bool(reuse_forward)),
                                     None if logits is None else logits.data_ptr(), None if seg is None else seg.data_ptr(),
                                     loss.data_ptr(), grads.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                     _stream_ptr(dev))
    L.check(rc, "inrfit_cnnseg_step")
    return CnnSegResult(logits, seg, loss, grads, status)


def assign_grads(net, grads: Tensor) -> None:
    """Every parameter's .grad becomes its view of the flat gradient buffer (parameters() order)."""
    off = 0
    for p in net.parameters():
        k = p.numel()
        p.grad = grads[off:off + k].view_as(p)
        off += k
    assert off == grads.numel()
