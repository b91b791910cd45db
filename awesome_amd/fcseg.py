"""The convexity benchmark's fully connected segmentation network on the device (include/inrfit.h: inrfit_fcseg_*, csrc/fcseg.h).

An FCNet (awesome_amd.model.FCNet with an image input: Linear(F, 16), ReLU, depth x [Linear(16, 16), ReLU], Linear(16, 1), depth <= 3,
'rgb' / 'rgbxy' rows of at most 8 channels) trained with a plain mean BCELoss - the criterion of the benchmark's FCNet configs -
takes its whole step in HIP: one launch over the pixel rows (forward, the data term on the first `data_count` rows, the backward
and every weight gradient) and one fixed-order reduction (DESIGN.md "FCNet segmentation step").  Every other network or criterion
keeps the torch path; that is routing (`net_supported`, `criterion_form` return False / None)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from . import _lib as L
from .icnn import _check_dev, _stream_ptr


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


def _plain_bce(c) -> bool:
    return type(c) is torch.nn.BCELoss and c.weight is None and c.reduction == "mean"


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


def param_count(desc: L.InrFcSegDesc) -> int:
    n = L.load().inrfit_fcseg_param_count(C.byref(desc))
    if n < 0:
        raise L.InrfitError("inrfit_fcseg_param_count: unsupported FCNet shape")
    return int(n)


_ws_cache = {}


def _workspace(desc: L.InrFcSegDesc, dev) -> Tensor:
    """One workspace per (shape, device)."""
    key = (desc.in_channels, desc.depth, desc.n_rows, str(dev))
    ws = _ws_cache.get(key)
    if ws is None:
        nbytes = int(L.load().inrfit_fcseg_workspace_bytes(C.byref(desc)))
        if nbytes < 0:
            raise L.InrfitError("inrfit_fcseg_workspace_bytes: unsupported FCNet shape")
        ws = _ws_cache[key] = L.scratch(nbytes // 4 + 64, dtype=torch.float32, device=dev)
    return ws


def _layer_ptrs(net):
    lins = net.linear_layers()
    w = (C.c_void_p * len(lins))(*[m.weight.data_ptr() for m in lins])
    b = (C.c_void_p * len(lins))(*[m.bias.data_ptr() for m in lins])
    return C.cast(w, C.c_void_p), C.cast(b, C.c_void_p), (w, b)       # (the arrays stay alive with the caller's reference)


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


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


@dataclass
class FcSegResult:
    logits: Optional[Tensor]   # [n] f
    seg: Optional[Tensor]      # [n] s
    loss: Optional[Tensor]     # [1] g mean BCE (None: forward without a target)
    grads: Optional[Tensor] = None    # [P] in parameters() order
    status: Optional[Tensor] = None   # [1] int32: 1 = non-finite loss or gradient (grads zeroed)


def _target(desc, target: Tensor) -> Tensor:
    target = _check_dev(target.detach().float(), "target")
    assert target.numel() == (desc.data_count or desc.n_rows), (tuple(target.shape), desc.data_count, desc.n_rows)
    return target


def forward(net, desc: L.InrFcSegDesc, image: Optional[Tensor], features: Optional[Tensor],
            target: Optional[Tensor] = None) -> FcSegResult:
    """f and s of the network on the rows [image | features] (and with `target` the loss); target None: the evaluation forward."""
    dev = (image if image is not None else features).device
    n = desc.n_rows
    image, features = _inputs(desc, image, features)
    loss = None
    if target is not None:
        target = _target(desc, target)
        loss = L.scratch(1, dtype=torch.float32, device=dev)
    w, b, _keep = _layer_ptrs(net)
    logits = L.scratch(n, dtype=torch.float32, device=dev)
    seg = L.scratch(n, dtype=torch.float32, device=dev)
    ws = _workspace(desc, dev)
    rc = L.load().inrfit_fcseg_forward(C.byref(desc), w, b, _ptr(image), _ptr(features), _ptr(target), logits.data_ptr(),
                                       seg.data_ptr(), _ptr(loss), ws.data_ptr(), ws.numel() * 4, _stream_ptr(dev))
    L.check(rc, "inrfit_fcseg_forward")
    return FcSegResult(logits, seg, loss)


def step(net, desc: L.InrFcSegDesc, image: Optional[Tensor], features: Optional[Tensor], target: Tensor,
         dseg: Optional[Tensor] = None, reuse_forward: bool = False, grads: Optional[Tensor] = None) -> FcSegResult:
    """The network's gradient of loss + sum(dseg * s) into `grads` ([param_count] float32, allocated when None).  reuse_forward:
    forward(..., target) ran with the same arguments just before (the joint step puts the prior's step in between), so f and s
    are not returned again."""
    dev = (image if image is not None else features).device
    n = desc.n_rows
    image, features = _inputs(desc, image, features)
    target = _target(desc, target)
    if dseg is not None:
        dseg = _check_dev(dseg.detach(), "dseg")
        assert dseg.numel() == n
    P = param_count(desc)
    if grads is None:
        grads = L.scratch(P, dtype=torch.float32, device=dev)
    assert grads.numel() == P and grads.is_contiguous() and grads.dtype == torch.float32 and grads.is_cuda
    w, b, _keep = _layer_ptrs(net)
    logits = seg = None
    if not reuse_forward:
        logits = L.scratch(n, dtype=torch.float32, device=dev)
        seg = L.scratch(n, dtype=torch.float32, device=dev)
    loss = L.scratch(1, dtype=torch.float32, device=dev)
    status = L.scratch(1, dtype=torch.int32, device=dev)      # (always written)
    ws = _workspace(desc, dev)
    rc = L.load().inrfit_fcseg_step(C.byref(desc), w, b, _ptr(image), _ptr(features), target.data_ptr(), _ptr(dseg),
                                    int(bool(reuse_forward)), _ptr(logits), _ptr(seg), loss.data_ptr(), grads.data_ptr(),
                                    status.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream_ptr(dev))
    L.check(rc, "inrfit_fcseg_step")
    return FcSegResult(logits, seg, loss, grads, status)


def assign_grads(net, grads: Tensor) -> None:
    """Every parameter's .grad becomes its view of the flat gradient buffer (parameters() order)."""
    off = 0
    for p in net.parameters():
        k = p.numel()
        p.grad = grads[off:off + k].view_as(p)
        off += k
    assert off == grads.numel()
