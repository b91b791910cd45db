"""Host-side driver of the fused joint-training step (include/inrfit.h: inrfit_joint_step / _pcn_joint_step / _cdn_joint_step).

One call = everything of TorchAgent._perform_step (awesome/agent/torch_agent.py:428-551) that lies behind the segmentation
network's output, for ONE image: prior forward on this image's parameter row, sigmoid, the composite loss (FBMSJointLoss, or
AwesomeImageLoss before or after its extra penalty), d loss / d seg for the backbone, the prior's backward from the activations of
that same pass, Adam / Adamax + enforce_convexity on the row in place.  Nothing syncs with the host.

AwesomeImageLoss with `extra_penalty=True` in the desc, loss = gamma (crit(seg, t) + alpha pcrit(prior, t)) + beta
mean((prior - [seg > 0.5])^2): the prior's step kernel evaluates both of its data terms in the same pass (unaries targets, no
noneclass); `loss[2]` is then the mean align term before beta and `loss[3]` = 1, as inrfit_joint_loss gives them.

`joint_prior_step` (inrfit_joint_prior_step) is the prior's share alone, for the convexity benchmark's losses: the caller evaluates
the segmentation share in torch (any criterion, second-order autograd included) and hands its device scalar over; the call adds
the prior's masked data term and the hard / soft align term, steps the row and returns d(prior's share) / d seg.

`wide_joint_step`, `pcn_wide_joint_step` and `wide_joint_prior_step` are the same three steps for ICNN shapes of the layer-by-layer
path (n_hidden > 130 or more than two hidden layers: inrfit_wide_joint_step / _pcn_wide_joint_step / _wide_joint_prior_step), and
`cdn_wide_joint_step` is `cdn_joint_step` for them (inrfit_cdn_wide_joint_step); the entry points above refuse those shapes, these
refuse the shapes with a fused kernel."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _call as X
from . import _lib as L
from . import icnn as K

Tensor = torch.Tensor


@dataclass
class JointStepResult:
    loss: Tensor                 # [4] device: loss, mean weighted crit(seg), mean penalty / align term, clip factor
    dseg: Tensor                 # [N] d loss / d seg
    prior_logits: Tensor         # [N] the prior's pre-sigmoid output of this step's forward
    status: Tensor               # [1] int32: 1 = non-finite loss, nothing was updated


def joint_desc(kind: str = "bce", weight_mode: str = "sssdms", ratio: float = 1.0, alpha: float = 1.0, beta: float = 1.0,
               clip_penalty: bool = True, form: int = L.JOINT_FBMS, prior_kind: str = "bce", prior_weight_mode: str = "none",
               prior_ratio: float = 1.0, gamma: float = 1.0, extra_penalty: bool = False, n_scribble: int = 0,
               class_targets: bool = False, noneclass=None) -> L.InrJointLossDesc:
    return L.InrJointLossDesc(L.LOSS_KINDS[kind], L.WEIGHT_MODES[weight_mode], float(ratio), float(alpha), float(beta),
                              int(bool(clip_penalty)), int(form), L.LOSS_KINDS[prior_kind], L.WEIGHT_MODES[prior_weight_mode],
                              float(prior_ratio), float(gamma), int(bool(extra_penalty)), int(n_scribble),
                              int(bool(class_targets)), int(noneclass is not None), float(noneclass if noneclass is not None else 0.0))


def _outputs(n: int, dev) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return (L.scratch(4, dtype=torch.float32, device=dev), L.scratch(n, dtype=torch.float32, device=dev),
            L.scratch(n, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))


def _workspace(key, nbytes_fn, dev) -> Tensor:
    """One workspace per (model shape, grid size, device): a joint epoch calls the step thousands of times (X.cached_workspace)."""
    return X.cached_workspace(key, nbytes_fn, dev, refresh_under_poison=True, what="joint step workspace")


def _state(t: Tensor, name: str, numel: int) -> Tensor:
    """An optimizer-state row: updated in place, so it has to be contiguous as it comes."""
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (it is updated in place)")
    return X.flat(t, name, numel)


def _icnn_joint(entry: str, spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
                n_target: int, desc, extra: tuple, od: L.InrOptDesc, step: int, wide: bool = False) -> JointStepResult:
    """inrfit_joint_step / inrfit_joint_prior_step: `extra` is what the entry point takes between its loss desc and its opt desc
    (nothing, or the prior step's checked seg_term / None).
    `wide`: the layer-by-layer entry points and their workspace."""
    K._check_spec(spec)
    dev, n = params.device, grid.n_points
    params, opt_state = X.flat(params, "params", spec.n_params), _state(opt_state, "opt_state", 2 * spec.n_params + L.INR_OPT_HEADER_FLOATS)
    seg, target = X.flat(seg, "seg", n), X.flat(target, "target", n_target)
    X.on_gpu(params=params, opt_state=opt_state, seg=seg, target=target, seg_term=extra[0] if extra else None)
    md, gd = spec._desc, grid._desc
    ws_bytes = getattr(L.load(), "inrfit_wide_joint_step_workspace_bytes" if wide else "inrfit_joint_step_workspace_bytes")
    ws = _workspace(("icnn-wide" if wide else "icnn", spec, n), lambda: ws_bytes(C.byref(md), C.byref(gd)), dev)
    loss, dseg, logits, status = _outputs(n, dev)
    X.call(entry, md, params, opt_state, gd, seg, target, desc, *extra, od, int(step), loss, dseg, logits, status, ws=ws, device=dev)
    return JointStepResult(loss, dseg, logits, status)


def _flow_joint(family: str, ispec: K.IcnnSpec, fspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor,
                flow_opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, od: L.InrOptDesc,
                flow_weight_decay: float, step: int) -> JointStepResult:
    """inrfit_pcn_joint_step / inrfit_cdn_joint_step: `fspec` is the family's flow (RnvpSpec / FlowSpec); families 'pcn_wide' and
    'cdn_wide': inrfit_pcn_wide_joint_step / inrfit_cdn_wide_joint_step, each with its own workspace call."""
    K._check_spec(ispec)
    dev, n = icnn_params.device, grid.n_points
    icnn_params, flow_params = X.flat(icnn_params, "icnn_params", ispec.n_params), X.flat(flow_params, "flow_params", fspec.n_params)
    icnn_opt_state = _state(icnn_opt_state, "icnn_opt_state", 2 * ispec.n_params + L.INR_OPT_HEADER_FLOATS)
    flow_opt_state = _state(flow_opt_state, "flow_opt_state", 2 * fspec.n_params)
    seg, target = X.flat(seg, "seg", n), X.flat(target, "target", n)
    X.on_gpu(icnn_params=icnn_params, flow_params=flow_params, icnn_opt_state=icnn_opt_state, flow_opt_state=flow_opt_state, seg=seg,
             target=target)
    md, fd, gd = ispec._desc, fspec._desc, grid._desc
    lib = L.load()
    if family in ("pcn_wide", "cdn_wide"):
        ws_bytes = getattr(lib, f"inrfit_{family}_joint_step_workspace_bytes")
        ws = _workspace((family, ispec, fspec, n), lambda: ws_bytes(C.byref(md), C.byref(fd), C.byref(gd)), dev)
    else:
        ws_bytes = getattr(lib, f"inrfit_{family}_workspace_bytes")
        ws = _workspace((family, ispec, fspec, n),
                        lambda: ws_bytes(C.byref(md), C.byref(fd), C.byref(gd), 1) + lib.inrfit_joint_loss_workspace_bytes(n) + 4 * n + 1024,
                        dev)
    loss, dseg, logits, status = _outputs(n, dev)
    X.call(f"inrfit_{family}_joint_step", md, fd, icnn_params, flow_params, icnn_opt_state, flow_opt_state, gd, seg, target, desc, od,
           float(flow_weight_decay), int(step), loss, dseg, logits, status, ws=ws, device=dev)
    return JointStepResult(loss, dseg, logits, status)


def joint_step(spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
               desc: L.InrJointLossDesc, step: int, lr: float, optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8,
               weight_decay: float = 0.0, clamp: bool = True) -> JointStepResult:
    """ICNN prior (ConvexNet / ConvexNextNet).  `params` [P] and `opt_state` [2P + 8] are updated IN PLACE."""
    return _icnn_joint("inrfit_joint_step", spec, params, opt_state, grid, seg, target, grid.n_points, desc, (),
                       X.opt_desc(optimizer, lr, betas, eps, weight_decay, clamp), step)


def pcn_joint_step(ispec: K.IcnnSpec, rspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor, flow_opt_state: Tensor,
                   grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, step: int, lr: float,
                   optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8, flow_weight_decay: float = 0.0) -> JointStepResult:
    """PathConnectedNet prior (ICNN behind the RealNVP deformation); every tensor is one row, updated in place."""
    return _flow_joint("pcn", ispec, rspec, icnn_params, flow_params, icnn_opt_state, flow_opt_state, grid, seg, target, desc,
                       X.opt_desc(optimizer, lr, betas, eps, clamp=True), flow_weight_decay, step)


def cdn_joint_step(ispec: K.IcnnSpec, fspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor, flow_opt_state: Tensor,
                   grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, step: int, lr: float,
                   betas=(0.9, 0.999), eps: float = 1e-8, weight_decay_on_weight_g: float = 0.0) -> JointStepResult:
    """ConvexDiffeomorphismNet prior (ICNN behind the weight-normed coupling flow); Adam only, like its pretrain loop."""
    return _flow_joint("cdn", ispec, fspec, icnn_params, flow_params, icnn_opt_state, flow_opt_state, grid, seg, target, desc,
                       X.opt_desc("adam", lr, betas, eps, clamp=True), weight_decay_on_weight_g, step)


def cdn_wide_joint_step(ispec: K.IcnnSpec, fspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor,
                        flow_opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, step: int,
                        lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay_on_weight_g: float = 0.0) -> JointStepResult:
    """`cdn_joint_step` over an ICNN of the layer-by-layer path (inrfit_cdn_wide_joint_step)."""
    return _flow_joint("cdn_wide", ispec, fspec, icnn_params, flow_params, icnn_opt_state, flow_opt_state, grid, seg, target, desc,
                       X.opt_desc("adam", lr, betas, eps, clamp=True), weight_decay_on_weight_g, step)


def joint_prior_desc(kind: str = "bce", weight_mode: str = "none", ratio: float = 1.0, noneclass=None, data_count: int = 0,
                     c_data: float = 1.0, align_rule: int = L.ALIGN_NONE, beta: float = 0.0, align_begin: int = 0) -> L.InrJointPriorDesc:
    return L.InrJointPriorDesc(L.LOSS_KINDS[kind], L.WEIGHT_MODES[weight_mode], float(ratio), int(noneclass is not None),
                               float(noneclass if noneclass is not None else 0.0), int(data_count), float(c_data), int(align_rule),
                               float(beta), int(align_begin))


def joint_prior_step(spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
                     desc: L.InrJointPriorDesc, step: int, lr: float, seg_term: Optional[Tensor] = None, optimizer: str = "adam",
                     betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, clamp: bool = True) -> JointStepResult:
    """ICNN prior, the prior's share only (include/inrfit.h: inrfit_joint_prior_step).  `target` holds desc.data_count values (all
    points when 0); `seg_term` is None or a one-element float32 device tensor, the caller's segmentation share.  `params` [P] and
    `opt_state` [2P + 8] are updated IN PLACE.  loss: composite, data term, mean align term before beta, gradient scale."""
    if seg_term is not None:
        seg_term = X.flat(seg_term, "seg_term", 1)
    return _icnn_joint("inrfit_joint_prior_step", spec, params, opt_state, grid, seg, target,
                       desc.data_count if desc.data_count > 0 else grid.n_points, desc,
                       (seg_term,),
                       X.opt_desc(optimizer, lr, betas, eps, weight_decay, clamp), step)


def wide_joint_step(spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
                    desc: L.InrJointLossDesc, step: int, lr: float, optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8,
                    weight_decay: float = 0.0, clamp: bool = True) -> JointStepResult:
    """`joint_step` for an ICNN of the layer-by-layer path (inrfit_wide_joint_step)."""
    return _icnn_joint("inrfit_wide_joint_step", spec, params, opt_state, grid, seg, target, grid.n_points, desc, (),
                       X.opt_desc(optimizer, lr, betas, eps, weight_decay, clamp), step, wide=True)


def pcn_wide_joint_step(ispec: K.IcnnSpec, rspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor,
                        flow_opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, step: int,
                        lr: float, optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8,
                        flow_weight_decay: float = 0.0) -> JointStepResult:
    """`pcn_joint_step` over an ICNN of the layer-by-layer path (inrfit_pcn_wide_joint_step)."""
    return _flow_joint("pcn_wide", ispec, rspec, icnn_params, flow_params, icnn_opt_state, flow_opt_state, grid, seg, target, desc,
                       X.opt_desc(optimizer, lr, betas, eps, clamp=True), flow_weight_decay, step)


def wide_joint_prior_step(spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
                          desc: L.InrJointPriorDesc, step: int, lr: float, seg_term: Optional[Tensor] = None, optimizer: str = "adam",
                          betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, clamp: bool = True) -> JointStepResult:
    """`joint_prior_step` for an ICNN of the layer-by-layer path (inrfit_wide_joint_prior_step)."""
    if seg_term is not None:
        seg_term = X.flat(seg_term, "seg_term", 1)
    return _icnn_joint("inrfit_wide_joint_prior_step", spec, params, opt_state, grid, seg, target,
                       desc.data_count if desc.data_count > 0 else grid.n_points, desc,
                       (seg_term,),
                       X.opt_desc(optimizer, lr, betas, eps, weight_decay, clamp), step, wide=True)
