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
path (n_hidden > 130 or more than two hidden layers: inrfit_wide_joint_step / _pcn_wide_joint_step / _wide_joint_prior_step); the
entry points above refuse those shapes, these refuse the shapes with a fused kernel."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

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


def _opt_desc(optimizer: str, lr: float, betas, eps: float, weight_decay: float, clamp: bool) -> L.InrOptDesc:
    return L.InrOptDesc(L.OPT_KINDS[optimizer], float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                        int(bool(clamp)), 0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0, 0)


def _outputs(n: int, dev) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return (L.scratch(4, dtype=torch.float32, device=dev), L.scratch(n, dtype=torch.float32, device=dev),
            L.scratch(n, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))


_ws_cache = {}


def _workspace(key, nbytes_fn, dev) -> Tensor:
    """One workspace per (model shape, grid size, device): a joint epoch calls the step thousands of times.  Every call here
    writes all of its workspace before it reads it, so under L.POISON a fresh NaN-filled one per call is the check that it does;
    the segmentation networks' cache (_segnet.SegDriver.workspace) carries state between two calls and must not do that."""
    k = (key, str(dev))
    ws = _ws_cache.get(k)
    if ws is None or L.POISON:
        nbytes = int(nbytes_fn())
        if nbytes < 0:
            L.check(nbytes, "joint step workspace")
        ws = L.scratch(nbytes // 4 + 64, dtype=torch.float32, device=dev)
        _ws_cache[k] = ws
    return ws


def _icnn_joint(entry: str, spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
                n_target: int, desc, extra: tuple, od: L.InrOptDesc, step: int, wide: bool = False) -> JointStepResult:
    """inrfit_joint_step / inrfit_joint_prior_step: `extra` is what the entry point takes between its loss desc and its opt desc.
    `wide`: the layer-by-layer entry points and their workspace."""
    params, seg, target = K._check_dev(params, "params"), K._check_dev(seg, "seg"), K._check_dev(target, "target")
    dev, n = params.device, grid.n_points
    assert params.numel() == spec.n_params and seg.numel() == n and target.numel() == n_target
    assert opt_state.numel() == 2 * spec.n_params + L.INR_OPT_HEADER_FLOATS and opt_state.is_contiguous()
    md, gd = spec.desc(), grid.desc()
    lib = L.load()
    ws_bytes = lib.inrfit_wide_joint_step_workspace_bytes if wide else lib.inrfit_joint_step_workspace_bytes
    ws = _workspace(("icnn-wide" if wide else "icnn", spec, n), lambda: ws_bytes(C.byref(md), C.byref(gd)), dev)
    loss, dseg, logits, status = _outputs(n, dev)
    rc = getattr(lib, entry)(C.byref(md), params.data_ptr(), opt_state.data_ptr(), C.byref(gd), seg.data_ptr(), target.data_ptr(),
                             C.byref(desc), *extra, C.byref(od), int(step), loss.data_ptr(), dseg.data_ptr(), logits.data_ptr(),
                             status.data_ptr(), ws.data_ptr(), ws.numel() * 4, K._stream_ptr(dev))
    L.check(rc, entry)
    return JointStepResult(loss, dseg, logits, status)


def _flow_joint(family: str, ispec: K.IcnnSpec, fspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor,
                flow_opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, od: L.InrOptDesc,
                flow_weight_decay: float, step: int) -> JointStepResult:
    """inrfit_pcn_joint_step / inrfit_cdn_joint_step: `fspec` is the family's flow (RnvpSpec / FlowSpec); family 'pcn_wide':
    inrfit_pcn_wide_joint_step with its own workspace call."""
    dev, n = icnn_params.device, grid.n_points
    md, fd, gd = ispec.desc(), fspec.desc(), grid.desc()
    lib = L.load()
    if family == "pcn_wide":
        ws = _workspace((family, ispec, fspec, n),
                        lambda: lib.inrfit_pcn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(fd), C.byref(gd)), dev)
    else:
        ws_bytes = getattr(lib, f"inrfit_{family}_workspace_bytes")
        ws = _workspace((family, ispec, fspec, n),
                        lambda: ws_bytes(C.byref(md), C.byref(fd), C.byref(gd), 1) + lib.inrfit_joint_loss_workspace_bytes(n) + 4 * n + 1024,
                        dev)
    loss, dseg, logits, status = _outputs(n, dev)
    entry = f"inrfit_{family}_joint_step"
    rc = getattr(lib, entry)(C.byref(md), C.byref(fd), icnn_params.data_ptr(), flow_params.data_ptr(), icnn_opt_state.data_ptr(),
                             flow_opt_state.data_ptr(), C.byref(gd), seg.data_ptr(), target.data_ptr(), C.byref(desc), C.byref(od),
                             float(flow_weight_decay), int(step), loss.data_ptr(), dseg.data_ptr(), logits.data_ptr(),
                             status.data_ptr(), ws.data_ptr(), ws.numel() * 4, K._stream_ptr(dev))
    L.check(rc, entry)
    return JointStepResult(loss, dseg, logits, status)


def joint_step(spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
               desc: L.InrJointLossDesc, step: int, lr: float, optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8,
               weight_decay: float = 0.0, clamp: bool = True) -> JointStepResult:
    """ICNN prior (ConvexNet / ConvexNextNet).  `params` [P] and `opt_state` [2P + 8] are updated IN PLACE."""
    return _icnn_joint("inrfit_joint_step", spec, params, opt_state, grid, seg, target, grid.n_points, desc, (),
                       _opt_desc(optimizer, lr, betas, eps, weight_decay, clamp), step)


def pcn_joint_step(ispec: K.IcnnSpec, rspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor, flow_opt_state: Tensor,
                   grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, step: int, lr: float,
                   optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8, flow_weight_decay: float = 0.0) -> JointStepResult:
    """PathConnectedNet prior (ICNN behind the RealNVP deformation); every tensor is one row, updated in place."""
    return _flow_joint("pcn", ispec, rspec, icnn_params, flow_params, icnn_opt_state, flow_opt_state, grid, seg, target, desc,
                       _opt_desc(optimizer, lr, betas, eps, 0.0, True), flow_weight_decay, step)


def cdn_joint_step(ispec: K.IcnnSpec, fspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor, flow_opt_state: Tensor,
                   grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, step: int, lr: float,
                   betas=(0.9, 0.999), eps: float = 1e-8, weight_decay_on_weight_g: float = 0.0) -> JointStepResult:
    """ConvexDiffeomorphismNet prior (ICNN behind the weight-normed coupling flow); Adam only, like its pretrain loop."""
    return _flow_joint("cdn", ispec, fspec, icnn_params, flow_params, icnn_opt_state, flow_opt_state, grid, seg, target, desc,
                       _opt_desc("adam", lr, betas, eps, 0.0, True), weight_decay_on_weight_g, step)


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
        seg_term = K._check_dev(seg_term, "seg_term")
        assert seg_term.numel() == 1
    return _icnn_joint("inrfit_joint_prior_step", spec, params, opt_state, grid, seg, target,
                       desc.data_count if desc.data_count > 0 else grid.n_points, desc,
                       (None if seg_term is None else seg_term.data_ptr(),),
                       _opt_desc(optimizer, lr, betas, eps, weight_decay, clamp), step)


def wide_joint_step(spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
                    desc: L.InrJointLossDesc, step: int, lr: float, optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8,
                    weight_decay: float = 0.0, clamp: bool = True) -> JointStepResult:
    """`joint_step` for an ICNN of the layer-by-layer path (inrfit_wide_joint_step)."""
    return _icnn_joint("inrfit_wide_joint_step", spec, params, opt_state, grid, seg, target, grid.n_points, desc, (),
                       _opt_desc(optimizer, lr, betas, eps, weight_decay, clamp), step, wide=True)


def pcn_wide_joint_step(ispec: K.IcnnSpec, rspec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor,
                        flow_opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor, desc: L.InrJointLossDesc, step: int,
                        lr: float, optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8,
                        flow_weight_decay: float = 0.0) -> JointStepResult:
    """`pcn_joint_step` over an ICNN of the layer-by-layer path (inrfit_pcn_wide_joint_step)."""
    return _flow_joint("pcn_wide", ispec, rspec, icnn_params, flow_params, icnn_opt_state, flow_opt_state, grid, seg, target, desc,
                       _opt_desc(optimizer, lr, betas, eps, 0.0, True), flow_weight_decay, step)


def wide_joint_prior_step(spec: K.IcnnSpec, params: Tensor, opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor,
                          desc: L.InrJointPriorDesc, step: int, lr: float, seg_term: Optional[Tensor] = None, optimizer: str = "adam",
                          betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, clamp: bool = True) -> JointStepResult:
    """`joint_prior_step` for an ICNN of the layer-by-layer path (inrfit_wide_joint_prior_step)."""
    if seg_term is not None:
        seg_term = K._check_dev(seg_term, "seg_term")
        assert seg_term.numel() == 1
    return _icnn_joint("inrfit_wide_joint_prior_step", spec, params, opt_state, grid, seg, target,
                       desc.data_count if desc.data_count > 0 else grid.n_points, desc,
                       (None if seg_term is None else seg_term.data_ptr(),),
                       _opt_desc(optimizer, lr, betas, eps, weight_decay, clamp), step, wide=True)
