"""Host-side driver of the HIP coupling-flow kernels and of the fused ICNN(flow(Ax+b)) fit (include/inrfit.h, flow part).

  flow_forward  <- ConvexDiffeomorphismNet.get_deformation            (awesome/model/convex_diffeomorphism_net.py:179-184)
  cdn_forward   <- ConvexDiffeomorphismNet.forward                    (:173-178)
  cdn_loss_grad <- criterion(sigmoid(model(grid)), unaries).backward()  w.r.t. every parameter
  cdn_fit       <- the inner loop of ConvexDiffeomorphismNet.pretrain (:405-430)

The ICNN may be a fused shape or one of the layer-by-layer path (n_hidden > 130 or more than two hidden layers): the same calls take
both, and inrfit_cdn_workspace_bytes sizes the workspace of either.  `cdn_wide_joint_step` is the fused joint step of the second kind
(inrfit_cdn_wide_joint_step; the fused shapes' is `awesome_amd.joint.cdn_joint_step`).
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import cached_property
from typing import Dict, List, Optional, Tuple

import torch

from . import _call as X
from . import _lib as L
from . import icnn as K

Tensor = torch.Tensor


@dataclass(frozen=True)
class FlowSpec:
    width: int = 130
    num_coupling: int = 6
    backbone: str = "normal_block"   # 'normal_block' (= 'residual_block') | 'default' (SimpleBackbone), diffeomorphism_net.py:252-268

    def desc(self) -> L.InrFlowDesc:
        return L.InrFlowDesc(self.width, self.num_coupling, L.INR_FLOW_SIMPLE if self.backbone == "default" else L.INR_FLOW_NORMAL_BLOCK)

    @cached_property
    def _desc(self) -> L.InrFlowDesc:      # for the wrappers, once per spec (never written to)
        return self.desc()

    @cached_property
    def n_params(self) -> int:
        return 6 + 2 * self.num_coupling * (3 * self.width + 3) + 4 * self.num_coupling

    def keys_shapes(self, prefix: str = "diffeo_net.", linear_prefix: str = "linear.") -> List[Tuple[str, Tuple[int, ...]]]:
        """state_dict keys of ConvexDiffeomorphismNet's flow part in flat-vector order."""
        W, out = self.width, [(linear_prefix + "weight", (2, 2)), (linear_prefix + "bias", (2,))]
        l1, l2 = ("linear1", "linear2") if self.backbone == "default" else ("in_linear", "out_linear")
        for i in range(self.num_coupling):
            for net in ("s", "t"):
                b = f"{prefix}{net}.{i}."
                out += [(b + l1 + ".linear.weight_v", (W, 1)), (b + l1 + ".linear.weight_g", ()),
                        (b + l1 + ".linear.bias", (W,)), (b + l2 + ".linear.weight_v", (1, W)),
                        (b + l2 + ".linear.weight_g", ()), (b + l2 + ".linear.bias", (1,))]
        for i in range(self.num_coupling):
            b = f"{prefix}scale.{i}."
            out += [(b + "weight", (1,)), (b + "scale.bias", (1,)), (b + "scale.weight_g", (1, 1)), (b + "scale.weight_v", (1, 1))]
        return out

    def weight_g_mask(self) -> Tensor:
        """1 where the flat flow parameter is a *weight_g (the group that gets weight decay, awesome/util/torch.py:19-35)."""
        parts = []
        for k, shp in self.keys_shapes():
            n = 1
            for s in shp:
                n *= s
            parts.append(torch.full((n,), 1.0 if k.endswith("weight_g") else 0.0))
        return torch.cat(parts)


def pack_flow_state_dict(spec: FlowSpec, sd: Dict[str, Tensor], device=None) -> Tensor:
    parts = []
    for k, shp in spec.keys_shapes():
        t = sd[k]
        if tuple(t.shape) != shp:
            raise ValueError(f"{k}: expected shape {shp}, got {tuple(t.shape)}")
        parts.append(t.detach().reshape(-1).to(torch.float32))
    flat = torch.cat(parts)
    return flat.to(device) if device is not None else flat


def unpack_flow_params(spec: FlowSpec, flat: Tensor) -> Dict[str, Tensor]:
    flat = flat.detach().reshape(-1).clone()
    out, off = {}, 0
    for k, shp in spec.keys_shapes():
        n = 1
        for s in shp:
            n *= s
        out[k] = flat[off:off + n].reshape(shp)
        off += n
    return out


def split_cdn_state_dict(ispec: K.IcnnSpec, fspec: FlowSpec, sd: Dict[str, Tensor], device=None) -> Tuple[Tensor, Tensor]:
    """ConvexDiffeomorphismNet.state_dict() -> (flat ICNN params, flat flow params)."""
    icnn_sd = {k[len("convex_net."):]: v for k, v in sd.items() if k.startswith("convex_net.")}
    return K.pack_state_dict(ispec, icnn_sd, device), pack_flow_state_dict(fspec, sd, device)


def merge_cdn_state_dict(ispec: K.IcnnSpec, fspec: FlowSpec, icnn_flat: Tensor, flow_flat: Tensor) -> Dict[str, Tensor]:
    sd = {"convex_net." + k: v for k, v in K.unpack_params(ispec, icnn_flat).items()}
    sd.update(unpack_flow_params(fspec, flow_flat))
    return sd


def _ws(ispec: Optional[K.IcnnSpec], fspec: FlowSpec, grid: K.Grid, n_images: int) -> Tensor:
    return X.workspace("inrfit_cdn_workspace_bytes", ispec._desc if ispec is not None else None, fspec._desc, grid._desc, n_images,
                       device=grid.device)


def _params(ispec: K.IcnnSpec, fspec: FlowSpec, icnn_params: Tensor, flow_params: Tensor) -> Tuple[Tensor, Tensor, int]:
    """icnn_params [n_images, P] and flow_params [n_images, FP], checked against their specs."""
    K._check_spec(ispec)
    ip = X.rows(icnn_params, "icnn_params", None, ispec.n_params)
    return ip, X.rows(flow_params, "flow_params", ip.shape[0], fspec.n_params), ip.shape[0]


def flow_forward(fspec: FlowSpec, flow_params: Tensor, grid: K.Grid) -> Tensor:
    """flow_params [n_images, FP] -> deformed coordinates [n_images, 2, N]."""
    fp = X.rows(flow_params, "flow_params", None, fspec.n_params)
    X.on_gpu(flow_params=fp)
    n = fp.shape[0]
    out = L.scratch(n, 2, grid.n_points, dtype=torch.float32, device=fp.device)
    X.call("inrfit_flow_forward", fspec._desc, fp, grid._desc, n, out, ws=_ws(None, fspec, grid, n), device=fp.device)
    return out


def flow_backward(fspec: FlowSpec, flow_params: Tensor, grid: K.Grid, dout_coords: Tensor) -> Tensor:
    """Vector-Jacobian product of flow_forward: dout_coords [n_images, 2, N] -> gradients [n_images, FP] (forward recomputed)."""
    fp = X.rows(flow_params, "flow_params", None, fspec.n_params)
    n = fp.shape[0]
    d = X.rows(dout_coords, "dout_coords", n, (2, grid.n_points))
    X.on_gpu(flow_params=fp, dout_coords=d)
    grads = L.scratch_like(fp)
    X.call("inrfit_flow_backward", fspec._desc, fp, grid._desc, d, n, grads, ws=_ws(None, fspec, grid, n), device=fp.device)
    return grads


def cdn_forward(ispec: K.IcnnSpec, fspec: FlowSpec, icnn_params: Tensor, flow_params: Tensor, grid: K.Grid) -> Tensor:
    ip, fp, n = _params(ispec, fspec, icnn_params, flow_params)
    X.on_gpu(icnn_params=ip, flow_params=fp)
    logits = L.scratch(n, grid.n_points, dtype=torch.float32, device=ip.device)
    X.call("inrfit_cdn_forward", ispec._desc, fspec._desc, ip, fp, grid._desc, n, logits, ws=_ws(ispec, fspec, grid, n),
           device=ip.device)
    return logits


def cdn_loss_grad(ispec: K.IcnnSpec, fspec: FlowSpec, icnn_params: Tensor, flow_params: Tensor, grid: K.Grid, targets: Tensor,
                  loss: str = "bce", weight_mode: str = "none", ratio: float = 1.0) -> Tuple[Tensor, Tensor, Tensor]:
    ip, fp, n = _params(ispec, fspec, icnn_params, flow_params)
    targets = K._per_point(ispec, targets, "targets", n, grid)
    X.on_gpu(icnn_params=ip, flow_params=fp, targets=targets)
    lo = L.scratch(n, dtype=torch.float32, device=ip.device)
    gi, gf = L.scratch_like(ip), L.scratch_like(fp)
    X.call("inrfit_cdn_loss_grad", ispec._desc, fspec._desc, ip, fp, grid._desc, targets, X.loss_desc(loss, weight_mode, ratio, 0.0, 0.0),
           n, lo, gi, gf, ws=_ws(ispec, fspec, grid, n), device=ip.device)
    return lo, gi, gf


@dataclass
class CdnFitResult:
    icnn_params: Tensor
    flow_params: Tensor
    icnn_opt_state: Tensor
    flow_opt_state: Tensor
    loss_hist: Optional[Tensor]
    logits: Optional[Tensor]
    status: Tensor


def cdn_fit(ispec: K.IcnnSpec, fspec: FlowSpec, icnn_params: Tensor, flow_params: Tensor, grid: K.Grid, targets: Tensor,
            steps: int, lr: float = 3e-3, loss: str = "bce", weight_mode: str = "none", ratio: float = 1.0,
            weight_decay_on_weight_g: float = 5e-5, betas=(0.9, 0.999), eps: float = 1e-8, plateau: Optional[dict] = None,
            icnn_opt_state: Optional[Tensor] = None, flow_opt_state: Optional[Tensor] = None, step0: int = 0,
            record_loss: bool = True, want_logits: bool = True, gate_logits: bool = False, clamp: bool = True,
            c_fg: float = 0.0, c_bg: float = 0.0) -> CdnFitResult:
    """ConvexDiffeomorphismNet.pretrain's inner loop on the device (defaults: Adam lr 3e-3, BCE, wd 5e-5 on weight_g, the ICNN's
    projection after every step; c_fg / c_bg: the coefficients of weight_mode 'explicit')."""
    ip, fp, n = _params(ispec, fspec, icnn_params, flow_params)
    dev = ip.device
    targets = K._per_point(ispec, targets, "targets", n, grid)
    icnn_opt_state, flow_opt_state = K._opt_states(ispec, fspec.n_params, n, dev, icnn_opt_state, flow_opt_state)
    X.on_gpu(icnn_params=ip, flow_params=fp, targets=targets, icnn_opt_state=icnn_opt_state, flow_opt_state=flow_opt_state)
    hist, logits, status = X.fit_outputs(n, steps, (n, grid.n_points), record_loss, want_logits, dev)
    od = X.opt_desc("adam", lr, betas, eps, clamp=clamp, plateau=plateau, gate_logits=gate_logits)
    X.call("inrfit_cdn_fit", ispec._desc, fspec._desc, ip, fp, icnn_opt_state, flow_opt_state, grid._desc, targets,
           X.loss_desc(loss, weight_mode, ratio, c_fg, c_bg), od, float(weight_decay_on_weight_g), n, int(steps), int(step0), hist, logits,
           status, ws=_ws(ispec, fspec, grid, n), device=dev)
    return CdnFitResult(ip, fp, icnn_opt_state, flow_opt_state, X.trim(hist, steps), logits, status)


def cdn_wide_joint_step(ispec: K.IcnnSpec, fspec: FlowSpec, icnn_params: Tensor, flow_params: Tensor, icnn_opt_state: Tensor,
                        flow_opt_state: Tensor, grid: K.Grid, seg: Tensor, target: Tensor, desc, step: int, lr: float,
                        betas=(0.9, 0.999), eps: float = 1e-8, weight_decay_on_weight_g: float = 0.0):
    """One fused joint-training step of ICNN(flow(Ax + b)) over an ICNN of the layer-by-layer path, one image, every row updated in
    place (inrfit_cdn_wide_joint_step through awesome_amd.joint's call path) -> JointStepResult."""
    from . import joint as J
    return J.cdn_wide_joint_step(ispec, fspec, icnn_params, flow_params, icnn_opt_state, flow_opt_state, grid, seg, target, desc, step,
                                 lr, betas=betas, eps=eps, weight_decay_on_weight_g=weight_decay_on_weight_g)
