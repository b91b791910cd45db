"""Host side of the star-shape prior's device-resident entry points (include/inrfit.h: inrfit_star_forward / _loss_grad / _fit, and
the dense full-batch, many-image form inrfit_star_fit_dense / _loss_grad_dense; kernels in csrc/star.h).  Mirrors
notebooks/icml_teaser_code/star_shaped/star.ipynb: `myNet` (cell 2) and its training loop (cell 3).

Parameters travel as ONE flat vector in the order of the notebook class's named_parameters() (PARAM_ORDER)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _call as X
from . import _lib as L

Tensor = torch.Tensor

PARAM_ORDER = ("offset", "W0.weight", "W0.bias", "W1.weight", "W1.bias", "W2.weight", "W2.bias", "W1_r.weight", "W1_r.bias",
               "W2_r.weight", "W2_r.bias")
MAX_BATCH = 1 << 16


@dataclass(frozen=True)
class StarSpec:
    n_hidden: int

    def desc(self) -> L.InrStarDesc:
        return L.InrStarDesc(int(self.n_hidden))

    @property
    def shapes(self) -> Dict[str, Tuple[int, ...]]:
        h = self.n_hidden
        return {"offset": (1, 2), "W0.weight": (h, 2), "W0.bias": (h,), "W1.weight": (h, h), "W1.bias": (h,), "W2.weight": (1, h),
                "W2.bias": (1,), "W1_r.weight": (h, 1), "W1_r.bias": (h,), "W2_r.weight": (1, h), "W2_r.bias": (1,)}

    @property
    def n_params(self) -> int:
        h = self.n_hidden
        return h * h + 8 * h + 4


def flatten_state_dict(spec: StarSpec, sd: Dict[str, Tensor], device) -> Tensor:
    """state_dict of the notebook class (or of StarShapedNet) -> [P] float32 on `device`."""
    parts = []
    for k, shape in spec.shapes.items():
        v = sd[k].detach().to(torch.float32)
        if tuple(v.shape) != shape:
            raise ValueError(f"{k}: expected {shape}, got {tuple(v.shape)}")
        parts.append(v.reshape(-1))
    return torch.cat(parts).to(device).contiguous()


def unflatten(spec: StarSpec, flat: Tensor) -> Dict[str, Tensor]:
    out, o = {}, 0
    for k, shape in spec.shapes.items():
        n = 1
        for s in shape:
            n *= s
        out[k] = flat[o:o + n].reshape(shape).clone()
        o += n
    return out


def _workspace(spec: StarSpec, n_points: int, dev) -> Tensor:
    return X.workspace("inrfit_star_workspace_bytes", spec.desc(), int(n_points), device=dev, slack=64)


def _check(params: Tensor, spec: StarSpec, coords: Tensor, labels: Optional[Tensor] = None):
    if not params.is_contiguous():
        raise ValueError("params must be one contiguous flat vector (it is updated in place)")
    params = X.flat(params, "params", spec.n_params)
    coords = X.rows(coords, "coords", None, 2)                  # (n_pixels, 2)
    if labels is not None:
        labels = X.flat(labels, "labels", coords.shape[0])      # one per pixel
    return params, coords, labels


def star_forward(spec: StarSpec, params: Tensor, coords: Tensor) -> Tensor:
    """logits [n] of every row of coords [n, 2] (cell 4 / 6 of the notebook: inference on all pixels)."""
    params, coords, _ = _check(params, spec, coords)
    X.on_gpu(params=params, coords=coords)
    n, dev = coords.shape[0], params.device
    out = L.scratch(n, dtype=torch.float32, device=dev)
    X.call("inrfit_star_forward", spec.desc(), params, coords, n, out, ws=_workspace(spec, n, dev), device=dev)
    return out


def star_loss_grad(spec: StarSpec, params: Tensor, coords: Tensor, labels: Tensor, index: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(loss [1], grads [P]) of MSE(sigmoid(net(coords[index])), labels[index]); index None = every pixel."""
    params, coords, labels = _check(params, spec, coords, labels)
    X.on_gpu(params=params, coords=coords, labels=labels)
    dev, npx = params.device, coords.shape[0]
    if index is not None:
        index = index.to(device=dev, dtype=torch.int32).contiguous()
    batch = int(index.numel()) if index is not None else npx
    loss = L.scratch(1, dtype=torch.float32, device=dev)
    grads = L.scratch(spec.n_params, dtype=torch.float32, device=dev)
    X.call("inrfit_star_loss_grad", spec.desc(), params, coords, labels, npx, index, batch, loss, grads, ws=_workspace(spec, batch, dev),
           device=dev)
    return loss, grads


@dataclass
class StarFitResult:
    params: Tensor              # [P], same storage as the input
    opt_state: Tensor           # [2P] exp_avg | exp_avg_sq
    loss_hist: Optional[Tensor]  # [steps]


def star_fit(spec: StarSpec, params: Tensor, coords: Tensor, labels: Tensor, batch_index: Tensor, lr: float = 1e-2,
             betas=(0.9, 0.999), eps: float = 1e-8, step0: int = 0, offset_first_step: int = 1001,
             opt_state: Optional[Tensor] = None, record_loss: bool = True) -> StarFitResult:
    """The loop of star.ipynb cell 3 on the device: epoch e = step0 + k takes the minibatch batch_index[k] ([steps, batch] pixel numbers),
    Adam(lr) on every parameter IN PLACE, then W2_r.weight <- relu(W2_r.weight).  `offset` takes its first step at epoch
    offset_first_step (the notebook: requires_grad after the forward of epoch 1000 -> 1001; < 0: never)."""
    params, coords, labels = _check(params, spec, coords, labels)
    dev, npx = params.device, coords.shape[0]
    if batch_index.dim() != 2:
        raise ValueError("batch_index: expected (steps, batch)")
    steps, batch = int(batch_index.shape[0]), int(batch_index.shape[1])
    if batch < 1 or batch > MAX_BATCH:
        raise ValueError(f"batch must be in [1, {MAX_BATCH}]")
    if opt_state is None:
        opt_state = torch.zeros(2 * spec.n_params, dtype=torch.float32, device=dev)
    if not opt_state.is_contiguous() or opt_state.device != dev:
        raise ValueError("opt_state must be contiguous (it is updated in place) and live on the parameters' device")
    opt_state = X.flat(opt_state, "opt_state", 2 * spec.n_params)
    X.on_gpu(params=params, coords=coords, labels=labels, opt_state=opt_state)
    batch_index = batch_index.to(device=dev, dtype=torch.int32).contiguous()
    hist = L.scratch(max(steps, 1), dtype=torch.float32, device=dev) if record_loss else None
    X.call("inrfit_star_fit", spec.desc(), params, opt_state, coords, labels, npx, batch_index, batch, X.opt_desc("adam", lr, betas, eps),
           steps, int(step0), int(offset_first_step), hist, ws=_workspace(spec, batch, dev), device=dev)
    return StarFitResult(params, opt_state, X.trim(hist, steps))


# ---- the dense full-batch form (inrfit_star_fit_dense / _loss_grad_dense) -------------------------------------------------------------
def dense_tile_points() -> int:
    """Points per tile of the dense entry points: a constant of the library (it fixes the order of the sums)."""
    return int(L.load().inrfit_star_dense_tile_points())


def opt_state_floats(spec: StarSpec) -> int:
    return 2 * spec.n_params + L.INR_OPT_HEADER_FLOATS


def new_dense_opt_state(spec: StarSpec, n_images: int, device) -> Tensor:
    """Zeroed: a cold fit (moments 0; step0 == 0 fills the header)."""
    return torch.zeros(n_images, opt_state_floats(spec), dtype=torch.float32, device=device)


def _check_dense(spec: StarSpec, params: Tensor, coords: Tensor, targets: Tensor):
    """params [n, P]; coords [N, 2] (one grid for all images) or [n, N, 2]; targets [n, N] -> (..., n, N, coords' image stride)."""
    if params.dim() != 2:
        raise ValueError("params must be [n_images, P]")
    if not params.is_contiguous():
        raise ValueError("params must be contiguous (they are updated in place)")
    n = int(params.shape[0])
    params = X.rows(params, "params", n, spec.n_params)
    if coords.dim() == 3:
        coords = X.rows(coords, "coords", n, (int(coords.shape[1]), 2))
        npx = int(coords.shape[1])
        stride = 2 * npx
    else:
        coords = X.rows(coords, "coords", None, 2)
        npx, stride = int(coords.shape[0]), 0
    targets = X.rows(targets, "targets", n, npx)
    return params, coords, targets, n, npx, stride


@dataclass
class StarDenseFitResult:
    params: Tensor               # [n, P], same storage as the input
    opt_state: Tensor            # [n, 2P + header]
    loss_hist: Optional[Tensor]  # [n, steps]: the loss before each step
    logits: Optional[Tensor]     # [n, N]
    status: Tensor               # [n] int32, INR_STATUS_*


def star_fit_dense(spec: StarSpec, params: Tensor, coords: Tensor, targets: Tensor, steps: int, lr: float = 1e-2, loss: str = "se",
                   weight_mode: str = "none", ratio: float = 1.0, c_fg: float = 0.0, c_bg: float = 0.0, optimizer: str = "adam",
                   betas=(0.9, 0.999), eps: float = 1e-8, plateau: Optional[dict] = None, opt_state: Optional[Tensor] = None,
                   step0: int = 0, offset_first_step: int = 0, record_loss: bool = True, want_logits: bool = True,
                   gate_logits: bool = False, weight_decay: float = 0.0) -> StarDenseFitResult:
    """`steps` full-batch steps of n independent star-shape fits on the device (params IN PLACE): criterion(sigmoid(net), targets)
    as the ICNN fits read it, Adam / Adamax, W2_r.weight <- relu, ReduceLROnPlateau (`plateau`: None = off).  The centre takes its
    first step at step `offset_first_step` (< 0: never).  gate_logits: `logits` = the output of the last training forward (what the
    IoU gate reads) instead of the logits at the final parameters.  Continue a fit by handing `opt_state` back with `step0`."""
    params, coords, targets, n, npx, stride = _check_dense(spec, params, coords, targets)
    dev = params.device
    if opt_state is None:
        opt_state = new_dense_opt_state(spec, n, dev)
    if not opt_state.is_contiguous():
        raise ValueError("opt_state must be contiguous (it is updated in place)")
    opt_state = X.rows(opt_state, "opt_state", n, opt_state_floats(spec))
    X.on_gpu(params=params, coords=coords, targets=targets, opt_state=opt_state)
    ws = X.workspace("inrfit_star_dense_workspace_bytes", spec.desc(), npx, n, device=dev, slack=64)
    hist, logits, status = X.fit_outputs(n, steps, (n, npx), record_loss, want_logits, dev)
    od = X.opt_desc(optimizer, lr, betas, eps, weight_decay, plateau=plateau, gate_logits=gate_logits)
    X.call("inrfit_star_fit_dense", spec.desc(), params, opt_state, coords, stride, targets, X.loss_desc(loss, weight_mode, ratio, c_fg, c_bg),
           od, npx, n, int(steps), int(step0), int(offset_first_step), hist, logits, status, ws=ws, device=dev)
    return StarDenseFitResult(params, opt_state, X.trim(hist, steps), logits, status)


def star_loss_grad_dense(spec: StarSpec, params: Tensor, coords: Tensor, targets: Tensor, loss: str = "se", weight_mode: str = "none",
                         ratio: float = 1.0, c_fg: float = 0.0, c_bg: float = 0.0) -> Tuple[Tensor, Tensor]:
    """(loss [n], grads [n, P]) of the dense criterion at `params`, every pixel, any number of them."""
    params, coords, targets, n, npx, stride = _check_dense(spec, params, coords, targets)
    X.on_gpu(params=params, coords=coords, targets=targets)
    dev = params.device
    ws = X.workspace("inrfit_star_dense_workspace_bytes", spec.desc(), npx, n, device=dev, slack=64)
    loss_out = L.scratch(n, dtype=torch.float32, device=dev)
    grads = L.scratch(n, spec.n_params, dtype=torch.float32, device=dev)
    X.call("inrfit_star_loss_grad_dense", spec.desc(), params, coords, stride, targets, X.loss_desc(loss, weight_mode, ratio, c_fg, c_bg),
           npx, n, loss_out, grads, ws=ws, device=dev)
    return loss_out, grads


def notebook_minibatches(labels: Tensor, steps: int, number: int = 500, generator: Optional[torch.Generator] = None,
                         chunk: int = 64) -> Tensor:
    """[steps, 2 * number] pixel numbers: per epoch `number` random background pixels (label > 0.5: cell 3's labels = 1 - likelihood)
    followed by `number` random foreground pixels, each a uniformly random subset without repetition - what
    `torch.randperm(n)[:number]` of cell 3 draws.  Random keys + top-k on the device, `chunk` epochs at a time."""
    from .minibatch import draw_class_batches
    back = torch.nonzero(labels.reshape(-1) > 0.5).reshape(-1)
    fore = torch.nonzero(labels.reshape(-1) <= 0.5).reshape(-1)
    return draw_class_batches(back, fore, steps, number, generator, chunk)
