"""Rotation / mirror-symmetry prior of the teaser on the device: pose and network trained together (include/inrfit.h: inrfit_sym_*,
csrc/sym.h).  Mirrors notebooks/icml_teaser_code/rotation_symmetric/rotation_symmetric.ipynb: `myNet` (cell 2) and its training loop
(cell 3: 10 000 epochs of 500 + 500 random pixels, 2 MSE(bg) + 1 MSE(fg), ONE Adam over pose and network, `symmetry_prior` switched on
once training has started).

The network is an `IcnnSpec(h, 3, 1)` run as an unconstrained MLP (clamp = False, freeze_skips = True); the pose is three numbers per
image, `pose [n_images, 3]` = offset[2] | orientation, with `pose_opt_state [n_images, 6]` = exp_avg[3] | exp_avg_sq[3].  `sym_fit` /
`sym_fit_minibatch` update params, pose and both optimizer states IN PLACE; step k of `sym_fit_minibatch` launches exactly what
`sym_fit(steps=1, step0=step0 + k)` launches on the gathered rows, so a finite run ends bit for bit where the per-step loop ends."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _call as X
from . import _lib as L
from . import icnn as K
from . import minibatch as MB

Tensor = torch.Tensor
R_EPS = 0.001   # the notebook's x / (0.001 + r)


@dataclass
class SymFitResult:
    params: Tensor             # [n_images, P]
    pose: Tensor               # [n_images, 3]
    opt_state: Tensor
    pose_opt_state: Tensor     # [n_images, 6]
    loss_hist: Optional[Tensor]
    status: Tensor


def _check(spec: K.IcnnSpec, params: Tensor, pose: Tensor) -> Tuple[Tensor, Tensor, int]:
    K._check_spec(spec)
    if spec.in_features != 3 or spec.n_out != 1:
        raise ValueError("the network behind the pose reads the 3 features (u, v, r) and has one output")
    params = X.rows(params, "params", None, spec.n_params)
    return params, X.rows(pose, "pose", params.shape[0], 3), int(params.shape[0])   # pose: offset[2] | orientation


def _grid(grid: K.Grid) -> K.Grid:
    if grid.mode == L.INR_GRID_EXPLICIT and int(grid.coords.shape[-2]) != 2:
        raise ValueError("the pose reads a 2-channel grid")
    return grid


def _ws(spec: K.IcnnSpec, grid: K.Grid, n_images: int) -> Tensor:
    return X.workspace("inrfit_sym_workspace_bytes", spec._desc, grid._desc, n_images, device=grid.device)


def _sym_desc(symmetry_from_step: int, r_eps: float) -> L.InrSymDesc:
    return L.InrSymDesc(int(symmetry_from_step), float(r_eps))


def new_pose_opt_state(n_images: int, device) -> Tensor:
    return torch.zeros(n_images, 6, dtype=torch.float32, device=device)


def sym_forward(spec: K.IcnnSpec, params: Tensor, pose: Tensor, grid: K.Grid, symmetry_prior: bool = True, r_eps: float = R_EPS) -> Tensor:
    """logits [n_images, N] of pose + network on the 2-channel grid, with or without the mirror."""
    params, pose, n = _check(spec, params, pose)
    grid = _grid(grid)
    X.on_gpu(params=params, pose=pose)
    logits = L.scratch(n, grid.n_points, dtype=torch.float32, device=params.device)
    X.call("inrfit_sym_forward", spec._desc, _sym_desc(-1, r_eps), params, pose, grid._desc, n, int(bool(symmetry_prior)), logits,
           ws=_ws(spec, grid, n), device=params.device)
    return logits


def sym_loss_grad(spec: K.IcnnSpec, params: Tensor, pose: Tensor, grid: K.Grid, targets: Tensor, symmetry_prior: bool = True,
                  loss: str = "se", weight_mode: str = "none", ratio: float = 1.0, c_fg: float = 0.0, c_bg: float = 0.0,
                  r_eps: float = R_EPS) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (loss [n_images], network gradients [n_images, P], pose gradients [n_images, 3])."""
    params, pose, n = _check(spec, params, pose)
    grid = _grid(grid)
    targets = K._per_point(spec, targets, "targets", n, grid)
    X.on_gpu(params=params, pose=pose, targets=targets)
    lo = L.scratch(n, dtype=torch.float32, device=params.device)
    g, gp = L.scratch_like(params), L.scratch_like(pose)
    X.call("inrfit_sym_loss_grad", spec._desc, _sym_desc(-1, r_eps), params, pose, grid._desc, targets,
           X.loss_desc(loss, weight_mode, ratio, c_fg, c_bg), n, int(bool(symmetry_prior)), lo, g, gp, ws=_ws(spec, grid, n),
           device=params.device)
    return lo, g, gp


def _states(spec, n, dev, opt_state, pose_opt_state):
    if opt_state is None:
        opt_state = K.new_opt_state(spec, n, dev)
    if pose_opt_state is None:
        pose_opt_state = new_pose_opt_state(n, dev)
    return (X.rows(opt_state, "opt_state", n, 2 * spec.n_params + L.INR_OPT_HEADER_FLOATS),
            X.rows(pose_opt_state, "pose_opt_state", n, 6))


def _opt_desc(lr, betas, eps, weight_decay, plateau) -> L.InrOptDesc:
    """ONE Adam over pose and an unconstrained MLP: no projection, the skip weights stay where they are."""
    return X.opt_desc("adam", lr, betas, eps, weight_decay, clamp=False, plateau=plateau, freeze_skips=True)


def sym_fit(spec: K.IcnnSpec, params: Tensor, pose: Tensor, grid: K.Grid, targets: Tensor, steps: int, lr: float = 1e-3,
            loss: str = "se", weight_mode: str = "none", ratio: float = 1.0, c_fg: float = 0.0, c_bg: float = 0.0,
            symmetry_from_step: int = 0, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
            plateau: Optional[dict] = None, opt_state: Optional[Tensor] = None, pose_opt_state: Optional[Tensor] = None, step0: int = 0,
            record_loss: bool = True, r_eps: float = R_EPS) -> SymFitResult:
    """`steps` full-batch Adam steps over pose and network.  The step with 0-based number step0 + k mirrors iff it is >=
    symmetry_from_step (negative: never)."""
    params, pose, n = _check(spec, params, pose)
    grid = _grid(grid)
    dev = params.device
    targets = K._per_point(spec, targets, "targets", n, grid)
    opt_state, pose_opt_state = _states(spec, n, dev, opt_state, pose_opt_state)
    X.on_gpu(params=params, pose=pose, targets=targets, opt_state=opt_state, pose_opt_state=pose_opt_state)
    hist, _, status = X.fit_outputs(n, steps, None, record_loss, False, dev)
    X.call("inrfit_sym_fit", spec._desc, _sym_desc(symmetry_from_step, r_eps), params, pose, opt_state, pose_opt_state, grid._desc,
           targets, X.loss_desc(loss, weight_mode, ratio, c_fg, c_bg), _opt_desc(lr, betas, eps, weight_decay, plateau), n, int(steps),
           int(step0), hist, status, ws=_ws(spec, grid, n), device=dev)
    return SymFitResult(params, pose, opt_state, pose_opt_state, X.trim(hist, steps), status)


def sym_fit_minibatch(spec: K.IcnnSpec, params: Tensor, pose: Tensor, pool_coords: Tensor, pool_targets: Tensor, index: Tensor,
                      counts: Optional[Sequence[int]] = None, lr: float = 1e-3, loss: str = "se", weight_mode: str = "none",
                      ratio: float = 1.0, c_fg: float = 0.0, c_bg: float = 0.0, symmetry_from_step: int = 0,
                      betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                      plateau: Optional[dict] = None, opt_state: Optional[Tensor] = None, pose_opt_state: Optional[Tensor] = None,
                      step0: int = 0, record_loss: bool = True, r_eps: float = R_EPS) -> SymFitResult:
    """index.shape[0] Adam steps over pose and network, step k on the pixels index[k, :counts[k]] of the pool: pool_coords [2, n_pool]
    and the index table are shared by the images, pool_targets [n_images, n_pool] are their own (`minibatch.fit_minibatch`'s
    contract).  No final logits (`sym_forward`)."""
    params, pose, n = _check(spec, params, pose)
    dev = params.device
    pool_coords, pool_targets, n_pool = MB._pool(spec, n, pool_coords, pool_targets, channels=2)
    opt_state, pose_opt_state = _states(spec, n, dev, opt_state, pose_opt_state)
    X.on_gpu(params=params, pose=pose, pool_coords=pool_coords, pool_targets=pool_targets, opt_state=opt_state, pose_opt_state=pose_opt_state)
    index, carr, steps, batch = MB._table(index, counts, dev)
    ws = X.workspace("inrfit_sym_minibatch_workspace_bytes", spec._desc, batch, n, device=dev)
    hist, _, status = X.fit_outputs(n, steps, None, record_loss, False, dev)
    X.call("inrfit_sym_fit_minibatch", spec._desc, _sym_desc(symmetry_from_step, r_eps), params, pose, opt_state, pose_opt_state,
           pool_coords, pool_targets, n_pool, index, carr, batch, X.loss_desc(loss, weight_mode, ratio, c_fg, c_bg),
           _opt_desc(lr, betas, eps, weight_decay, plateau), n, steps, int(step0), hist, status, ws=ws, device=dev)
    return SymFitResult(params, pose, opt_state, pose_opt_state, X.trim(hist, steps), status)
