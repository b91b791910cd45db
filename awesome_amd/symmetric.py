"""Rotation / mirror-symmetry prior of the teaser on the device: pose and network trained together (include/inrfit.h: inrfit_sym_*,
csrc/sym.h).  Mirrors notebooks/icml_teaser_code/rotation_symmetric/rotation_symmetric.ipynb: `myNet` (cell 2) and its training loop
(cell 3: 10 000 epochs of 500 + 500 random pixels, 2 MSE(bg) + 1 MSE(fg), ONE Adam over pose and network, `symmetry_prior` switched on
once training has started).

The network is an `IcnnSpec(h, 3, 1)` run as an unconstrained MLP (clamp = False, freeze_skips = True); the pose is three numbers per
image, `pose [n_images, 3]` = offset[2] | orientation, with `pose_opt_state [n_images, 6]` = exp_avg[3] | exp_avg_sq[3].  `sym_fit` /
`sym_fit_minibatch` update params, pose and both optimizer states IN PLACE; step k of `sym_fit_minibatch` launches exactly what
`sym_fit(steps=1, step0=step0 + k)` launches on the gathered rows, so a finite run ends bit for bit where the per-step loop ends."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

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
    params, pose = K._check_dev(params, "params"), K._check_dev(pose, "pose")
    if params.dim() != 2 or params.shape[1] != spec.n_params:
        raise ValueError("params must be [n_images, P]")
    if tuple(pose.shape) != (params.shape[0], 3):
        raise ValueError("pose must be [n_images, 3] (offset[2] | orientation)")
    return params, pose, int(params.shape[0])


def _grid(grid: K.Grid) -> K.Grid:
    if grid.mode == L.INR_GRID_EXPLICIT and int(grid.coords.shape[-2]) != 2:
        raise ValueError("the pose reads a 2-channel grid")
    return grid


def _ws(spec: K.IcnnSpec, grid: K.Grid, n_images: int) -> Tensor:
    md, gd = spec.desc(), grid.desc()
    nbytes = L.load().inrfit_sym_workspace_bytes(C.byref(md), C.byref(gd), n_images)
    if nbytes < 0:
        L.check(int(nbytes), "inrfit_sym_workspace_bytes")
    return L.scratch(int(nbytes) // 4 + 1, dtype=torch.float32, device=grid.device)


def _sym_desc(symmetry_from_step: int, r_eps: float) -> L.InrSymDesc:
    return L.InrSymDesc(int(symmetry_from_step), float(r_eps))


def new_pose_opt_state(n_images: int, device) -> Tensor:
    return torch.zeros(n_images, 6, dtype=torch.float32, device=device)


def sym_forward(spec: K.IcnnSpec, params: Tensor, pose: Tensor, grid: K.Grid, symmetry_prior: bool = True, r_eps: float = R_EPS) -> Tensor:
    """logits [n_images, N] of pose + network on the 2-channel grid, with or without the mirror."""
    params, pose, n = _check(spec, params, pose)
    grid = _grid(grid)
    logits = L.scratch(n, grid.n_points, dtype=torch.float32, device=params.device)
    ws = _ws(spec, grid, n)
    md, sd, gd = spec.desc(), _sym_desc(-1, r_eps), grid.desc()
    rc = L.load().inrfit_sym_forward(C.byref(md), C.byref(sd), params.data_ptr(), pose.data_ptr(), C.byref(gd), n, int(bool(symmetry_prior)),
                                     logits.data_ptr(), ws.data_ptr(), ws.numel() * 4, K._stream_ptr(params.device))
    L.check(rc, "inrfit_sym_forward")
    return logits


def sym_loss_grad(spec: K.IcnnSpec, params: Tensor, pose: Tensor, grid: K.Grid, targets: Tensor, symmetry_prior: bool = True,
                  loss: str = "se", weight_mode: str = "none", ratio: float = 1.0, c_fg: float = 0.0, c_bg: float = 0.0,
                  r_eps: float = R_EPS) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (loss [n_images], network gradients [n_images, P], pose gradients [n_images, 3])."""
    params, pose, n = _check(spec, params, pose)
    grid = _grid(grid)
    targets = K._check_dev(targets, "targets").reshape(n, -1)
    lo = L.scratch(n, dtype=torch.float32, device=params.device)
    g, gp = L.scratch_like(params), L.scratch_like(pose)
    ws = _ws(spec, grid, n)
    md, sd, gd, ld = spec.desc(), _sym_desc(-1, r_eps), grid.desc(), K._loss_desc(loss, weight_mode, ratio, c_fg, c_bg)
    rc = L.load().inrfit_sym_loss_grad(C.byref(md), C.byref(sd), params.data_ptr(), pose.data_ptr(), C.byref(gd), targets.data_ptr(),
                                       C.byref(ld), n, int(bool(symmetry_prior)), lo.data_ptr(), g.data_ptr(), gp.data_ptr(), ws.data_ptr(),
                                       ws.numel() * 4, K._stream_ptr(params.device))
    L.check(rc, "inrfit_sym_loss_grad")
    return lo, g, gp


def _states(spec, n, dev, opt_state, pose_opt_state):
    if opt_state is None:
        opt_state = K.new_opt_state(spec, n, dev)
    if pose_opt_state is None:
        pose_opt_state = new_pose_opt_state(n, dev)
    return opt_state, K._check_dev(pose_opt_state, "pose_opt_state")


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
    targets = K._check_dev(targets, "targets").reshape(n, -1)
    opt_state, pose_opt_state = _states(spec, n, dev, opt_state, pose_opt_state)
    hist = L.scratch(n, max(steps, 1), dtype=torch.float32, device=dev) if record_loss else None
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    od = MB._opt_desc("adam", lr, betas, eps, weight_decay, False, plateau, True, False)
    ws = _ws(spec, grid, n)
    md, sd, gd, ld = spec.desc(), _sym_desc(symmetry_from_step, r_eps), grid.desc(), K._loss_desc(loss, weight_mode, ratio, c_fg, c_bg)
    rc = L.load().inrfit_sym_fit(C.byref(md), C.byref(sd), params.data_ptr(), pose.data_ptr(), opt_state.data_ptr(),
                                 pose_opt_state.data_ptr(), C.byref(gd), targets.data_ptr(), C.byref(ld), C.byref(od), n, int(steps),
                                 int(step0), hist.data_ptr() if hist is not None else None, status.data_ptr(), ws.data_ptr(),
                                 ws.numel() * 4, K._stream_ptr(dev))
    L.check(rc, "inrfit_sym_fit")
    return SymFitResult(params, pose, opt_state, pose_opt_state, hist[:, :steps] if hist is not None else None, status)


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
    pool_coords = K._check_dev(pool_coords, "pool_coords")
    pool_targets = K._check_dev(pool_targets, "pool_targets")
    if pool_coords.dim() != 2 or pool_coords.shape[0] != 2:
        raise ValueError("pool_coords must be [2, n_pool] (shared by all images)")
    n_pool = int(pool_coords.shape[1])
    pool_targets = pool_targets.reshape(n, -1)
    if pool_targets.shape[1] != n_pool:
        raise ValueError(f"pool_targets must be [n_images, n_pool], got {tuple(pool_targets.shape)}")
    index, carr, steps, batch = MB._table(index, counts, dev)
    opt_state, pose_opt_state = _states(spec, n, dev, opt_state, pose_opt_state)
    md = spec.desc()
    nbytes = L.load().inrfit_sym_minibatch_workspace_bytes(C.byref(md), batch, n)
    if nbytes < 0:
        L.check(int(nbytes), "inrfit_sym_minibatch_workspace_bytes")
    ws = L.scratch(int(nbytes) // 4 + 1, dtype=torch.float32, device=dev)
    hist = L.scratch(n, max(steps, 1), dtype=torch.float32, device=dev) if record_loss else None
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    od = MB._opt_desc("adam", lr, betas, eps, weight_decay, False, plateau, True, False)
    sd, ld = _sym_desc(symmetry_from_step, r_eps), K._loss_desc(loss, weight_mode, ratio, c_fg, c_bg)
    rc = L.load().inrfit_sym_fit_minibatch(C.byref(md), C.byref(sd), params.data_ptr(), pose.data_ptr(), opt_state.data_ptr(),
                                           pose_opt_state.data_ptr(), pool_coords.data_ptr(), pool_targets.data_ptr(), n_pool,
                                           index.data_ptr(), carr, batch, C.byref(ld), C.byref(od), n, steps, int(step0),
                                           hist.data_ptr() if hist is not None else None, status.data_ptr(), ws.data_ptr(),
                                           ws.numel() * 4, K._stream_ptr(dev))
    L.check(rc, "inrfit_sym_fit_minibatch")
    return SymFitResult(params, pose, opt_state, pose_opt_state, hist[:, :steps] if hist is not None else None, status)
