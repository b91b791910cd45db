"""Pixel-minibatch fits of the coordinate nets in one device call (include/inrfit.h: inrfit_fit_minibatch, inrfit_cdn_fit_minibatch).

The teaser notebooks train a coordinate net on a fresh random subset of the pixels at every optimizer step:

  convex.ipynb cell 3          myConvexNet(150)            700 epochs of 2000 + 2000 pixels, MSE on the sigmoid, Adam 1e-2, clamp
  repeating.ipynb cell 4       myNet(200)                  10 000 epochs of 500 + 500 pixels, 2 MSE(bg) + 1 MSE(fg)
  imageRepresentationTest.ipynb cell 6  ourSimpleNetwork   150 epochs of DataLoader(batch_size=64, shuffle=True), short last batch
  diffeo_convex.ipynb cells 9-11  ConvexDiffeomorphismNet  2000 epochs of 1000 + 1000 pixels, 2 BCE(bg) + 1 BCE(fg)

`fit_minibatch` / `cdn_fit_minibatch` run such a loop as ONE call: step k gathers the pool by row k of a device index table and then
launches exactly what `fit(steps=1, step0=step0 + k)` launches for that explicit grid, so a finite run ends bit for bit where the
per-step host loop ends.  `class_balanced_batches` and `dataloader_batches` draw the tables."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _call as X
from . import _lib as L
from . import flow as FL
from . import icnn as K

Tensor = torch.Tensor


# ----------------------------------------------------------------------------------------------------------------------
# index tables
# ----------------------------------------------------------------------------------------------------------------------
def draw_class_batches(back: Tensor, fore: Tensor, steps: int, number: int, generator: Optional[torch.Generator] = None,
                       chunk: int = 64) -> Tensor:
    """[steps, 2 * number] int32: per row `number` distinct entries of `back`, then `number` distinct entries of `fore`, each a
    uniformly random subset without repetition - what `torch.randperm(n)[:number]` draws.  Random keys + top-k, `chunk` rows at a
    time, on the generator's device (without one: the pools')."""
    if back.numel() < number or fore.numel() < number:
        raise ValueError(f"need at least {number} pixels of each class (background {back.numel()}, foreground {fore.numel()})")
    dev = generator.device if generator is not None else back.device
    out = torch.empty(steps, 2 * number, dtype=torch.int32, device=dev)
    for s0 in range(0, steps, chunk):
        n = min(chunk, steps - s0)
        for col, pool in ((0, back.to(dev)), (number, fore.to(dev))):
            keys = torch.rand(n, pool.numel(), device=dev, generator=generator)
            out[s0:s0 + n, col:col + number] = pool[torch.topk(keys, number, dim=1).indices].to(torch.int32)
    return out


def class_balanced_batches(labels: Tensor, steps: int, number: int, generator: Optional[torch.Generator] = None) -> Tensor:
    """The notebooks' two `randperm(n)[:number]` draws per epoch: [steps, 2 * number] pixel numbers, `number` distinct background
    pixels (label < 0.5: the labels are the likelihood) followed by `number` distinct foreground pixels."""
    flat = labels.reshape(-1)
    return draw_class_batches(torch.nonzero(flat < 0.5).reshape(-1), torch.nonzero(flat >= 0.5).reshape(-1), steps, number, generator)


def dataloader_batches(n: int, batch_size: int, epochs: int, generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor]:
    """DataLoader(batch_size, shuffle=True) over n items for `epochs` epochs -> (index [steps, batch] int32, counts [steps] int32, on
    the CPU).  One permutation per epoch, cut into batches of `batch_size`, the last one short where batch_size does not divide n; the
    entries behind a short batch repeat its first one (any valid index: they are never read)."""
    if n < 1 or batch_size < 1 or epochs < 0:
        raise ValueError("n and batch_size must be positive, epochs >= 0")
    batch = min(batch_size, n)
    per = (n + batch - 1) // batch
    index = torch.empty(epochs * per, batch, dtype=torch.int32)
    counts = torch.full((epochs * per,), batch, dtype=torch.int32)
    for e in range(epochs):
        perm = torch.randperm(n, generator=generator).to(torch.int32)
        for j in range(per):
            row = perm[j * batch:(j + 1) * batch]
            index[e * per + j, :row.numel()] = row
            index[e * per + j, row.numel():] = row[0]
            counts[e * per + j] = row.numel()
    return index, counts


# ----------------------------------------------------------------------------------------------------------------------
# entry points
# ----------------------------------------------------------------------------------------------------------------------
def _pool(spec: K.IcnnSpec, n_images: int, pool_coords: Tensor, pool_targets: Tensor, channels: Optional[int] = None) -> Tuple[Tensor, Tensor, int]:
    """pool_coords [C, n_pool] (shared by all images; C = spec.in_features unless `channels`) and pool_targets [n_images, n_pool]
    ([n_images, O, n_pool] for n_out > 1), checked -> (pool_coords, pool_targets [n_images, O * n_pool], n_pool)."""
    n_pool = int(pool_coords.shape[-1]) if pool_coords.dim() else 0
    pool_coords = X.rows(pool_coords, "pool_coords", channels or spec.in_features, n_pool)
    return pool_coords, X.flat(pool_targets, "pool_targets", n_images * spec.n_out * n_pool).reshape(n_images, -1), n_pool


def _table(index: Tensor, counts, device) -> Tuple[Tensor, Optional[C.Array], int, int]:
    if index.dim() != 2 or index.shape[1] < 1:
        raise ValueError("index: expected (steps, batch)")
    index = index.to(device=device, dtype=torch.int32).contiguous()
    steps, batch = int(index.shape[0]), int(index.shape[1])
    carr = None
    if counts is not None:
        host = [int(c) for c in (counts.tolist() if isinstance(counts, torch.Tensor) else counts)]
        if len(host) != steps:
            raise ValueError("counts: one per step")
        carr = (C.c_int32 * max(steps, 1))(*host)
    return index, carr, steps, batch


def _workspace(spec: K.IcnnSpec, fspec: Optional[FL.FlowSpec], batch: int, n_images: int, device) -> Tensor:
    if fspec is not None and not spec.fused():   # the flow over a layer-by-layer ICNN: its own entry pair
        return X.workspace("inrfit_cdn_wide_minibatch_workspace_bytes", spec._desc, fspec._desc, batch, n_images, device=device)
    return X.workspace("inrfit_minibatch_workspace_bytes", spec._desc, fspec._desc if fspec is not None else None, batch, n_images,
                       device=device)


def fit_minibatch(spec: K.IcnnSpec, params: Tensor, pool_coords: Tensor, pool_targets: Tensor, index: Tensor,
                  counts: Optional[Sequence[int]] = None, lr: float = 2e-3, loss: str = "se", weight_mode: str = "none",
                  ratio: float = 1.0, c_fg: float = 0.0, c_bg: float = 0.0, optimizer: str = "adam",
                  betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, clamp: bool = True,
                  plateau: Optional[dict] = None, opt_state: Optional[Tensor] = None, step0: int = 0, record_loss: bool = True,
                  freeze_skips: bool = False, freeze_input: bool = False) -> K.FitResult:
    """index.shape[0] optimizer steps of n_images independent fits (params [n_images, P] updated IN PLACE), step k on the pixels
    index[k, :counts[k]] of the pool: pool_coords [C, n_pool] and the index table are shared by the images, pool_targets
    [n_images, n_pool] ([n_images, O, n_pool] for n_out > 1) are their own.  The keyword arguments are `icnn.fit`'s; there are no
    final logits (inference over all pixels is `icnn.forward`)."""
    K._check_spec(spec)
    params = X.rows(params, "params", None, spec.n_params)
    n_images, dev = params.shape[0], params.device
    pool_coords, pool_targets, n_pool = _pool(spec, n_images, pool_coords, pool_targets)
    if opt_state is None:
        opt_state = K.new_opt_state(spec, n_images, dev)
    opt_state = X.rows(opt_state, "opt_state", n_images, 2 * spec.n_params + L.INR_OPT_HEADER_FLOATS)
    X.on_gpu(params=params, pool_coords=pool_coords, pool_targets=pool_targets, opt_state=opt_state)
    index, carr, steps, batch = _table(index, counts, dev)
    ws = _workspace(spec, None, batch, n_images, dev)
    hist, _, status = X.fit_outputs(n_images, steps, None, record_loss, False, dev)
    od = X.opt_desc(optimizer, lr, betas, eps, weight_decay, clamp, plateau, freeze_skips, freeze_input)
    X.call("inrfit_fit_minibatch", spec._desc, params, opt_state, pool_coords, pool_targets, n_pool, index, carr, batch,
           X.loss_desc(loss, weight_mode, ratio, c_fg, c_bg), od, n_images, steps, int(step0), hist, status, ws=ws, device=dev)
    return K.FitResult(params, opt_state, X.trim(hist, steps), None, status)


def cdn_fit_minibatch(ispec: K.IcnnSpec, fspec: FL.FlowSpec, icnn_params: Tensor, flow_params: Tensor, pool_coords: Tensor,
                      pool_targets: Tensor, index: Tensor, counts: Optional[Sequence[int]] = None, lr: float = 3e-3, loss: str = "bce",
                      weight_mode: str = "none", ratio: float = 1.0, c_fg: float = 0.0, c_bg: float = 0.0,
                      weight_decay_on_weight_g: float = 5e-5, betas=(0.9, 0.999), eps: float = 1e-8, clamp: bool = True,
                      plateau: Optional[dict] = None, icnn_opt_state: Optional[Tensor] = None,
                      flow_opt_state: Optional[Tensor] = None, step0: int = 0, record_loss: bool = True) -> FL.CdnFitResult:
    """`fit_minibatch` for ICNN(flow(Ax + b)): `flow.cdn_fit`'s step (Adam over everything, weight decay on the weight_g group) on
    the pixels index[k, :counts[k]] of the pool at step k.  No final logits (`flow.cdn_forward`).  An ICNN of the layer-by-layer path
    (n_hidden > 130 or more than two hidden layers) goes through inrfit_cdn_wide_fit_minibatch, the same call for those shapes."""
    ip, fp, n = FL._params(ispec, fspec, icnn_params, flow_params)
    dev = ip.device
    pool_coords, pool_targets, n_pool = _pool(ispec, n, pool_coords, pool_targets)
    icnn_opt_state, flow_opt_state = K._opt_states(ispec, fspec.n_params, n, dev, icnn_opt_state, flow_opt_state)
    X.on_gpu(icnn_params=ip, flow_params=fp, pool_coords=pool_coords, pool_targets=pool_targets, icnn_opt_state=icnn_opt_state,
             flow_opt_state=flow_opt_state)
    index, carr, steps, batch = _table(index, counts, dev)
    ws = _workspace(ispec, fspec, batch, n, dev)
    hist, _, status = X.fit_outputs(n, steps, None, record_loss, False, dev)
    od = X.opt_desc("adam", lr, betas, eps, clamp=clamp, plateau=plateau)
    X.call("inrfit_cdn_fit_minibatch" if ispec.fused() else "inrfit_cdn_wide_fit_minibatch", ispec._desc, fspec._desc, ip, fp, icnn_opt_state, flow_opt_state, pool_coords, pool_targets,
           n_pool, index, carr, batch, X.loss_desc(loss, weight_mode, ratio, c_fg, c_bg), od, float(weight_decay_on_weight_g), n, steps,
           int(step0), hist, status, ws=ws, device=dev)
    return FL.CdnFitResult(ip, fp, icnn_opt_state, flow_opt_state, X.trim(hist, steps), None, status)


# ----------------------------------------------------------------------------------------------------------------------
# the module surface (model/convex_net.py _IcnnModule.fit_minibatch, model/diffeomorphism_net.py)
# ----------------------------------------------------------------------------------------------------------------------
def module_batches(labels: Tensor, n_pixels: int, num_epochs: int, number: Optional[int], batch_size: Optional[int],
                   class_weights: Tuple[float, float], batch_index: Optional[Tensor], counts, generator) -> Tuple[Tensor, object, dict]:
    """The index table and the loss weighting of a module's `fit_minibatch`: `number` per class -> class-balanced rows and the loss
    w_bg mean(bg) + w_fg mean(fg) as INR_WEIGHT_EXPLICIT (the kernels' c_fg weighs the targets < 0.5, the notebooks' background);
    `batch_size` -> DataLoader rows and the plain mean."""
    if (number is None) == (batch_size is None) and batch_index is None:
        raise ValueError("give `number` (pixels per class and epoch) or `batch_size` (DataLoader batches)")
    weights = dict(weight_mode="none")
    if batch_size is None and (number is not None or batch_index is not None):
        per = int(number) if number is not None else int(batch_index.shape[1]) // 2
        weights = dict(weight_mode="explicit", c_fg=float(class_weights[0]) / per, c_bg=float(class_weights[1]) / per)
    if batch_index is None:
        if number is not None:
            batch_index = class_balanced_batches(labels, num_epochs, int(number), generator)
        else:
            batch_index, counts = dataloader_batches(int(n_pixels), int(batch_size), num_epochs, generator)
    return batch_index, counts, weights
