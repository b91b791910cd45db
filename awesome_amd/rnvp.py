"""Host-side driver of the HIP RealNVP kernels and of the fused PathConnectedNet fit (include/inrfit.h, InrRnvpDesc part).

  rnvp_forward  <- PathConnectedNet.get_deformation                 (awesome/model/path_connected_net.py:124-128)
  rnvp_backward <- its autograd backward (get_deformation(differentiable=True))
  pcn_forward   <- PathConnectedNet.forward                         (:79-85)
  pcn_loss_grad <- criterion(sigmoid(model(grid)), unaries).backward()  w.r.t. every parameter
  pcn_fit       <- the inner loop of _prior_based_pretrain          (:937-962, Adamax + param groups :922-929)
  actnorm_init  <- the data-dependent first forward of nf.flows.ActNorm
  pcn_fit_sequence      <- the mini-batch epochs of _non_prior_based_pretrain (:634-713) in one device call
  fit_identity_sequence <- the mini-batched learn_flow_identity (:200-236) in one device call
  sequence_orders       <- the frame orders of the reference's DataLoaders

The flow itself (MaskedAffineFlow / ActNorm / MLP) is normflows==1.7.3 code that is not part of the reference checkout:
parity for this variant is UNPINNED; the flow is built as awesome/model/net_factory.py:70-114 builds it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from functools import cached_property
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _call as X
from . import _lib as L
from . import icnn as K

Tensor = torch.Tensor


def rnvp_masks(channels: int, n_flows: int) -> List[int]:
    """Coupling masks of init_realnvp (awesome/model/net_factory.py:86-99): 1 .. 2^C - 2 counted in binary (bit c = channel c),
    repeated to n_flows entries."""
    base = list(range(1, 2 ** channels - 1))
    return [base[i % len(base)] for i in range(n_flows)]


@dataclass(frozen=True)
class RnvpSpec:
    channels: int = 2
    hidden_units: int = 32
    n_flows: int = 12
    output_fn: Optional[str] = "tanh"
    output_scale: Optional[float] = None
    vmin: Tuple[float, ...] = (0.0, 0.0)
    vmax: Tuple[float, ...] = (1.0, 1.0)
    new_min: float = -1.0
    new_max: float = 1.0
    masks: Tuple[int, ...] = field(default=())

    def __post_init__(self):
        if self.output_fn not in (None, "tanh"):
            raise ValueError("output_fn must be None or 'tanh' (the only ones the reference configs use)")
        if not self.masks:
            object.__setattr__(self, "masks", tuple(rnvp_masks(self.channels, self.n_flows)))
        if len(self.vmin) != self.channels or len(self.vmax) != self.channels:
            object.__setattr__(self, "vmin", tuple([0.0] * self.channels) if len(self.vmin) != self.channels else self.vmin)
            object.__setattr__(self, "vmax", tuple([1.0] * self.channels) if len(self.vmax) != self.channels else self.vmax)

    def desc(self) -> L.InrRnvpDesc:
        d = L.InrRnvpDesc()
        d.channels, d.hidden_units, d.n_flows = self.channels, self.hidden_units, self.n_flows
        d.output_fn = 1 if self.output_fn == "tanh" else 0
        d.output_scale = float(self.output_scale) if self.output_scale is not None else 1.0
        for c in range(self.channels):
            d.vmin[c], d.vmax[c] = float(self.vmin[c]), float(self.vmax[c])
        d.new_min, d.new_max = float(self.new_min), float(self.new_max)
        for f, m in enumerate(self.masks):
            d.masks[f] = int(m)
        return d

    @cached_property
    def _desc(self) -> L.InrRnvpDesc:      # for the wrappers, once per spec (never written to)
        return self.desc()

    @property
    def net_params(self) -> int:
        return 2 * self.hidden_units * self.channels + self.hidden_units + self.channels

    @cached_property
    def n_params(self) -> int:
        return 2 * self.channels + self.n_flows * (2 * self.net_params + 2 * self.channels)

    def keys_shapes(self, prefix: str = "flow_net.net.network.", linear_prefix: str = "linear.") -> List[Tuple[str, Tuple[int, ...]]]:
        """state_dict keys of PathConnectedNet's flow part (NormNet(PixelizeNet(nf.NormalizingFlow))) in flat-vector order."""
        c, h = self.channels, self.hidden_units
        out = [(linear_prefix + "weight", (c, 1, 1, 1)), (linear_prefix + "bias", (c,))]
        for f in range(self.n_flows):
            for net in ("s", "t"):
                b = f"{prefix}flows.{2 * f}.{net}.net."
                out += [(b + "0.weight", (h, c)), (b + "0.bias", (h,)), (b + "2.weight", (c, h)), (b + "2.bias", (c,))]
            b = f"{prefix}flows.{2 * f + 1}."
            out += [(b + "s", (1, c)), (b + "t", (1, c))]
        return out

    def actnorm_slices(self) -> List[Tuple[int, int]]:
        """(start, stop) of every flow's ActNorm s|t block in the flat vector."""
        c, pf = self.channels, 2 * self.net_params + 2 * self.channels
        return [(2 * c + f * pf + 2 * self.net_params, 2 * c + (f + 1) * pf) for f in range(self.n_flows)]


def pack_rnvp_state_dict(spec: RnvpSpec, sd: Dict[str, Tensor], device=None) -> Tensor:
    parts = []
    for k, shp in spec.keys_shapes():
        t = sd[k]
        if tuple(t.shape) != shp:
            raise ValueError(f"{k}: expected shape {shp}, got {tuple(t.shape)}")
        parts.append(t.detach().reshape(-1).to(torch.float32))
    flat = torch.cat(parts)
    return flat.to(device) if device is not None else flat


def unpack_rnvp_params(spec: RnvpSpec, flat: Tensor) -> Dict[str, Tensor]:
    flat = flat.detach().reshape(-1).clone()
    out, off = {}, 0
    for k, shp in spec.keys_shapes():
        n = 1
        for s in shp:
            n *= s
        out[k] = flat[off:off + n].reshape(shp)
        off += n
    return out


def init_rnvp_params(spec: RnvpSpec) -> Tensor:
    """Fresh flow parameters as the reference factory creates them (global torch RNG, like the reference): nn.Linear default
    init for the hidden layers, zeros for the MLPs' last layers (init_zeros=True, net_factory.py:104-105), ActNorm s = t = 0
    (set by actnorm_init on first use), linear weight 1 / bias 0 (path_connected_net.py:72-77)."""
    sd = {}
    for k, shp in spec.keys_shapes():
        if k.endswith("net.0.weight"):
            lin = torch.nn.Linear(shp[1], shp[0])
            sd[k] = lin.weight.data
            sd[k[:-len("weight")] + "bias"] = lin.bias.data
        elif k.endswith("net.0.bias"):
            continue
        elif k == "linear.weight":
            sd[k] = torch.ones(shp)
        else:
            sd[k] = torch.zeros(shp)
    return pack_rnvp_state_dict(spec, sd)


def _ws(ispec: Optional[K.IcnnSpec], rspec: RnvpSpec, grid: K.Grid, n_images: int) -> Tensor:
    return X.workspace("inrfit_pcn_workspace_bytes", ispec._desc if ispec is not None else None, rspec._desc, grid._desc, n_images,
                       device=grid.device)


def _flow_params(rspec: RnvpSpec, flow_params: Tensor, n: Optional[int] = None) -> Tensor:
    return X.rows(flow_params, "flow_params", n, rspec.n_params)


def _params(ispec: K.IcnnSpec, rspec: RnvpSpec, icnn_params: Tensor, flow_params: Tensor, n: Optional[int] = None) -> Tuple[Tensor, Tensor, int]:
    """icnn_params [n_images, P] and flow_params [n_images, RP], checked against their specs."""
    K._check_spec(ispec)
    ip = X.rows(icnn_params, "icnn_params", n, ispec.n_params)
    return ip, _flow_params(rspec, flow_params, ip.shape[0]), ip.shape[0]


def actnorm_init(rspec: RnvpSpec, flow_params: Tensor, grid: K.Grid) -> Tensor:
    """Data-dependent ActNorm initialisation, in place on flow_params [n_images, RP]."""
    fp = _flow_params(rspec, flow_params)
    X.on_gpu(flow_params=fp)
    n = fp.shape[0]
    X.call("inrfit_rnvp_actnorm_init", rspec._desc, fp, grid._desc, n, ws=_ws(None, rspec, grid, n), device=fp.device)
    return fp


def rnvp_forward(rspec: RnvpSpec, flow_params: Tensor, grid: K.Grid) -> Tensor:
    """flow_params [n_images, RP] -> deformed coordinates [n_images, C, N]."""
    fp = _flow_params(rspec, flow_params)
    X.on_gpu(flow_params=fp)
    n = fp.shape[0]
    out = L.scratch(n, rspec.channels, grid.n_points, dtype=torch.float32, device=fp.device)
    X.call("inrfit_rnvp_forward", rspec._desc, fp, grid._desc, n, out, ws=_ws(None, rspec, grid, n), device=fp.device)
    return out


def rnvp_backward(rspec: RnvpSpec, flow_params: Tensor, grid: K.Grid, dout: Tensor, want_dcoords: bool = False):
    """The vector-Jacobian product of rnvp_forward: dout [n_images, C, N] (d loss / d deformed coordinates) -> flow gradients
    [n_images, RP] in the flat layout (linear.weight / linear.bias included); with want_dcoords also d loss / d input coordinates
    [n_images, C, N].  Returns flow_grads or (flow_grads, dcoords)."""
    fp = _flow_params(rspec, flow_params)
    n = fp.shape[0]
    dout = X.flat(dout, "dout", n * rspec.channels * grid.n_points)
    X.on_gpu(flow_params=fp, dout=dout)
    gf = L.scratch_like(fp)
    din = L.scratch(n, rspec.channels, grid.n_points, dtype=torch.float32, device=fp.device) if want_dcoords else None
    X.call("inrfit_rnvp_backward", rspec._desc, fp, grid._desc, dout, n, gf, din, ws=_ws(None, rspec, grid, n), device=fp.device)
    return (gf, din) if want_dcoords else gf


def rnvp_inverse(rspec: RnvpSpec, flow_params: Tensor, coords: Tensor) -> Tensor:
    """PathConnectedNet.inverse (path_connected_net.py:107-122): coords (C, N) shared or (n_images, C, N) -> [n_images, C, N]."""
    fp = _flow_params(rspec, flow_params)
    n, N = fp.shape[0], (coords.shape[-1] if coords.dim() else 0)
    coords = X.rows(coords, "coords", n, (rspec.channels, N)) if coords.dim() == 3 else X.rows(coords, "coords", rspec.channels, N)
    X.on_gpu(flow_params=fp, coords=coords)
    stride = 0 if coords.dim() == 2 else coords.shape[1] * coords.shape[2]
    out = L.scratch(n, rspec.channels, N, dtype=torch.float32, device=fp.device)
    X.call("inrfit_rnvp_inverse", rspec._desc, fp, coords, stride, N, n, out, ws=_ws(None, rspec, K.Grid.explicit(coords), n),
           device=fp.device)
    return out


def fit_identity(rspec: RnvpSpec, flow_params: Tensor, grid: K.Grid, steps: int = 100, lr: float = 1e-2, weight_decay: float = 1e-5,
                 optimizer: str = "adamax", betas=(0.9, 0.999), eps: float = 1e-8, flow_opt_state: Optional[Tensor] = None,
                 step0: int = 0) -> Tuple[Tensor, Tensor]:
    """PathConnectedNet.learn_flow_identity (path_connected_net.py:155-250; defaults of the prefit kwargs :771-774): the flow_net
    alone is trained towards the identity on the grid, in place on flow_params [n_images, RP].  Returns (loss_hist, opt_state)."""
    fp = _flow_params(rspec, flow_params)
    n, dev = fp.shape[0], fp.device
    flow_opt_state = _flow_opt_state(rspec, n, dev, flow_opt_state)
    X.on_gpu(flow_params=fp, flow_opt_state=flow_opt_state)
    hist = L.scratch(n, max(steps, 1), dtype=torch.float32, device=dev)
    X.call("inrfit_rnvp_fit_identity", rspec._desc, fp, flow_opt_state, grid._desc, X.opt_desc(optimizer, lr, betas, eps, weight_decay),
           n, int(steps), int(step0), hist, ws=_ws(None, rspec, grid, n), device=dev)
    return hist[:, :steps], flow_opt_state


def _flow_opt_state(rspec: RnvpSpec, n: int, dev, flow_opt_state: Optional[Tensor]) -> Tensor:
    if flow_opt_state is None:
        flow_opt_state = torch.zeros(n, 2 * rspec.n_params, dtype=torch.float32, device=dev)
    return X.rows(flow_opt_state, "flow_opt_state", n, 2 * rspec.n_params)


def pcn_forward(ispec: K.IcnnSpec, rspec: RnvpSpec, icnn_params: Tensor, flow_params: Tensor, grid: K.Grid) -> Tensor:
    ip, fp, n = _params(ispec, rspec, icnn_params, flow_params)
    X.on_gpu(icnn_params=ip, flow_params=fp)
    logits = L.scratch(n, grid.n_points, dtype=torch.float32, device=ip.device)
    X.call("inrfit_pcn_forward", ispec._desc, rspec._desc, ip, fp, grid._desc, n, logits, ws=_ws(ispec, rspec, grid, n),
           device=ip.device)
    return logits


def pcn_loss_grad(ispec: K.IcnnSpec, rspec: RnvpSpec, icnn_params: Tensor, flow_params: Tensor, grid: K.Grid, targets: Tensor,
                  loss: str = "se", weight_mode: str = "none", ratio: float = 1.0) -> Tuple[Tensor, Tensor, Tensor]:
    ip, fp, n = _params(ispec, rspec, icnn_params, flow_params)
    targets = K._per_point(ispec, targets, "targets", n, grid)
    X.on_gpu(icnn_params=ip, flow_params=fp, targets=targets)
    lo = L.scratch(n, dtype=torch.float32, device=ip.device)
    gi, gf = L.scratch_like(ip), L.scratch_like(fp)
    X.call("inrfit_pcn_loss_grad", ispec._desc, rspec._desc, ip, fp, grid._desc, targets, X.loss_desc(loss, weight_mode, ratio, 0.0, 0.0),
           n, lo, gi, gf, ws=_ws(ispec, rspec, grid, n), device=ip.device)
    return lo, gi, gf


@dataclass
class PcnFitResult:
    icnn_params: Tensor
    flow_params: Tensor
    icnn_opt_state: Tensor
    flow_opt_state: Tensor
    loss_hist: Optional[Tensor]
    logits: Optional[Tensor]
    status: Tensor


def pcn_fit(ispec: K.IcnnSpec, rspec: RnvpSpec, icnn_params: Tensor, flow_params: Tensor, grid: K.Grid, targets: Tensor,
            steps: int, lr: float = 1e-3, optimizer: str = "adamax", loss: str = "se", weight_mode: str = "none",
            ratio: float = 1.0, flow_weight_decay: float = 1e-5, betas=(0.9, 0.999), eps: float = 1e-8,
            plateau: Optional[dict] = None, icnn_opt_state: Optional[Tensor] = None, flow_opt_state: Optional[Tensor] = None,
            step0: int = 0, record_loss: bool = True, want_logits: bool = True, gate_logits: bool = False) -> PcnFitResult:
    """_prior_based_pretrain's inner loop for PathConnectedNet on the device (defaults of path_connected_net.py:756-760,
    922-933: Adamax lr 1e-3, flow weight decay 1e-5, UnariesWeightedLoss(SE); pass plateau={} for ReduceLROnPlateau(200, 0.5))."""
    ip, fp, n = _params(ispec, rspec, icnn_params, flow_params)
    dev = ip.device
    targets = K._per_point(ispec, targets, "targets", n, grid)
    icnn_opt_state, flow_opt_state = K._opt_states(ispec, rspec.n_params, n, dev, icnn_opt_state, flow_opt_state)
    X.on_gpu(icnn_params=ip, flow_params=fp, targets=targets, icnn_opt_state=icnn_opt_state, flow_opt_state=flow_opt_state)
    hist, logits, status = X.fit_outputs(n, steps, (n, grid.n_points), record_loss, want_logits, dev)
    od = X.opt_desc(optimizer, lr, betas, eps, clamp=True, plateau=plateau, gate_logits=gate_logits)
    X.call("inrfit_pcn_fit", ispec._desc, rspec._desc, ip, fp, icnn_opt_state, flow_opt_state, grid._desc, targets,
           X.loss_desc(loss, weight_mode, ratio, 0.0, 0.0), od, float(flow_weight_decay), n, int(steps), int(step0), hist, logits, status,
           ws=_ws(ispec, rspec, grid, n), device=dev)
    return PcnFitResult(ip, fp, icnn_opt_state, flow_opt_state, X.trim(hist, steps), logits, status)


# ---- sequence pretraining: all mini-batch epochs in one device call (include/inrfit.h, "sequence pretraining") --------------------
def sequence_orders(T: int, batch_size: int, num_epochs: int, shuffle: bool = True, one_loader: bool = False) -> Tensor:
    """Frame orders (num_epochs, T) from torch's own sampler: a DataLoader over range(T) with the caller's batch size, iterated on the
    host under the global torch RNG - the same torch.manual_seed therefore gives the orders the reference's loaders draw.
    one_loader: ONE loader iterated num_epochs times (learn_flow_identity, path_connected_net.py:200-220); else a new loader per epoch
    (the main loop of _non_prior_based_pretrain, :662-668)."""
    from torch.utils.data import DataLoader, TensorDataset
    ds = TensorDataset(torch.arange(T))
    new = lambda: DataLoader(ds, batch_size=int(batch_size), shuffle=bool(shuffle))  # noqa: E731
    loader = new() if one_loader else None
    rows = []
    for _ in range(int(num_epochs)):
        rows.append(torch.cat([b[0] for b in (loader if one_loader else new())]))
    return torch.stack(rows).to(torch.int64) if rows else torch.zeros(0, T, dtype=torch.int64)


def _orders_host(orders, num_epochs: int, T: int):
    """(num_epochs, T) integer tensor -> the host int32 array the C ABI reads (validated there: a permutation per row)."""
    o = torch.as_tensor(orders).detach().to("cpu", torch.int64).reshape(-1, T)
    if o.shape[0] != num_epochs:
        raise ValueError(f"orders must have one row of {T} frame ids per epoch ({num_epochs}), got {tuple(o.shape)}")
    flat = o.reshape(-1).clamp(-2 ** 31, 2 ** 31 - 1).tolist()
    return (C.c_int32 * max(len(flat), 1))(*flat)


def _seq_ws(ispec: Optional[K.IcnnSpec], rspec: RnvpSpec, HW: int, T: int, batch_size: int, device) -> Tensor:
    return X.workspace("inrfit_pcn_sequence_workspace_bytes", ispec._desc if ispec is not None else None, rspec._desc, int(HW), int(T),
                       int(batch_size), device=device)


def _frames(rspec: RnvpSpec, frame_coords: Tensor, orders) -> Tuple[Tensor, int, int, int, C.Array]:
    """frame_coords (T, C, HW) checked -> (it, T, HW, num_epochs, the host order table)."""
    if frame_coords.dim() != 3:
        raise ValueError(f"frame_coords: expected (T, C, HW), got shape {tuple(frame_coords.shape)}")
    fc = X.rows(frame_coords, "frame_coords", None, (rspec.channels, frame_coords.shape[2]))
    T, HW = int(fc.shape[0]), int(fc.shape[2])
    num_epochs = int(torch.as_tensor(orders).reshape(-1, T).shape[0])
    return fc, T, HW, num_epochs, _orders_host(orders, num_epochs, T)


@dataclass
class PcnSequenceResult:
    icnn_params: Tensor
    flow_params: Tensor
    icnn_opt_state: Tensor
    flow_opt_state: Tensor
    epoch_loss: Tensor     # [num_epochs], on the device
    status: Tensor


def pcn_fit_sequence(ispec: K.IcnnSpec, rspec: RnvpSpec, icnn_params: Tensor, flow_params: Tensor, frame_coords: Tensor,
                     frame_targets: Tensor, orders, batch_size: int, lr: float = 1e-3, optimizer: str = "adamax", loss: str = "se",
                     weight_mode: str = "none", ratio: float = 1.0, flow_weight_decay: float = 1e-5, betas=(0.9, 0.999),
                     eps: float = 1e-8, plateau: Optional[dict] = None, icnn_opt_state: Optional[Tensor] = None,
                     flow_opt_state: Optional[Tensor] = None) -> PcnSequenceResult:
    """The mini-batch epochs of _non_prior_based_pretrain (path_connected_net.py:634-713) in ONE `inrfit_pcn_fit_sequence` call: per
    batch of `orders[e]` what pcn_fit(steps=1) runs, per epoch the mean batch loss and ReduceLROnPlateau, nothing read back in
    between.  icnn_params [1, P], flow_params [1, RP] (in place); frame_coords (T, C, HW), frame_targets (T, HW)."""
    ip, fp, _ = _params(ispec, rspec, icnn_params, flow_params, 1)
    dev = ip.device
    fc, T, HW, num_epochs, order = _frames(rspec, frame_coords, orders)
    ft = X.flat(frame_targets, "frame_targets", T * HW)
    icnn_opt_state, flow_opt_state = K._opt_states(ispec, rspec.n_params, 1, dev, icnn_opt_state, flow_opt_state)
    X.on_gpu(icnn_params=ip, flow_params=fp, frame_coords=fc, frame_targets=ft, icnn_opt_state=icnn_opt_state, flow_opt_state=flow_opt_state)
    epoch_loss = L.scratch(max(num_epochs, 1), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    od = X.opt_desc(optimizer, lr, betas, eps, clamp=True, plateau=plateau)
    # the scheduler's numbers as the Python loop carries them (doubles, where the desc holds floats)
    pl = plateau or {}
    schedule = (C.c_double * 5)(float(lr), float(pl.get("factor", 0.5)), float(pl.get("threshold", 1e-4)), float(pl.get("min_lr", 0.0)),
                                float(pl.get("eps", 1e-8)))
    X.call("inrfit_pcn_fit_sequence", ispec._desc, rspec._desc, ip, fp, icnn_opt_state, flow_opt_state, fc, ft, order, T, HW,
           int(batch_size), num_epochs, X.loss_desc(loss, weight_mode, ratio, 0.0, 0.0), od, schedule, float(flow_weight_decay), 0,
           epoch_loss, status, ws=_seq_ws(ispec, rspec, HW, T, batch_size, dev), device=dev)
    return PcnSequenceResult(ip, fp, icnn_opt_state, flow_opt_state, epoch_loss[:num_epochs], status)


def fit_identity_sequence(rspec: RnvpSpec, flow_params: Tensor, frame_coords: Tensor, orders, batch_size: int, lr: float = 1e-2,
                          weight_decay: float = 1e-5, optimizer: str = "adamax", betas=(0.9, 0.999), eps: float = 1e-8,
                          flow_opt_state: Optional[Tensor] = None, step0: int = 0) -> Tuple[Tensor, Tensor]:
    """The mini-batched learn_flow_identity (path_connected_net.py:200-236) in ONE `inrfit_rnvp_fit_identity_sequence` call, in place
    on flow_params [1, RP]; frame_coords (T, C, HW).  Returns (loss_hist [num_epochs]: every epoch's LAST batch loss, opt_state)."""
    fp = _flow_params(rspec, flow_params, 1)
    dev = fp.device
    fc, T, HW, num_epochs, order = _frames(rspec, frame_coords, orders)
    flow_opt_state = _flow_opt_state(rspec, 1, dev, flow_opt_state)
    X.on_gpu(flow_params=fp, frame_coords=fc, flow_opt_state=flow_opt_state)
    hist = L.scratch(max(num_epochs, 1), dtype=torch.float32, device=dev)
    X.call("inrfit_rnvp_fit_identity_sequence", rspec._desc, fp, flow_opt_state, fc, order, T, HW, int(batch_size), num_epochs,
           X.opt_desc(optimizer, lr, betas, eps, weight_decay), int(step0), hist, ws=_seq_ws(None, rspec, HW, T, batch_size, dev), device=dev)
    return hist[:num_epochs], flow_opt_state
