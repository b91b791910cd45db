"""What every family module's wrappers share on their way into libinrfit.so: the tensor check, the workspace query, the optimizer and
loss descriptors, a fit's output buffers and the call itself.  The C side receives raw pointers and cannot know a buffer's size, so
every tensor a wrapper hands over goes through `rows` / `flat` against the width its spec implies."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L

Tensor = torch.Tensor


# ---- the one tensor check -------------------------------------------------------------------------------------------------------------
def _refuse(t: Tensor, name: str, want: str):
    """float32, then shape.  The device comes last, for all of a wrapper's tensors at once (on_gpu): every shape error shows before
    it, with CPU tensors too."""
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    raise ValueError(f"{name}: expected {want}, got shape {tuple(t.shape)}")


def rows(t: Tensor, name: str, n: Optional[int], width) -> Tensor:
    """t is float32 [n, width], or [n, *width] for a trailing shape (n None: any number of rows); -> the contiguous tensor."""
    s = t.shape
    if type(width) is int:      # (the common case, spelled out: this runs for every tensor of every call of a per-step wrapper)
        if len(s) == 2 and s[1] == width and (n is None or s[0] == n) and t.dtype is torch.float32:
            return t.contiguous()
        trail = (width,)
    else:
        trail = tuple(width)
        if len(s) > 0 and s[1:] == trail and (n is None or s[0] == n) and t.dtype is torch.float32:
            return t.contiguous()
    _refuse(t, name, f"shape {('n' if n is None else n, *trail)}")


def flat(t: Tensor, name: str, numel: int) -> Tensor:
    """t holds `numel` float32 values in any shape (one row of a joint step, the star prior's flat vector); -> the contiguous tensor."""
    if t.numel() == numel and t.dtype is torch.float32:
        return t.contiguous()
    _refuse(t, name, f"{numel} floats")


def on_gpu(**tensors) -> None:
    """Behind a wrapper's shape checks and in front of everything else: none of its tensors lives on the CPU."""
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise L.InrfitError(f"{name} must live on the GPU (awesome_amd has no CPU path)")


def on_device(t: Tensor, name: str) -> Tensor:
    """dtype and device only (icnn._check_dev): for a tensor whose shape the callee derives its sizes from."""
    if t.dtype != torch.float32:
        _refuse(t, name, "")
    on_gpu(**{name: t})
    return t.contiguous()


# ---- workspaces -------------------------------------------------------------------------------------------------------------------------
def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


_plans = {}      # entry -> (positions of its pointer arguments, positions of its structures), from _lib.EXPORTS, once per entry


def _marshal(entry: str, args) -> list:
    """A ctypes.Structure travels by reference, a Tensor as its data pointer; None (NULL), numbers, ctypes arrays and pointers as they
    are.  Which positions can hold which is the entry's own argtypes, read once."""
    plan = _plans.get(entry)
    if plan is None:
        types = L.EXPORTS[entry][1][:len(args)]
        plan = _plans[entry] = (tuple(i for i, t in enumerate(types) if t is C.c_void_p),
                                tuple(i for i, t in enumerate(types) if isinstance(getattr(t, "_type_", None), type)
                                      and issubclass(t._type_, C.Structure)))
    a = list(args)
    for i in plan[0]:
        if isinstance(a[i], Tensor):
            a[i] = a[i].data_ptr()
    for i in plan[1]:
        if a[i] is not None:
            a[i] = C.byref(a[i])
    return a


def workspace(entry: str, *args, device, slack: int = 1) -> Tensor:
    """The size query `entry` (it answers on the host), its negative return raised under its own name, and the scratch buffer:
    nbytes // 4 + slack floats."""
    nbytes = int(getattr(L.load(), entry)(*_marshal(entry, args)))
    if nbytes < 0:
        L.check(nbytes, entry)
    return L.scratch(nbytes // 4 + slack, dtype=torch.float32, device=device)


_ws_cache = {}


def cached_workspace(key, nbytes_fn, device, refresh_under_poison: bool, what: str = "workspace query") -> Tensor:
    """One workspace of nbytes_fn() // 4 + 64 floats per (key, device), for steps that run thousands of times per epoch.
    refresh_under_poison = True (the joint steps): every call writes all of its workspace before it reads it, so under L.POISON a
    fresh NaN-filled one per call is the check that it does.  False (the segmentation networks, _segnet.SegDriver): the workspace
    carries state between two calls - step(reuse_forward=True) reads what forward left in it - and a fresh one would lose it."""
    k = (key, str(device))
    ws = _ws_cache.get(k)
    if ws is None or (refresh_under_poison and L.POISON):
        nbytes = int(nbytes_fn())
        if nbytes < 0:
            L.check(nbytes, what)
        ws = _ws_cache[k] = L.scratch(nbytes // 4 + 64, dtype=torch.float32, device=device)
    return ws


# ---- descriptors ------------------------------------------------------------------------------------------------------------------------
def opt_desc(optimizer: str, lr: float, betas, eps: float, weight_decay: float = 0.0, clamp: bool = False,
             plateau: Optional[dict] = None, freeze_skips: bool = False, freeze_input: bool = False,
             gate_logits: bool = False) -> L.InrOptDesc:
    """The only place that builds an InrOptDesc.  plateau: None = off, a dict = ReduceLROnPlateau with torch's defaults for the keys it
    leaves out.  The library reads the plateau_* fields only behind `plateau` (icnn_update_kernel; inrfit_pcn_fit_sequence's epoch
    end), so while it is off they carry the same defaults from every wrapper."""
    pl = plateau or {}
    return L.InrOptDesc(kind=L.OPT_KINDS[optimizer], lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps),
                        weight_decay=float(weight_decay), clamp=int(bool(clamp)), plateau=int(plateau is not None),
                        plateau_patience=int(pl.get("patience", 200)), plateau_factor=float(pl.get("factor", 0.5)),
                        plateau_threshold=float(pl.get("threshold", 1e-4)), plateau_min_lr=float(pl.get("min_lr", 0.0)),
                        plateau_eps=float(pl.get("eps", 1e-8)), freeze_skips=int(bool(freeze_skips)),
                        freeze_input=int(bool(freeze_input)), logits_at_last_forward=int(bool(gate_logits)))


def loss_desc(kind: str, weight_mode: str, ratio: float, c_fg: float, c_bg: float) -> L.InrLossDesc:
    return L.InrLossDesc(L.LOSS_KINDS[kind], L.WEIGHT_MODES[weight_mode], float(ratio), float(c_fg), float(c_bg))


# ---- a fit's outputs --------------------------------------------------------------------------------------------------------------------
def fit_outputs(n: int, steps: int, logits_shape, record_loss: bool, want_logits: bool, device) -> Tuple[Optional[Tensor], Optional[Tensor], Tensor]:
    """-> (hist [n, max(steps, 1)] or None, logits or None, status [n] int32): hist and logits are scratch, status is zeroed."""
    hist = L.scratch(n, max(steps, 1), dtype=torch.float32, device=device) if record_loss else None
    logits = L.scratch(*logits_shape, dtype=torch.float32, device=device) if want_logits else None
    return hist, logits, torch.zeros(n, dtype=torch.int32, device=device)


def trim(hist: Optional[Tensor], steps: int) -> Optional[Tensor]:
    """The `steps` columns a fit wrote of its loss history (the buffer has at least one)."""
    return hist[..., :steps] if hist is not None else None


# ---- the call ---------------------------------------------------------------------------------------------------------------------------
def call(entry: str, *args, ws: Optional[Tensor] = None, device) -> None:
    """getattr(libinrfit, entry)(*args[, workspace, workspace bytes], stream of `device`), the arguments marshalled by the entry's plan
    (_marshal), the return code checked under `entry`."""
    a = _marshal(entry, args)
    if ws is not None:
        a += (ws.data_ptr(), ws.numel() * 4)
    rc = getattr(L.load(), entry)(*a, _stream_ptr(device))
    if rc != 0:
        L.check(rc, entry)
