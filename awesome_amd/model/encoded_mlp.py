"""Coordinate MLPs behind a periodic ENCODE stage (SURVEY.md §0 "Fourier/SIREN positional encoding -> small MLP").

The `awesome/` package has no such model; its two instances live in notebooks, and these classes follow them:

  FourierFeatureNet   `ourSimpleNetwork` (notebooks/imageRepresentationTest.ipynb cell 5):
                          x -> cos(x @ A + b)   with fixed buffers A = factor * randn(d_in, d_features), b = randn(d_features)
                            -> relu(fc1) -> relu(fc2) [-> relu(fc3)] -> fc_out     (the notebook ends in a sigmoid; here, as for
                          every model of this package, the sigmoid belongs to the wrapper / the data term)
  SineLayerNet        `myNet` (notebooks/icml_teaser_code/repeating/repeating.ipynb cell 3):
                          x -> sin(10 pi * W1(x + offset))  with a learnable W1 and a fixed offset  -> ... -> W_out

On the HIP path the encode IS layer 0 of the ICNN kernels with another activation (include/inrfit.h INR_ACT_COS / INR_ACT_SIN): the
network is  encode (d_features features) -> L relu layers of n_hidden units -> d_out outputs.  With d_features = n_hidden, d_out = 1 and
L in {1, 2} it is a shape of the fused step kernels (features computed in registers where relu(W_in x + b_in) is otherwise); the
notebooks' own shapes - `ourSimpleNetwork(2, 20, 350, 3, 30)`: 20 features -> 3 x 350 -> RGB, and `myNet(200)`: 200 sine units read
out directly (n_hidden_layers = 0) - run layer by layer (csrc/wide.h, the general shapes of ABI 8).  `load_notebook_state_dict` takes
the notebook classes' state_dicts.  No skip connections, no convexity clamp (`fit_options`); the Fourier features stay fixed
(`freeze_input`).  Autograd works through _IcnnFunction; `pretrain` (PriorFitMixin) fits one-channel priors only."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from .. import icnn as K
from .convex_net import _IcnnFunction, _IcnnModule


class _EncodedMLP(_IcnnModule):
    """Shared plumbing: the flat ICNN parameter vector with zero skip weights; subclasses provide layer 0."""

    def _layer0(self):
        raise NotImplementedError

    def _hidden(self) -> List[nn.Linear]:
        return [getattr(self, f"fc{k + 1}") for k in range(self.spec.n_layers)]

    def _param_list(self, detach: bool):
        w0, b0 = self._layer0()
        h, c = self.spec.n_hidden, self.spec.in_features
        dev = self.out.weight.device
        z = lambda *shape: torch.zeros(*shape, device=dev)  # noqa: E731  (skip weights: constants of value 0)
        ps = [w0, b0]
        for lin in self._hidden():
            ps += [lin.weight, lin.bias, z(h, c)]
        ps += [self.out.weight, self.out.bias, z(self.spec.n_out, c)]
        return [p.detach() for p in ps] if detach else ps

    def flat_parameters(self) -> torch.Tensor:
        return torch.cat([p.reshape(-1) for p in self._param_list(True)]).to(torch.float32)

    def forward(self, x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        """(B,C,H,W) -> (B,O,H,W) or (N,C) -> (N,O) logits (O = d_out), forward and autograd backward on the HIP path."""
        if not x.is_cuda:
            raise RuntimeError("awesome_amd modules run on the MI355X only (no CPU fallback); move module and input to cuda")
        params = self._param_list(False)
        o = self.spec.n_out
        if x.dim() == 4:
            b, c, h, w = x.shape
            return torch.stack([_IcnnFunction.apply(x[i].reshape(c, h * w), self.spec, *params).reshape(o, h, w) for i in range(b)], 0)
        y = _IcnnFunction.apply(x.t().contiguous(), self.spec, *params)
        return y[:, None] if o == 1 else y.t()   # ([O, N] from the channel-planar kernels)

    def pretrain(self, *args, **kwargs):
        if self.spec.n_out > 1:
            raise ValueError(f"{type(self).__name__} with d_out = {self.spec.n_out}: a segmentation prior has one output channel")
        return super().pretrain(*args, **kwargs)

    def _engine_fit(self, grid, unaries, flat, epochs, cold, opts, states=None):
        if self.spec.n_out > 1:
            raise ValueError(f"{type(self).__name__} with d_out = {self.spec.n_out}: a segmentation prior has one output channel")
        return super()._engine_fit(grid, unaries, flat, epochs, cold, opts, states)

    def enforce_convexity(self) -> None:   # the prior-module contract; nothing is constrained here
        return None

    def reset_parameters(self) -> None:
        """New draw of every linear layer (the retry of a failed fit, PriorFitMixin._engine_fresh_state); fixed features and poses stay."""
        for m in self.children():
            if isinstance(m, nn.Linear):
                m.reset_parameters()

    # -- PriorFitMixin engine: state_dict <-> flat -----------------------------------------------------------------------------
    def _engine_pack(self, sd: Dict[str, torch.Tensor]) -> torch.Tensor:
        keep = {k: v.detach().clone() for k, v in self.state_dict().items()}
        self.load_state_dict({k: v.to(self.out.weight.device) for k, v in sd.items()})
        flat = self.flat_parameters().cpu()
        self.load_state_dict(keep)
        return flat

    def _engine_unpack(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        sd = K.unpack_params(self.spec, flat)
        out = self._unpack_layer0(sd)
        for k in range(self.spec.n_layers):
            out[f"fc{k + 1}.weight"], out[f"fc{k + 1}.bias"] = sd[f"skip.{k}.ln.weight"], sd[f"skip.{k}.ln.bias"]
        out["out.weight"], out["out.bias"] = sd["out.ln.weight"], sd["out.ln.bias"]
        return out

    unpack_flat = _engine_unpack   # the name the fitters use for modules with their own key layout (like FCNet)


class FourierFeatureNet(_EncodedMLP):
    #: `awesome_amd.fit` options for this model: unconstrained MLP, fixed features
    fit_options = dict(clamp=False, freeze_skips=True, freeze_input=True)

    def __init__(self, d_in: int = 2, n_hidden: int = 130, n_hidden_layers: int = 1, factor: float = 30.0,
                 d_features: Optional[int] = None, d_out: int = 1, **kwargs):
        super().__init__()
        f = n_hidden if d_features is None else int(d_features)
        # (d_features = n_hidden, d_out = 1: today's spec, the fused kernels for n_hidden <= 130 and L <= 2)
        self.spec = K.IcnnSpec(n_hidden, d_in, n_hidden_layers, act0="cos", n_features=0 if f == n_hidden else f, n_out=int(d_out))
        # same creation order and expressions as the notebook's constructor: A, b, fc1 .. fcL, then the head (its fc{L+1})
        self.register_buffer("A", factor * torch.randn(d_in, f))
        self.register_buffer("b", torch.randn(f))
        for k in range(n_hidden_layers):
            setattr(self, f"fc{k + 1}", nn.Linear(f if k == 0 else n_hidden, n_hidden))
        self.out = nn.Linear(n_hidden if n_hidden_layers > 0 else f, int(d_out))

    def load_notebook_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """state_dict of `ourSimpleNetwork` (A, b, fc1 .. fc{L+1}): its last linear layer is this module's `out`."""
        n = self.spec.n_layers
        mine = {("out" + k[len(f"fc{n + 1}"):] if k.startswith(f"fc{n + 1}.") else k): v for k, v in sd.items()}
        self.load_state_dict(mine)

    def _layer0(self):
        return self.A.t().contiguous(), self.b          # cos(x @ A + b) = cos(W_in x + b_in) with W_in = A^T

    def _unpack_layer0(self, sd):
        return {"A": sd["input.weight"].t().contiguous(), "b": sd["input.bias"]}


class SineLayerNet(_EncodedMLP):
    """n_hidden_layers = 0 is `myNet`'s own shape: W2(sin(omega W1(x + offset))), the sine units read out directly."""
    fit_options = dict(clamp=False, freeze_skips=True)

    def __init__(self, in_features: int = 2, n_hidden: int = 130, n_hidden_layers: int = 1, omega: float = 10 * 3.141592, **kwargs):
        super().__init__()
        self.spec = K.IcnnSpec(n_hidden, in_features, n_hidden_layers, act0="sin", omega=float(omega))   # 10*3.141592 as in the cell
        self.offset = nn.Parameter(torch.zeros(1, in_features), requires_grad=False)
        self.W1 = nn.Linear(in_features, n_hidden)
        for k in range(n_hidden_layers):
            setattr(self, f"fc{k + 1}", nn.Linear(n_hidden, n_hidden))
        self.out = nn.Linear(n_hidden, 1)

    def load_notebook_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """state_dict of `myNet` (offset, W0, W1, W2): W2 is this module's `out`; W0 is ignored (myNet.forward never uses it)."""
        mine = {("out" + k[2:] if k.startswith("W2.") else k): v for k, v in sd.items() if not k.startswith("W0.")}
        self.load_state_dict(mine)

    def _layer0(self):
        # W1(x + offset) = W1 x + (W1 offset + b1): the fixed offset folds into the bias the kernel sees
        return self.W1.weight, self.W1.bias + (self.offset @ self.W1.weight.t()).reshape(-1)

    def _unpack_layer0(self, sd):
        w = sd["input.weight"]
        off = self.offset.detach().cpu()
        return {"offset": off.clone(), "W1.weight": w, "W1.bias": sd["input.bias"] - (off @ w.t()).reshape(-1)}
