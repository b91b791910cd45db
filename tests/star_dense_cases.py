"""Shared by the star-shape prior's dense-fit tests: seeded problems and the float64 reference loop, built on the CPU from
oracle.inr_oracle (star_shaped_forward, weighted_loss, miou_binary) and torch's own optimizers and ReduceLROnPlateau."""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import inr_oracle as O

KINDS = ("se", "bce")
MODES = ("none", "equal", "ratio", "sssdms", "explicit")
RATIO, C_FG, C_BG = 0.35, 3.0e-3, 1.25e-3     # of the 'ratio' / 'explicit' modes
PARAM_ORDER = ("offset", "W0.weight", "W0.bias", "W1.weight", "W1.bias", "W2.weight", "W2.bias", "W1_r.weight", "W1_r.bias",
               "W2_r.weight", "W2_r.bias")


def grid_rows(height: int, width: int) -> torch.Tensor:
    """(height * width, 2) float32 rows (x, y) of a centred grid, row-major."""
    ii, jj = torch.meshgrid(torch.arange(height), torch.arange(width), indexing="ij")
    return torch.stack([jj.reshape(-1) / (width - 1) - 0.5, ii.reshape(-1) / (height - 1) - 0.5], 1).float()


def star_targets(x: torch.Tensor, centre=(0.03, -0.05), r0: float = 0.22, a: float = 0.1, k: int = 5, soft: bool = False) -> torch.Tensor:
    """Unaries of a k-armed star (fg = low): {0, 1}, or {0.08, 0.93} with `soft`."""
    dx, dy = x[:, 0] - centre[0], x[:, 1] - centre[1]
    inside = (dx * dx + dy * dy).sqrt() < r0 + a * torch.cos(k * torch.atan2(dy, dx))
    t = 1.0 - inside.float()
    return 0.08 + 0.85 * t if soft else t


def make_state(h: int, seed: int, offset=(0.02, -0.04)) -> Dict[str, torch.Tensor]:
    """A seeded StarShapedNet state_dict (float32, CPU) with the centre off the origin and W2_r projected."""
    from awesome_amd.model import StarShapedNet
    torch.manual_seed(seed)
    m = StarShapedNet(h)
    with torch.no_grad():
        m.offset.copy_(torch.tensor([list(offset)]))
        m.enforce_star_shape()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def flat_of(sd: Dict[str, torch.Tensor]) -> torch.Tensor:
    return torch.cat([sd[k].reshape(-1).float() for k in PARAM_ORDER])


def _forward(p: Dict[str, torch.Tensor], x: torch.Tensor, mask_centre: bool) -> torch.Tensor:
    """star_shaped_forward; with mask_centre a pixel exactly at -offset sees a DETACHED centre: it contributes nothing to the centre's
    gradient (the dense entry points' convention), and torch.where keeps its 0/0 out of everyone else's."""
    if not mask_centre:
        return O.star_shaped_forward(p, x)
    at = ((x + p["offset"].detach()) == 0).all(1, keepdim=True)
    q = dict(p)
    q["offset"] = torch.where(at, p["offset"].detach().expand_as(x), p["offset"].expand_as(x))
    return O.star_shaped_forward(q, x)


def criterion(out: torch.Tensor, t: torch.Tensor, kind: str, mode: str) -> torch.Tensor:
    """weighted_loss of the oracle; 'explicit' (no reference class: the how-to loop's per-class coefficients) restated on its terms."""
    if mode != "explicit":
        return O.weighted_loss(out, t, kind, mode, RATIO)
    l = (t - out) ** 2 if kind == "se" else torch.nn.functional.binary_cross_entropy(out, t, reduction="none")
    return (l * torch.where(t < 0.5, torch.full_like(t, C_FG), torch.full_like(t, C_BG))).sum()


def ref_loss_grads(sd: Dict[str, torch.Tensor], x: torch.Tensor, t: torch.Tensor, kind: str, mode: str, dtype=torch.float64,
                   mask_centre: bool = True) -> Tuple[float, Dict[str, torch.Tensor]]:
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    loss = criterion(torch.sigmoid(_forward(p, x.to(dtype), mask_centre)).reshape(-1), t.to(dtype), kind, mode)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach() for k, v in p.items()}


class RefFit:
    """The float64 loop: full batch, torch.optim.Adam / Adamax over every parameter (the centre without a gradient until its first
    step: torch then counts its steps from there), W2_r.weight <- relu, ReduceLROnPlateau stepped with the loss.  Continues across
    calls of `run` like the device fit continues through opt_state / step0."""

    def __init__(self, sd, x, t, kind="se", mode="none", optimizer="adam", lr=1e-2, plateau: Optional[dict] = None, first: int = 0,
                 dtype=torch.float64):
        self.p = {k: v.detach().to(dtype).clone().requires_grad_(k != "offset") for k, v in sd.items()}
        self.x, self.t, self.kind, self.mode, self.first = x.to(dtype), t.to(dtype), kind, mode, first
        cls = torch.optim.Adam if optimizer == "adam" else torch.optim.Adamax
        self.opt = cls([self.p[k] for k in PARAM_ORDER], lr=lr)
        self.sched = torch.optim.lr_scheduler.ReduceLROnPlateau(self.opt, **plateau) if plateau is not None else None
        self.step, self.losses, self.last_forward = 0, [], None

    @property
    def lr(self) -> float:
        return float(self.opt.param_groups[0]["lr"])

    def run(self, steps: int) -> "RefFit":
        for _ in range(steps):
            if self.first >= 0 and self.step >= self.first:
                self.p["offset"].requires_grad_(True)
            out = _forward(self.p, self.x, True)
            loss = criterion(torch.sigmoid(out).reshape(-1), self.t, self.kind, self.mode)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            self.opt.step()
            with torch.no_grad():
                self.p["W2_r.weight"].clamp_(min=0.0)
            self.losses.append(float(loss.detach()))
            self.last_forward = out.detach().reshape(-1)
            if self.sched is not None:
                self.sched.step(self.losses[-1])
            self.step += 1
        return self

    def final_logits(self) -> torch.Tensor:
        with torch.no_grad():
            return _forward(self.p, self.x, True).reshape(-1)

    def state(self) -> Dict[str, torch.Tensor]:
        return {k: v.detach().clone() for k, v in self.p.items()}


def unflatten(h: int, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
    from awesome_amd import star as S
    return S.unflatten(S.StarSpec(h), flat)


def assert_grads_close(h: int, grads: torch.Tensor, ref: Dict[str, torch.Tensor], rtol: float = 5e-4, what: str = "") -> None:
    """The project's bars for this network: rtol 5e-4 with atol 5e-4 max|ref| per tensor."""
    g = unflatten(h, grads.detach().cpu())
    for k in PARAM_ORDER:
        r = ref[k].numpy()
        np.testing.assert_allclose(g[k].numpy().astype(np.float64), r.reshape(g[k].shape), rtol=rtol,
                                   atol=rtol * float(np.abs(r).max()) + 1e-8, err_msg=f"{what} {k}")


def star_rays_reenter(forward, centre, device) -> float:
    """Share of 90 rays from `centre` along which the region {out < 0} is re-entered after it was left (tests/test_gpu_teaser.py)."""
    t = torch.linspace(0.01, 0.7, 200, device=device)
    ang = torch.linspace(0, 2 * np.pi, 91, device=device)[:-1]
    pts = torch.stack((centre[0] + t[None, :] * torch.cos(ang)[:, None], centre[1] + t[None, :] * torch.sin(ang)[:, None]), -1).reshape(-1, 2)
    outside = (forward(pts.contiguous()).reshape(90, 200) >= 0).int()
    return float(((outside[:, 1:] - outside[:, :-1]).min(1).values < 0).float().mean())
