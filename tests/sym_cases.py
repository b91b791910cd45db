"""Shared cases of the rotation-symmetric prior's device fits (tests/test_gpu_symmetric.py, tests/test_symmetric_host.py): the shapes,
the per-step host loop the one call must equal bit for bit, the notebook's loop (rotation_symmetric.ipynb cell 3) restated on
oracle.inr_oracle's forward with autograd and O.adam_step in float64 / float32, and the pose's chain rule written out.

Every shape is the smallest that still crosses an edge: two images on the fused kernel (100 + 100), a batch that is no multiple of the
reduction block (96 + 96 = 192), the notebook's width on the layer-by-layer path, DataLoader batches with a short last one (64 / 64 /
3), and one full batch of 1440 points (six reduction blocks).  Six steps with the mirror switched on at step 3: inside the call."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from oracle import inr_oracle as O  # (checker only)
from tests.minibatch_cases import _balanced, _loader, _pixels, finite, parity_bound  # noqa: F401  (re-exported)

OFFSET, ORIENTATION = (0.013, -0.021), 0.3   # the initial pose of every case
SWITCH = 3                                   # symmetry_from_step
EPS = 0.001
MODULE_SEED, DRAW_SEED = 21, 3
MIN_V0, MIN_R = 1e-4, 1e-3                   # every drawn point keeps this far from the |v| kink and the 1 / r pole (float64 trajectory)


@dataclass
class Case:
    name: str
    modules: list                  # one per image (the initial parameters)
    pool_coords: torch.Tensor      # [2, n_pool]
    pool_targets: torch.Tensor     # [n_images, n_pool]
    index: Optional[torch.Tensor]  # [steps, batch] int32; None: full batch (sym_fit on the whole pool)
    counts: Optional[List[int]]
    kw: Dict = field(default_factory=dict)
    full_steps: int = 6

    @property
    def steps(self) -> int:
        return int(self.index.shape[0]) if self.index is not None else self.full_steps

    @property
    def n_images(self) -> int:
        return len(self.modules)

    def count(self, k: int) -> int:
        return int(self.counts[k]) if self.counts is not None else int(self.index.shape[1])

    def rows(self, k: int) -> torch.Tensor:
        if self.index is None:
            return torch.arange(self.pool_coords.shape[1])
        return self.index[k, :self.count(k)].long()


def likelihood(coords: torch.Tensor, cy: float = 0.03, cx: float = -0.04, ang: float = 0.4, shift: float = 0.0) -> torch.Tensor:
    """Mirror-symmetric about the axis through (cy, cx) at angle `ang`: two overlapping soft ellipses, one on each side of it.  No
    value within 0.02 of 0.5 (the class of a pixel is beyond rounding)."""
    import math
    a, b = coords[0] - cy, coords[1] - cx
    u = a * math.cos(ang) + b * math.sin(ang)
    v = -a * math.sin(ang) + b * math.cos(ang)
    d = ((u / 0.36) ** 2 + ((v.abs() - 0.08 - shift) / 0.19) ** 2).sqrt()
    lik = torch.sigmoid((1.0 - d) * 6.0)
    return torch.where((lik - 0.5).abs() < 0.02, lik + 0.05, lik).float()


def _modules(h: int, n: int = 1):
    from awesome_amd.model import RotationSymmetricNet
    torch.manual_seed(MODULE_SEED)
    mods = [RotationSymmetricNet(h) for _ in range(n)]
    for m in mods:
        with torch.no_grad():
            m.offset.copy_(torch.tensor([OFFSET]))
            m.orientation.fill_(ORIENTATION)
    return mods


def _class_kw(number: int) -> Dict:
    return dict(lr=1e-3, loss="se", weight_mode="explicit", c_fg=2.0 / number, c_bg=1.0 / number, symmetry_from_step=SWITCH)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    co = _pixels(36, 40)
    if name == "sym130x2":        # fused, two images with their own targets, 100 + 100
        tg = torch.stack([likelihood(co), likelihood(co, shift=0.03)])
        return Case(name, _modules(130, 2), co, tg, _balanced(tg[0], 6, 100, DRAW_SEED), None, _class_kw(100))
    if name == "sym32":           # fused, 192 points: the reduction block's tail
        tg = likelihood(co)[None]
        return Case(name, _modules(32), co, tg, _balanced(tg[0], 6, 96, DRAW_SEED), None, _class_kw(96))
    if name == "sym32_wd":        # weight decay: one Adam over pose and network decays both
        tg = likelihood(co)[None]
        return Case(name, _modules(32), co, tg, _balanced(tg[0], 6, 96, DRAW_SEED), None, dict(_class_kw(96), weight_decay=0.05))
    if name == "sym150":          # layer by layer, the notebook's width
        tg = likelihood(co)[None]
        return Case(name, _modules(150), co, tg, _balanced(tg[0], 6, 100, DRAW_SEED), None, _class_kw(100))
    if name == "sym150_loader":   # pool 131, batches 64 / 64 / 3, two epochs, the plain mean
        sub = _pixels(12, 11)[:, :131].contiguous()
        index, counts = _loader(131, 64, 2, DRAW_SEED)
        return Case(name, _modules(150), sub, likelihood(sub)[None], index, counts, dict(lr=1e-3, loss="se", symmetry_from_step=SWITCH))
    if name == "sym130_full":     # sym_fit on all 1440 points: six reduction blocks, added in block order
        return Case(name, _modules(130), co, likelihood(co)[None], None, None,
                    dict(lr=1e-3, loss="se", weight_mode="explicit", c_fg=2.0 / 1440, c_bg=1.0 / 1440, symmetry_from_step=SWITCH))
    raise KeyError(name)


MINIBATCH_CASES = ["sym130x2", "sym32", "sym150", "sym150_loader"]
ALL_CASES = MINIBATCH_CASES + ["sym130_full", "sym32_wd"]


# ---- device side --------------------------------------------------------------------------------------------------------------------------
def spec(c: Case):
    return c.modules[0].spec


def initial(c: Case, dev):
    """-> (params [n, P], pose [n, 3]) on the device."""
    prm = torch.stack([m.flat_parameters() for m in c.modules]).to(dev).contiguous()
    pose = torch.stack([m._pose() for m in c.modules]).to(dev).contiguous()
    return prm, pose


def device_call(c: Case, dev, rows=None, state=None, index=None, targets=None, coords=None):
    """The one call on rows [a, b) of the case's table (the full-batch case: steps a .. b) -> SymFitResult."""
    import awesome_amd as A
    import awesome_amd.symmetric as SY
    a, b = rows if rows is not None else (0, c.steps)
    prm, pose, opt, popt = state if state is not None else (*initial(c, dev), None, None)
    co = (c.pool_coords if coords is None else coords).to(dev)
    tg = (c.pool_targets if targets is None else targets).to(dev)
    if c.index is None:
        return SY.sym_fit(spec(c), prm, pose, A.Grid.explicit(co), tg, b - a, opt_state=opt, pose_opt_state=popt, step0=a, **c.kw)
    table = (c.index if index is None else index)[a:b]
    counts = c.counts[a:b] if c.counts is not None else None
    return SY.sym_fit_minibatch(spec(c), prm, pose, co, tg, table, counts, opt_state=opt, pose_opt_state=popt, step0=a, **c.kw)


def host_loop(c: Case, dev, steps=None):
    """The loop the one call replaces: per step a gather on the host side and one sym_fit(steps=1, step0=k) call."""
    import awesome_amd as A
    import awesome_amd.symmetric as SY
    prm, pose = initial(c, dev)
    opt = popt = None
    co, tg = c.pool_coords.to(dev), c.pool_targets.to(dev)
    hist = []
    for k in range(c.steps if steps is None else steps):
        idx = c.rows(k).to(dev)
        r = SY.sym_fit(spec(c), prm, pose, A.Grid.explicit(co[:, idx].contiguous()), tg[:, idx].contiguous(), 1, opt_state=opt,
                       pose_opt_state=popt, step0=k, **c.kw)
        opt, popt = r.opt_state, r.pose_opt_state
        hist.append(r.loss_hist[:, 0].clone())
    return prm, pose, opt, popt, torch.stack(hist, 1)


# ---- the notebook's loop on the oracle's forward (CPU) --------------------------------------------------------------------------------------
def oracle_state(m, dtype) -> Dict[str, torch.Tensor]:
    return {k: v.detach().clone().to(dtype) for k, v in m.state_dict().items()}


def to_flat(sp, p: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The network of the oracle's state in the library's flat order (the skip weights: zeros)."""
    z = lambda *s: torch.zeros(*s, dtype=p["W0.weight"].dtype)  # noqa: E731
    q = {"input.weight": p["W0.weight"], "input.bias": p["W0.bias"], "skip.0.ln.weight": p["W1.weight"], "skip.0.ln.bias": p["W1.bias"],
         "skip.0.skp.weight": z(sp.n_hidden, 3), "out.ln.weight": p["W2.weight"], "out.ln.bias": p["W2.bias"], "out.skp.weight": z(1, 3)}
    return torch.cat([q[k].detach().reshape(-1) for k, _ in sp.keys_shapes()])


def learned(sp) -> torch.Tensor:
    """[P] bool: the flat entries the notebook's net has (the ICNN layout's skip weights are constants of value 0, frozen in the fits;
    the library still reports d loss / d skip for them, which no reference has)."""
    return torch.cat([torch.full((int(torch.tensor(shp).prod()),), ".skp." not in k) for k, shp in sp.keys_shapes()])


def to_pose(p: Dict[str, torch.Tensor]) -> torch.Tensor:
    return torch.cat([p["offset"].detach().reshape(-1), p["orientation"].detach().reshape(-1)])


def loss_of(kw: Dict, prob: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    el = (prob - t) ** 2
    if kw.get("weight_mode", "none") == "explicit":
        return (torch.where(t < 0.5, torch.full_like(t, kw["c_fg"]), torch.full_like(t, kw["c_bg"])) * el).sum()
    return el.mean()


def reference_loop(c: Case, dtype, steps=None):
    """-> (network flats [n, P], poses [n, 3], losses [n, steps], min |v0| and min r over every drawn point of every step) of the
    notebook's loop in `dtype`: gather, forward with the switch, loss, autograd, ONE Adam over pose and network."""
    steps = c.steps if steps is None else steps
    co = c.pool_coords.to(dtype)
    flats, poses, hists, min_v0, min_r = [], [], [], float("inf"), float("inf")
    for img, m in enumerate(c.modules):
        tg = c.pool_targets[img].to(dtype)
        p = {k: v.requires_grad_(True) for k, v in oracle_state(m, dtype).items()}
        st = O.AdamState(p)
        hist = []
        for k in range(steps):
            idx = c.rows(k)
            x = co[:, idx].t()
            with torch.no_grad():
                f = O.rotation_symmetric_features(x, p["offset"], p["orientation"], False)
                min_v0, min_r = min(min_v0, float(f[:, 1].abs().min())), min(min_r, float(f[:, 2].min()))
            for v in p.values():
                v.grad = None
            loss = loss_of(c.kw, torch.sigmoid(O.rotation_symmetric_forward(p, x, k >= SWITCH))[:, 0], tg[idx])
            loss.backward()
            O.adam_step(p, {n: v.grad for n, v in p.items()}, st, c.kw["lr"], weight_decay=c.kw.get("weight_decay", 0.0))
            hist.append(float(loss.detach()))
        flats.append(to_flat(spec(c), p))
        poses.append(to_pose(p))
        hists.append(torch.tensor(hist, dtype=torch.float64))
    return torch.stack(flats), torch.stack(poses), torch.stack(hists), min_v0, min_r


@functools.lru_cache(maxsize=None)
def references(name: str):
    """Computed once, shared, never changed: float64 (network, pose, losses), e32 of each, (min |v0|, min r)."""
    c = case(name)
    f64, q64, h64, mv, mr = reference_loop(c, torch.float64)
    f32, q32, h32, _, _ = reference_loop(c, torch.float32)
    e = lambda a, b: float((a.double() - b).abs().max())  # noqa: E731
    return dict(net=f64, pose=q64, hist=h64, e_net=e(f32, f64), e_pose=e(q32, q64), e_hist=e(h32, h64), min_v0=mv, min_r=mr)


# ---- one loss and its gradients (GPU test 1) ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gradient_reference(h: int, n: int, sym: bool):
    """The plain mean MSE of the first n pool pixels under the initial pose: float64 autograd (loss, network gradient in flat order,
    pose gradient), the float32 autograd's distance from each, and (min |v0|, min r)."""
    m = _modules(h)[0]
    co = _pixels(36, 40)[:, :n]
    tg = likelihood(_pixels(36, 40))[:n]
    out = {}
    for dtype in (torch.float64, torch.float32):
        p = {k: v.requires_grad_(True) for k, v in oracle_state(m, dtype).items()}
        x = co.to(dtype).t()
        loss = ((torch.sigmoid(O.rotation_symmetric_forward(p, x, sym))[:, 0] - tg.to(dtype)) ** 2).mean()
        loss.backward()
        g = {k: v.grad for k, v in p.items()}
        out[dtype] = (loss.detach().double(), to_flat(m.spec, g).double(), to_pose(g).double())
        if dtype == torch.float64:
            f = O.rotation_symmetric_features(x, p["offset"], p["orientation"], False).detach()
            cond = (float(f[:, 1].abs().min()), float(f[:, 2].min()))
    (l64, g64, q64), (l32, g32, q32) = out[torch.float64], out[torch.float32]
    return dict(module=m, coords=co, targets=tg, loss=l64, net=g64, pose=q64, e_loss=float((l32 - l64).abs()),
                e_net=float((g32 - g64).abs().max()), e_pose=float((q32 - q64).abs().max()), min_v0=cond[0], min_r=cond[1])


# ---- the pose's chain rule, as csrc/sym.h computes it ---------------------------------------------------------------------------------------
def pose_gradient(x: torch.Tensor, offset: torch.Tensor, orientation: torch.Tensor, g: torch.Tensor, sym: bool, eps: float = EPS):
    """x (N, 2), g (N, 3) = dL / d(u, v, r) -> (d offset (2,), d orientation ()).  A point with r == 0 contributes nothing."""
    xp = x + offset.reshape(1, 2)
    r = (xp * xp).sum(1).sqrt()
    q = 1.0 / (eps + r)
    n = q[:, None] * xp
    c, s = torch.cos(orientation.reshape(())), torch.sin(orientation.reshape(()))
    u, v0 = n[:, 0] * c - n[:, 1] * s, n[:, 0] * s + n[:, 1] * c
    gu, gv, gr = g[:, 0], g[:, 1], g[:, 2]
    gv0 = torch.sign(v0) * gv if sym else gv
    ok = r > 0
    dth = torch.where(ok, gv0 * u - gu * v0, torch.zeros_like(r)).sum()
    gn = torch.stack((gu * c + gv0 * s, -gu * s + gv0 * c), 1)
    rs = torch.where(ok, r, torch.ones_like(r))
    gx = q[:, None] * gn - (q * q * (gn * xp).sum(1) / rs)[:, None] * xp + (gr / rs)[:, None] * xp
    return torch.where(ok[:, None], gx, torch.zeros_like(gx)).sum(0), dth
