"""Shared cases of the pixel-minibatch fits (tests/test_gpu_minibatch.py, tests/test_minibatch_host.py): the shapes, the per-step host
loop the device call must equal bit for bit, and the notebooks' loop restated on oracle.inr_oracle's forwards in float64 / float32.

Every shape is the smallest at which the gather, the staging alignment, the count change or the step bookkeeping can go wrong: a batch
that is no multiple of a chunk (200), an odd one (67: staging planes start unaligned), DataLoader batches with a short last one (64 /
64 / 22 and 64 / 64 / 3), two images with their own targets, three output planes."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import inr_oracle as O  # (checker only)


@dataclass
class Case:
    name: str
    kind: str                      # 'icnn' | 'fourier' | 'flow'
    modules: list                  # one per image (the initial parameters)
    pool_coords: torch.Tensor      # [C, n_pool]
    pool_targets: torch.Tensor     # [n_images, n_pool] / [n_images, O, n_pool]
    index: torch.Tensor            # [steps, batch] int32
    counts: Optional[List[int]]
    kw: Dict = field(default_factory=dict)   # the fit's keyword arguments

    @property
    def steps(self) -> int:
        return int(self.index.shape[0])

    @property
    def n_images(self) -> int:
        return len(self.modules)

    def count(self, k: int) -> int:
        return int(self.counts[k]) if self.counts is not None else int(self.index.shape[1])


def _pixels(h: int, w: int, c: int = 2) -> torch.Tensor:
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    rows = [yy.reshape(-1) / h - 0.5, xx.reshape(-1) / w - 0.5]
    if c == 3:
        rows.append(((yy * w + xx).reshape(-1) % 7) / 7.0)
    return torch.stack(rows, 0).float().contiguous()


def _likelihood(coords: torch.Tensor, cy: float, cx: float, r: float) -> torch.Tensor:
    """A soft disc, no value within 0.02 of 0.5 (the class of a pixel is beyond rounding)."""
    d = ((coords[0] - cy) ** 2 + (coords[1] - cx) ** 2).sqrt()
    lik = torch.sigmoid((d - r) * 12.0)
    return torch.where((lik - 0.5).abs() < 0.02, lik + 0.05, lik).float()


def _balanced(labels: torch.Tensor, steps: int, number: int, seed: int) -> torch.Tensor:
    from awesome_amd.minibatch import class_balanced_batches
    return class_balanced_batches(labels, steps, number, torch.Generator().manual_seed(seed))


def _loader(n: int, batch: int, epochs: int, seed: int):
    from awesome_amd.minibatch import dataloader_batches
    index, counts = dataloader_batches(n, batch, epochs, torch.Generator().manual_seed(seed))
    return index, counts.tolist()


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    from awesome_amd.model import ConvexDiffeomorphismNet, ConvexNet, ConvexNextNet, FourierFeatureNet
    if name == "fused130":       # two images, 100 + 100 of 1440 pixels, 2 MSE(bg) + 1 MSE(fg)
        torch.manual_seed(11)
        mods = [ConvexNextNet(130, 2, 1, 1), ConvexNextNet(130, 2, 1, 1)]
        co = _pixels(36, 40)
        tg = torch.stack([_likelihood(co, 0.05, -0.1, 0.3), _likelihood(co, -0.1, 0.1, 0.25)])
        return Case(name, "icnn", mods, co, tg, _balanced(tg[0], 12, 100, 5), None,
                    dict(lr=1e-2, loss="se", weight_mode="explicit", c_fg=2 / 100, c_bg=1 / 100, optimizer="adam", clamp=True))
    if name == "depth50":        # the depth notebook's net (padded width, C = 3): DataLoader batches, a learning rate that changes
        torch.manual_seed(12)
        co = _pixels(10, 15, 3)
        index, counts = _loader(150, 64, 2, 6)
        return Case(name, "icnn", [ConvexNextNet(50, 3, 1, 1)], co, _likelihood(co, 0.0, 0.0, 0.3)[None], index, counts,
                    dict(lr=1e-2, loss="se", optimizer="adamax", clamp=True, plateau=dict(patience=1, factor=0.5, threshold=0.5)))
    if name == "fused130x2":     # two hidden layers, an odd batch
        torch.manual_seed(13)
        co = _pixels(15, 20)
        g = torch.Generator().manual_seed(7)
        index = torch.stack([torch.randperm(300, generator=g)[:67] for _ in range(4)]).to(torch.int32)
        return Case(name, "icnn", [ConvexNextNet(130, 2, 1, 2)], co, _likelihood(co, 0.0, 0.05, 0.3)[None], index, None,
                    dict(lr=1e-2, loss="bce", optimizer="adam", clamp=True))
    if name == "convexnet150":   # layer by layer, class-balanced
        torch.manual_seed(14)
        co = _pixels(36, 40)
        tg = _likelihood(co, 0.0, 0.0, 0.3)[None]
        return Case(name, "icnn", [ConvexNet(n_hidden=150)], co, tg, _balanced(tg[0], 5, 96, 8), None,
                    dict(lr=1e-2, loss="se", weight_mode="explicit", c_fg=1 / 96, c_bg=1 / 96, optimizer="adam", clamp=True))
    if name == "convexnet150_loader":   # layer by layer, batches 64 / 64 / 3
        torch.manual_seed(15)
        co = _pixels(1, 131)
        co[0] = torch.linspace(-0.5, 0.5, 131)
        index, counts = _loader(131, 64, 2, 9)
        return Case(name, "icnn", [ConvexNet(n_hidden=150)], co, _likelihood(co, 0.0, 0.0, 0.3)[None], index, counts,
                    dict(lr=1e-2, loss="se", optimizer="adam", clamp=True))
    if name == "fourier":        # frozen features, three output planes, the mean over O x count
        torch.manual_seed(16)
        m = FourierFeatureNet(d_in=2, n_hidden=48, n_hidden_layers=3, factor=3.0, d_features=20, d_out=3)
        co = _pixels(10, 15)
        tg = torch.stack([_likelihood(co, 0.0, 0.0, 0.3), _likelihood(co, 0.2, -0.2, 0.2), _likelihood(co, -0.2, 0.1, 0.35)])[None]
        index, counts = _loader(150, 64, 2, 10)
        return Case(name, "fourier", [m], co, tg.contiguous(), index, counts,
                    dict(lr=1e-3, loss="se", optimizer="adam", **FourierFeatureNet.fit_options))
    if name == "flow":           # ICNN(flow(Ax + b)), 2 BCE(bg) + 1 BCE(fg), Adam over everything, no projection
        torch.manual_seed(17)
        m = ConvexDiffeomorphismNet(n_hidden=130, n_hidden_layers=1, nf_layers=2, nf_hidden=16, diffeo_args=dict(backbone="normal_block"))
        co = _pixels(36, 40)
        tg = _likelihood(co, 0.0, 0.05, 0.3)[None]
        return Case(name, "flow", [m], co, tg, _balanced(tg[0], 5, 100, 11), None,
                    dict(lr=1e-2, loss="bce", weight_mode="explicit", c_fg=2 / 100, c_bg=1 / 100, clamp=False, weight_decay_on_weight_g=0.0))
    raise KeyError(name)


BIT_CASES = ["fused130", "depth50", "fused130x2", "convexnet150", "convexnet150_loader", "fourier", "flow"]
PARITY_CASES = ["fused130", "convexnet150", "convexnet150_loader", "fourier", "flow"]   # the convex, Fourier and flow cases
BIT_STEPS = {"fused130": 6}   # (its table holds 12 rows: the continuation test takes all of them)


# ---- device side: flat parameters, the one call, the per-step host loop -----------------------------------------------------------
def specs(c: Case):
    m = c.modules[0]
    return m._specs() if c.kind == "flow" else (m.spec, None)


def initial(c: Case, dev):
    """-> [icnn params [n, P], flow params [n, FP] or None] on the device."""
    ispec, fspec = specs(c)
    if c.kind == "flow":
        import awesome_amd.flow as FL
        pairs = [FL.split_cdn_state_dict(ispec, fspec, m.state_dict()) for m in c.modules]
        return [torch.stack([p[0] for p in pairs]).to(dev).contiguous(), torch.stack([p[1] for p in pairs]).to(dev).contiguous()]
    return [torch.stack([m.flat_parameters() for m in c.modules]).to(dev).contiguous(), None]


def device_call(c: Case, dev, rows=None, state=None, index=None):
    """The minibatch fit on rows [a, b) of the case's table; -> (params list, opt states list, loss_hist [n, b - a], status)."""
    import awesome_amd.minibatch as MB
    ispec, fspec = specs(c)
    a, b = rows if rows is not None else (0, BIT_STEPS.get(c.name, c.steps))
    table = (c.index if index is None else index)[a:b]
    counts = c.counts[a:b] if c.counts is not None else None
    prm, opt = state if state is not None else (initial(c, dev), [None, None])
    co, tg = c.pool_coords.to(dev), c.pool_targets.to(dev)
    if c.kind == "flow":
        r = MB.cdn_fit_minibatch(ispec, fspec, prm[0], prm[1], co, tg, table, counts, icnn_opt_state=opt[0], flow_opt_state=opt[1],
                                 step0=a, **c.kw)
        return [r.icnn_params, r.flow_params], [r.icnn_opt_state, r.flow_opt_state], r.loss_hist, r.status
    r = MB.fit_minibatch(ispec, prm[0], co, tg, table, counts, opt_state=opt[0], step0=a, **c.kw)
    return [r.params, None], [r.opt_state, None], r.loss_hist, r.status


def host_loop(c: Case, dev, steps=None):
    """The loop the device call replaces: per step a gather on the host side, an explicit grid and one fit(steps=1, step0=k) call."""
    import awesome_amd as A
    import awesome_amd.flow as FL
    ispec, fspec = specs(c)
    prm, opt = initial(c, dev), [None, None]
    co, tg = c.pool_coords.to(dev), c.pool_targets.to(dev)
    hist = []
    for k in range(BIT_STEPS.get(c.name, c.steps) if steps is None else steps):
        idx = c.index[k, :c.count(k)].long().to(dev)
        grid = A.Grid.explicit(co[:, idx].contiguous())
        t = tg[..., idx].contiguous()
        if c.kind == "flow":
            r = FL.cdn_fit(ispec, fspec, prm[0], prm[1], grid, t, 1, icnn_opt_state=opt[0], flow_opt_state=opt[1], step0=k,
                           want_logits=False, **c.kw)
            opt = [r.icnn_opt_state, r.flow_opt_state]
        else:
            r = A.fit(ispec, prm[0], grid, t, 1, opt_state=opt[0], step0=k, want_logits=False, **c.kw)
            opt = [r.opt_state, None]
        hist.append(r.loss_hist[:, 0].clone())
    return prm, opt, torch.stack(hist, 1)


# ---- the notebooks' loop restated on the oracle's forwards (CPU) ------------------------------------------------------------------
def _flat_keys(c: Case) -> List[str]:
    ispec, fspec = specs(c)
    if c.kind == "flow":
        return ["convex_net." + k for k, _ in ispec.keys_shapes()] + [k for k, _ in fspec.keys_shapes()]
    return [k for k, _ in ispec.keys_shapes()]


def _oracle_state(c: Case, m, dtype) -> Dict[str, torch.Tensor]:
    sd = {k: v.detach().clone().to(dtype) for k, v in m.state_dict().items()}
    if c.kind == "icnn":
        return O.to_convexnext_keys(sd)
    if c.kind == "fourier":   # ourSimpleNetwork's names: the head is its last fcK
        n = m.spec.n_layers
        return {(f"fc{n + 1}" + k[3:] if k.startswith("out.") else k): v for k, v in sd.items()}
    return sd


def _to_flat(c: Case, p: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The oracle's state in the library's flat order (dtype kept)."""
    if c.kind == "fourier":
        spec = specs(c)[0]
        z = lambda *s: torch.zeros(*s, dtype=p["A"].dtype)  # noqa: E731
        q = {"input.weight": p["A"].t(), "input.bias": p["b"]}
        for k in range(spec.n_layers):
            q[f"skip.{k}.ln.weight"], q[f"skip.{k}.ln.bias"] = p[f"fc{k + 1}.weight"], p[f"fc{k + 1}.bias"]
            q[f"skip.{k}.skp.weight"] = z(spec.n_hidden, spec.in_features)
        q["out.ln.weight"], q["out.ln.bias"] = p[f"fc{spec.n_layers + 1}.weight"], p[f"fc{spec.n_layers + 1}.bias"]
        q["out.skp.weight"] = z(spec.n_out, spec.in_features)
        p = q
    return torch.cat([p[k].detach().reshape(-1) for k in _flat_keys(c)])


def _probabilities(c: Case, p, x):
    """(N, O) probabilities of the net on rows x."""
    if c.kind == "icnn":
        return torch.sigmoid(O.icnn_forward(p, x))
    if c.kind == "fourier":
        return O.fourier_mlp_forward(p, x)   # (the notebook's forward ends in the sigmoid)
    return torch.sigmoid(O.convex_diffeo_forward(p, x, specs(c)[1].num_coupling))


def _loss(c: Case, prob: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """prob, t (N, O).  'explicit': sum of c_fg l over the targets < 0.5 and c_bg l over the others; else the mean over O x N."""
    kw = c.kw
    el = (prob - t) ** 2 if kw["loss"] == "se" else F.binary_cross_entropy(prob, t, reduction="none")
    if kw.get("weight_mode", "none") == "explicit":
        w = torch.where(t < 0.5, torch.full_like(t, kw["c_fg"]), torch.full_like(t, kw["c_bg"]))
        return (w * el).sum()
    return el.mean()


def reference_loop(c: Case, dtype, steps=None):
    """-> (flat parameters [n_images, P (+ FP)], loss history [n_images, steps], learning rates [steps]) of the notebook's loop in
    `dtype` on the CPU: gather, forward, loss, backward, Adam / Adamax, projection, ReduceLROnPlateau."""
    kw = c.kw
    steps = BIT_STEPS.get(c.name, c.steps) if steps is None else steps
    co = c.pool_coords.to(dtype)
    flats, hists, lrs = [], [], []
    for img, m in enumerate(c.modules):
        tg = c.pool_targets[img].to(dtype).reshape(-1, c.pool_coords.shape[1])   # [O, n_pool]
        p = _oracle_state(c, m, dtype)
        frozen = {"A", "b"} if c.kind == "fourier" else set()
        learn = {k: v.requires_grad_(True) for k, v in p.items() if k not in frozen}
        st = O.AdamState(learn)
        sched = O.PlateauState(kw["lr"], **kw["plateau"]) if kw.get("plateau") else None
        lr, hist, lrs = kw["lr"], [], []
        for k in range(steps):
            idx = c.index[k, :c.count(k)].long()
            for v in learn.values():
                v.grad = None
            loss = _loss(c, _probabilities(c, p, co[:, idx].t()), tg[:, idx].t())
            loss.backward()
            g = {n: v.grad for n, v in learn.items()}
            lrs.append(lr)
            (O.adamax_step if kw.get("optimizer", "adam") == "adamax" else O.adam_step)(learn, g, st, lr)
            if kw.get("clamp", False):
                with torch.no_grad():
                    for n in learn:
                        if n.endswith("ln.weight") and not n.startswith("input"):
                            learn[n].copy_(F.relu(learn[n]))
            hist.append(float(loss.detach()))
            if sched is not None:
                lr = sched.step(hist[-1])
        flats.append(_to_flat(c, p))
        hists.append(torch.tensor(hist, dtype=torch.float64))
    return torch.stack(flats), torch.stack(hists), lrs


@functools.lru_cache(maxsize=None)
def references(name: str):
    """Computed once, shared, never changed: (f64 params, f64 losses, e32 of the params, e32 of the losses, learning rates)."""
    c = case(name)
    p64, h64, lrs = reference_loop(c, torch.float64)
    p32, h32, _ = reference_loop(c, torch.float32)
    e_p = float((p32.double() - p64).abs().max())
    e_h = float((h32 - h64).abs().max())
    return p64, h64, e_p, e_h, lrs


def parity_bound(e32: float, ref64: torch.Tensor) -> float:
    """4 e32 + 1e-6 max|f64|: e32 is the float32 restatement's own distance from float64 - what rounding every operation to float32 costs
    at this shape in one order of summation; another order (the kernels') may cost a few times that."""
    return 4.0 * e32 + 1e-6 * float(ref64.abs().max())


def finite(*ts) -> bool:
    return all(bool(torch.isfinite(t).all()) for t in ts)
