"""PathConnectedNet over ICNNs of the layer-by-layer path (n_hidden > 130 or more than two hidden layers) and the RealNVP's own
backward (`inrfit_rnvp_backward`), through the C ABI and the modules, against the oracle under torch autograd
(oracle/inr_oracle.py: pcn_deformation, pcn_forward, fit_pcn).

Shapes: the smallest at which the composition can go wrong - grids of 480 and 437 points (437: a multiple of neither 16 nor 64),
three 12x10 frames as an explicit (x, y, t) grid; ICNN 144 x 1 (the first width past the fused kernels), 131 x 2 (row stride 136
against k-steps of 16), 64 x 3 (deep but narrow), 160 x 2 at C = 3; RealNVP 32 hidden units, tanh, 4 flows at C = 2 / 6 at C = 3
(every mask specialisation), ActNorm initialised on the grid.

Bars: the fused shapes' bars of tests/test_gpu_rnvp.py (deformation, logits, loss, flow gradients, fit trajectory); for the ICNN
half's gradients the bars of tests/test_gpu_icnn.py::test_wide_and_deep_shapes_on_the_layer_by_layer_path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import inr_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = {"24x20": (24, 20), "23x19": (23, 19)}
SHAPES = [(2, 144, 1), (2, 131, 2), (2, 64, 3), (3, 160, 2)]   # (C, n_hidden, hidden layers)


@pytest.fixture(scope="module")
def dev():
    import awesome_amd._lib as L
    L.load()
    return torch.device("cuda:0")


def _n_flows(C):
    return 4 if C == 2 else 6


def _coords(C, key):
    """Planar coordinates (C, N) and the oracle's rows (N, C)."""
    if key == "frames":   # three frames of 12 x 10 as one explicit (x, y, t) grid
        g = torch.cat([O.positional_grid(10, 12, float(t), 2.0).reshape(3, -1) for t in range(3)], 1)
    else:
        H, W = GRIDS[key]
        g = (O.positional_grid(W, H) if C == 2 else O.positional_grid(W, H, 0.37, 1.0)).reshape(C, -1)
    return g.contiguous(), g.t().contiguous()


def _target(N, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return (torch.rand(N, generator=g) > 0.55).float()


def _case(C, h, layers, key, seed=0, dev=None):
    """A random PathConnectedNet state (every parameter non-trivial), ActNorm initialised on the grid by the oracle."""
    import awesome_amd as A
    from awesome_amd import rnvp as R
    from awesome_amd.model import ConvexNextNet
    torch.manual_seed(1000 * C + h + 7 * layers + seed)
    F = _n_flows(C)
    vmin, vmax = (-0.1, 0.0, -0.05)[:C], (1.2, 1.0, 1.1)[:C]
    rspec, ispec = R.RnvpSpec(C, 32, F, "tanh", None, vmin, vmax), A.IcnnSpec(h, C, layers)
    sd = {}
    for k, shp in rspec.keys_shapes():
        if k == "linear.weight":
            sd[k] = 1.0 + 0.2 * torch.randn(shp)
        elif k == "linear.bias":
            sd[k] = 0.1 * torch.randn(shp)
        elif k.endswith("net.0.weight"):
            sd[k] = torch.randn(shp) * 0.8
        elif k.endswith("net.0.bias"):
            sd[k] = torch.randn(shp) * 0.5
        elif k.endswith("net.2.weight"):
            sd[k] = torch.randn(shp) * 0.15
        elif k.endswith("net.2.bias"):
            sd[k] = torch.randn(shp) * 0.1
        else:
            sd[k] = torch.zeros(shp)
    for k, v in ConvexNextNet(n_hidden=h, n_hidden_layers=layers, in_features=C).state_dict().items():
        sd["convex_net." + k] = v.detach().clone()
    planar, rows = _coords(C, key)
    masks = O.rnvp_masks(C, F)
    O.pcn_deformation(sd, rows, masks, torch.tensor(vmin), torch.tensor(vmax), actnorm_init=True)
    return ispec, rspec, sd, planar, rows, masks


def _split(ispec, rspec, sd, dev):
    import awesome_amd as A
    from awesome_amd import rnvp as R
    ip = A.pack_state_dict(ispec, {k[len("convex_net."):]: v for k, v in sd.items() if k.startswith("convex_net.")}, dev)
    return ip[None].contiguous(), R.pack_rnvp_state_dict(rspec, sd, dev)[None].contiguous()


def _merge(ispec, rspec, gi, gf):
    import awesome_amd as A
    from awesome_amd import rnvp as R
    out = {"convex_net." + k: v for k, v in A.unpack_params(ispec, gi).items()}
    out.update(R.unpack_rnvp_params(rspec, gf))
    return out


def _check_grads(got, ref, what=""):
    """Flow half: the gradient bar of tests/test_gpu_rnvp.py; ICNN half: the bar of the layer-by-layer shapes (tests/test_gpu_icnn.py)."""
    worst = {}
    for k, r in ref.items():
        r, g = r.numpy(), got[k].numpy().reshape(r.shape)
        scale = float(np.abs(r).max())
        icnn = k.startswith("convex_net.")
        rtol, atol = (5e-4, 5e-6 * scale + 1e-10) if icnn else (1e-3, 3e-5 * scale + 1e-7)
        ratio = float((np.abs(g - r) / (atol + rtol * np.abs(r))).max())
        half = "icnn" if icnn else "flow"
        worst[half] = max(worst.get(half, 0.0), ratio)
    print(f"[grad error / bar] {what}: " + ", ".join(f"{h} {v:.3f}" for h, v in sorted(worst.items())))
    for k, r in ref.items():
        r, g = r.numpy(), got[k].numpy().reshape(r.shape)
        scale = float(np.abs(r).max())
        if k.startswith("convex_net."):
            np.testing.assert_allclose(g, r, rtol=5e-4, atol=5e-6 * scale + 1e-10, err_msg=f"{what} {k}")
        else:
            np.testing.assert_allclose(g, r, rtol=1e-3, atol=3e-5 * scale + 1e-7, err_msg=f"{what} {k}")


def _vt(rspec):
    return torch.tensor(rspec.vmin), torch.tensor(rspec.vmax)


# ---- 1. inrfit_rnvp_backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,key", [(2, "24x20"), (2, "23x19"), (3, "frames"), (3, "23x19")])
def test_rnvp_backward_against_autograd(dev, C, key):
    """flow_grads and din_coords for a random dout_coords, two images with different parameters in one call."""
    import awesome_amd as A
    from awesome_amd import rnvp as R
    cases = [_case(C, 64, 1, key, seed=s) for s in (0, 1)]
    ispec, rspec, _, planar, rows, masks = cases[0]
    N = planar.shape[1]
    dout = torch.randn(2, C, N, generator=torch.Generator().manual_seed(3))
    fp = torch.cat([_split(ispec, rspec, c[2], dev)[1] for c in cases])
    gf, din = R.rnvp_backward(rspec, fp, A.Grid.explicit(planar.to(dev)), dout.to(dev), want_dcoords=True)
    gf_only = R.rnvp_backward(rspec, fp, A.Grid.explicit(planar.to(dev)), dout.to(dev))
    assert torch.equal(gf_only, gf)
    vmin, vmax = _vt(rspec)
    for i, c in enumerate(cases):
        sdo = {k: v.clone().requires_grad_(True) for k, v in c[2].items() if not k.startswith("convex_net.")}
        x = rows.clone().requires_grad_(True)
        xd = O.pcn_deformation(sdo, x, masks, vmin, vmax)
        (xd * dout[i].t()).sum().backward()
        got = R.unpack_rnvp_params(rspec, gf[i].cpu())
        _check_grads(got, {k: v.grad for k, v in sdo.items()}, f"rnvp_backward C={C} {key} image {i}")
        ref = x.grad.t().numpy()
        np.testing.assert_allclose(din[i].cpu().numpy(), ref, rtol=1e-3, atol=3e-5 * float(np.abs(ref).max()) + 1e-7)


# ---- 2. consistency with the fused composite ---------------------------------------------------------------------------------
def test_seeded_backward_reproduces_the_fused_composite(dev):
    """h = 64, L = 1 has a fused kernel: rnvp_backward seeded with the dcoords inrfit_backward returns on the deformed grid gives the
    flow gradients of inrfit_pcn_loss_grad(external)."""
    import awesome_amd as A
    from awesome_amd import rnvp as R
    ispec, rspec, sd, planar, rows, masks = _case(2, 64, 1, "23x19")
    assert ispec.fused()
    ip, fp = _split(ispec, rspec, sd, dev)
    grid = A.Grid.explicit(planar.to(dev))
    dl = torch.randn(1, planar.shape[1], generator=torch.Generator().manual_seed(5)).to(dev)
    _, gi, gf = R.pcn_loss_grad(ispec, rspec, ip, fp, grid, dl, loss="external")
    xd = R.rnvp_forward(rspec, fp, grid)
    gi2, dxd = A.icnn.backward(ispec, ip, A.Grid.explicit(xd), dl, want_dcoords=True)
    gf2 = R.rnvp_backward(rspec, fp, grid, dxd)
    np.testing.assert_allclose(gi2.cpu().numpy(), gi.cpu().numpy(), rtol=1e-5, atol=1e-7)
    ref = R.unpack_rnvp_params(rspec, gf[0].cpu())
    _check_grads(R.unpack_rnvp_params(rspec, gf2[0].cpu()), ref, "seeded vs fused")


# ---- 3. forward and loss_grad of every shape -----------------------------------------------------------------------------------
def _shape_grids():
    out = []
    for C, h, L in SHAPES:
        for key in (("24x20", "23x19") if C == 2 else ("frames",)):
            out.append((C, h, L, key))
    return out


@pytest.mark.parametrize("C,h,layers,key", _shape_grids())
def test_forward_and_loss_grad(dev, C, h, layers, key):
    import awesome_amd as A
    from awesome_amd import rnvp as R
    ispec, rspec, sd, planar, rows, masks = _case(C, h, layers, key)
    assert not ispec.fused() and ispec.supported()
    N = planar.shape[1]
    vmin, vmax = _vt(rspec)
    ip, fp = _split(ispec, rspec, sd, dev)
    grid = A.Grid.explicit(planar.to(dev))
    yo = O.pcn_forward(sd, rows, masks, vmin, vmax)
    y = R.pcn_forward(ispec, rspec, ip, fp, grid)
    np.testing.assert_allclose(y[0].cpu().numpy(), yo.reshape(-1).numpy(), rtol=1e-4, atol=5e-5)
    un = _target(N)
    dl = torch.randn(N, generator=torch.Generator().manual_seed(9))
    for kind in ("se", "bce", "external"):
        sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        yo = O.pcn_forward(sdo, rows, masks, vmin, vmax)
        if kind == "external":
            lo = (yo.reshape(-1) * dl).sum()
            tgt = dl
        else:
            lo = O.weighted_loss(torch.sigmoid(yo).reshape(1, 1, -1, 1), un.reshape(1, 1, -1, 1), kind, "none")
            tgt = un
        lo.backward()
        loss, gi, gf = R.pcn_loss_grad(ispec, rspec, ip, fp, grid, tgt.reshape(1, -1).to(dev), loss=kind)
        if kind != "external":
            assert float(loss[0]) == pytest.approx(float(lo.detach()), rel=3e-5)
        _check_grads(_merge(ispec, rspec, gi[0].cpu(), gf[0].cpu()), {k: v.grad for k, v in sdo.items()}, f"{h}x{layers} C={C} {key} {kind}")


# ---- 4. the fit -------------------------------------------------------------------------------------------------------------
def _fit_case(dev, C=2, h=144, layers=1, key="23x19"):
    import awesome_amd as A
    ispec, rspec, sd, planar, rows, masks = _case(C, h, layers, key, seed=2)
    H, W = GRIDS[key]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    un = (((yy - 0.45 * H) ** 2 + (xx - 0.5 * W) ** 2) > 0.07 * H * W).float().reshape(-1)
    ip, fp = _split(ispec, rspec, sd, dev)
    return ispec, rspec, sd, rows, masks, un, ip, fp, A.Grid.explicit(planar.to(dev))


@pytest.mark.parametrize("optimizer,wd,h,layers", [("adamax", 1e-5, 144, 1), ("adam", 0.0, 131, 2), ("adamax", 1e-5, 64, 3)])
def test_fit_trajectory(dev, optimizer, wd, h, layers):
    """15 optimizer steps against the oracle's loop: loss history, both parameter halves, the final logits."""
    from awesome_amd import rnvp as R
    ispec, rspec, sd, rows, masks, un, ip, fp, grid = _fit_case(dev, h=h, layers=layers)
    vmin, vmax = _vt(rspec)
    pf, losses, logits = O.fit_pcn(sd, rows, un.reshape(-1, 1), 15, masks, vmin, vmax, lr=2e-3, optimizer=optimizer, flow_weight_decay=wd)
    res = R.pcn_fit(ispec, rspec, ip, fp, grid, un.reshape(1, -1).to(dev), 15, lr=2e-3, optimizer=optimizer, flow_weight_decay=wd)
    assert int(res.status[0]) == 0
    np.testing.assert_allclose(res.loss_hist[0].cpu().numpy(), np.asarray(losses, np.float32), rtol=5e-4)
    got = _merge(ispec, rspec, res.icnn_params[0].cpu(), res.flow_params[0].cpu())
    for k in pf:
        np.testing.assert_allclose(got[k].numpy(), pf[k].numpy(), rtol=5e-3, atol=3e-4, err_msg=k)
    np.testing.assert_allclose(res.logits[0].cpu().numpy(), logits.reshape(-1).numpy(), rtol=5e-3, atol=2e-3)
    for k, v in got.items():   # enforce_convexity after every step
        if k.startswith("convex_net.") and k.endswith("ln.weight") and not k.startswith("convex_net.input"):
            assert float(v.min()) >= 0.0, k


def test_fit_in_two_calls_equals_one_call(dev):
    """8 steps, then 7 with step0 = 8 and the returned optimizer states: bit for bit the 15-step fit (status == NULL is allowed:
    the second half of the library's own call sequence passes none through the C ABI below)."""
    import ctypes as C
    from awesome_amd import _lib as L
    from awesome_amd import icnn as K
    from awesome_amd import rnvp as R
    ispec, rspec, sd, rows, masks, un, ip, fp, grid = _fit_case(dev)
    t = un.reshape(1, -1).to(dev)
    kw = dict(lr=2e-3, optimizer="adamax", flow_weight_decay=1e-5, plateau=dict(patience=2, factor=0.5))
    one = R.pcn_fit(ispec, rspec, ip.clone(), fp.clone(), grid, t, 15, **kw)
    a = R.pcn_fit(ispec, rspec, ip.clone(), fp.clone(), grid, t, 8, **kw)
    b = R.pcn_fit(ispec, rspec, a.icnn_params, a.flow_params, grid, t, 7, icnn_opt_state=a.icnn_opt_state,
                  flow_opt_state=a.flow_opt_state, step0=8, **kw)
    assert torch.equal(b.icnn_params, one.icnn_params) and torch.equal(b.flow_params, one.flow_params)
    assert torch.equal(torch.cat([a.loss_hist, b.loss_hist], 1), one.loss_hist)
    assert torch.equal(b.logits, one.logits)
    # status == NULL, loss_hist == NULL, final_logits == NULL
    ip2, fp2 = ip.clone(), fp.clone()
    io, fo = K.new_opt_state(ispec, 1, dev), torch.zeros(1, 2 * rspec.n_params, device=dev)
    od = L.InrOptDesc(L.OPT_KINDS["adamax"], 2e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 2, 0.5, 1e-4, 0.0, 1e-8, 0, 0, 0)
    ws = R._ws(ispec, rspec, grid, 1)
    md, rd, gd, ld = ispec.desc(), rspec.desc(), grid.desc(), K._loss_desc("se", "none", 1.0, 0.0, 0.0)
    rc = L.load().inrfit_pcn_fit(C.byref(md), C.byref(rd), ip2.data_ptr(), fp2.data_ptr(), io.data_ptr(), fo.data_ptr(), C.byref(gd),
                                 t.data_ptr(), C.byref(ld), C.byref(od), 1e-5, 1, 15, 0, None, None, None, ws.data_ptr(), ws.numel() * 4,
                                 K._stream_ptr(dev))
    assert rc == 0
    assert torch.equal(ip2, one.icnn_params) and torch.equal(fp2, one.flow_params)


def test_plateau_reduces_the_learning_rate_of_both_halves(dev):
    """ReduceLROnPlateau(patience 2, factor 0.5) on a loss that stalls (a relative threshold no step reaches): the learning rate halves
    after steps 4, 7 and 10 for BOTH halves - the trajectory over the steps after the reductions matches the oracle's loop."""
    from awesome_amd import rnvp as R
    ispec, rspec, sd, rows, masks, un, ip, fp, grid = _fit_case(dev)
    vmin, vmax = _vt(rspec)
    pl = dict(patience=2, factor=0.5, threshold=0.9)
    pf, losses, _ = O.fit_pcn(sd, rows, un.reshape(-1, 1), 12, masks, vmin, vmax, lr=4e-3, optimizer="adamax", flow_weight_decay=1e-5, plateau=pl)
    pn, losses_n, _ = O.fit_pcn(sd, rows, un.reshape(-1, 1), 12, masks, vmin, vmax, lr=4e-3, optimizer="adamax", flow_weight_decay=1e-5)
    assert abs(losses[-1] - losses_n[-1]) > 20 * 5e-4 * losses[-1]   # the reductions are visible far above the bar
    res = R.pcn_fit(ispec, rspec, ip, fp, grid, un.reshape(1, -1).to(dev), 12, lr=4e-3, optimizer="adamax", flow_weight_decay=1e-5, plateau=pl)
    np.testing.assert_allclose(res.loss_hist[0].cpu().numpy(), np.asarray(losses, np.float32), rtol=5e-4)
    got = _merge(ispec, rspec, res.icnn_params[0].cpu(), res.flow_params[0].cpu())
    for k in pf:
        np.testing.assert_allclose(got[k].numpy(), pf[k].numpy(), rtol=5e-3, atol=3e-4, err_msg=k)
    hdr = res.icnn_opt_state[0, 2 * ispec.n_params:]
    assert float(hdr[2]) == pytest.approx(4e-3 * 0.5 ** 3, rel=1e-6)   # reduced after steps 4, 7 and 10 (the oracle's PlateauState)


# ---- 5. two images in one call ---------------------------------------------------------------------------------------------------
def test_two_images_nan_target_freezes_both_halves(dev):
    from awesome_amd import rnvp as R
    ispec, rspec, sd, rows, masks, un, ip, fp, grid = _fit_case(dev, h=131, layers=2)
    ip2, fp2 = ip.repeat(2, 1).contiguous(), fp.repeat(2, 1).contiguous()
    fp2[1, :2] *= 1.1   # (another deformation for image 1)
    t = un.reshape(1, -1).repeat(2, 1).to(dev)
    t[1, 17] = float("nan")
    kw = dict(lr=2e-3, optimizer="adamax", flow_weight_decay=1e-5)
    r1 = R.pcn_fit(ispec, rspec, ip2.clone(), fp2.clone(), grid, t, 6, **kw)
    r2 = R.pcn_fit(ispec, rspec, ip2.clone(), fp2.clone(), grid, t, 6, **kw)
    single = R.pcn_fit(ispec, rspec, ip2[:1].clone(), fp2[:1].clone(), grid, t[:1].contiguous(), 6, **kw)
    assert int(r1.status[0]) == 0 and int(r1.status[1]) != 0
    assert torch.equal(r1.icnn_params[1], ip2[1]) and torch.equal(r1.flow_params[1], fp2[1])   # frozen at the parameters before the step
    assert torch.equal(r1.icnn_params[0], single.icnn_params[0]) and torch.equal(r1.flow_params[0], single.flow_params[0])
    assert torch.equal(r1.loss_hist[0], single.loss_hist[0])
    assert not torch.equal(r1.icnn_params[0], ip2[0]) and not torch.equal(r1.flow_params[0], fp2[0])
    for a, b in ((r1.icnn_params, r2.icnn_params), (r1.flow_params, r2.flow_params), (r1.logits[0], r2.logits[0])):
        assert torch.equal(a, b)


# ---- 6. modules ------------------------------------------------------------------------------------------------------------------
def _module(dev, h=144, layers=3, seed=3):
    from awesome_amd.model import real_nvp_path_connected_net
    torch.manual_seed(seed)
    m = real_nvp_path_connected_net(channels=2, hidden_units=32, flow_n_flows=4, flow_output_fn="tanh", convex_net_hidden_units=h,
                                    convex_net_hidden_layers=layers).to(dev)
    with torch.no_grad():   # off the identity: every gradient non-trivial
        for k, p in m.named_parameters():
            if k.endswith("net.2.weight") or k.endswith("net.2.bias"):
                p.copy_(0.1 * torch.randn_like(p))
    return m


def _oracle_state(m):
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return sd, {k: v.clone().requires_grad_(True) for k, v in sd.items()
                if v.dtype == torch.float32 and not k.startswith("flow_net.norm") and not k.endswith("data_dep_init_done")}


def test_module_forward_backward(dev):
    """real_nvp_path_connected_net(convex_net_hidden_units=144, convex_net_hidden_layers=3): forward + backward of a scalar loss."""
    m = _module(dev)
    H, W = 23, 19
    grid_t = O.positional_grid(W, H)
    rows = O.pixelize(grid_t[None])
    un = torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(1))
    out = torch.sigmoid(m(grid_t[None].to(dev)))
    loss = ((out - un.to(dev)) ** 2).mean()
    loss.backward()
    sd, sdo = _oracle_state(m)
    masks = O.rnvp_masks(2, 4)
    lo = ((torch.sigmoid(O.pcn_forward(sdo, rows, masks, torch.zeros(2), torch.ones(2))).reshape(1, 1, H, W) - un) ** 2).mean()
    lo.backward()
    assert float(loss.detach()) == pytest.approx(float(lo.detach()), rel=3e-5)
    _check_grads({k: p.grad.cpu() for k, p in m.named_parameters()}, {k: sdo[k].grad for k, _ in m.named_parameters()}, "module 144x3")


def test_get_deformation_differentiable(dev):
    m = _module(dev, h=64, layers=1)
    H, W = 23, 19
    grid_t = O.positional_grid(W, H)
    x = grid_t[None].to(dev)
    plain = m.get_deformation(x)
    assert plain.grad_fn is None and not plain.requires_grad
    xg = x.clone().requires_grad_(True)
    xd = m.get_deformation(xg, differentiable=True)
    assert xd.grad_fn is not None and torch.equal(xd.detach(), plain)
    wgt = torch.randn(1, 2, H, W, generator=torch.Generator().manual_seed(2))
    (xd * wgt.to(dev)).sum().backward()
    sd, sdo = _oracle_state(m)
    rows = O.pixelize(grid_t[None]).clone().requires_grad_(True)
    xr = O.pcn_deformation(sdo, rows, O.rnvp_masks(2, 4), torch.zeros(2), torch.ones(2))
    np.testing.assert_allclose(plain[0].reshape(2, -1).cpu().numpy(), xr.detach().t().numpy(), rtol=3e-5, atol=5e-6)
    (xr * O.pixelize(wgt)).sum().backward()
    flow = {k: p.grad.cpu() for k, p in m.named_parameters() if not k.startswith("convex_net.")}
    assert all(p.grad is None for k, p in m.named_parameters() if k.startswith("convex_net."))
    _check_grads(flow, {k: sdo[k].grad for k in flow}, "get_deformation")
    ref = rows.grad.t().reshape(2, H, W).numpy()
    np.testing.assert_allclose(xg.grad[0].cpu().numpy(), ref, rtol=1e-3, atol=3e-5 * float(np.abs(ref).max()) + 1e-7)
    # rows layout (N, C) as well
    xr2 = m.get_deformation(O.pixelize(grid_t[None]).to(dev).requires_grad_(True), differentiable=True)
    assert xr2.shape == (H * W, 2) and xr2.grad_fn is not None


def test_fit_images_with_both_prefit_stages(dev):
    import awesome_amd as A
    from awesome_amd.model import real_nvp_path_connected_net
    torch.manual_seed(0)
    m = real_nvp_path_connected_net(channels=2, hidden_units=32, flow_n_flows=4, flow_output_fn="tanh", convex_net_hidden_units=144,
                                    convex_net_hidden_layers=1).to(dev)
    H, W = 24, 20
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    un = (((yy - 11) ** 2 + (xx - 9) ** 2) > 30).float().reshape(1, -1).to(dev)
    res = m.fit_images(A.Grid.linspace(W, H, dev), un, num_epochs=150, lr=2e-3, prefit_flow_net_identity=True,
                       prefit_flow_net_identity_num_epochs=20, prefit_convex_net=True, prefit_convex_net_num_epochs=40)
    assert int(res.status[0]) == 0 and torch.isfinite(res.loss_hist).all()
    assert float(res.loss_hist[0, -1]) < 0.5 * float(res.loss_hist[0, 0]) or float(A.miou(torch.sigmoid(res.logits), un)[0]) > 0.8


class _Agent:
    def __init__(self, ds, dev):
        self.training_dataset, self.device, self.logger = ds, dev, None


_PCN_ARGS = dict(channels=2, hidden_units=32, flow_n_flows=4, flow_output_fn="tanh", convex_net_hidden_units=144, convex_net_hidden_layers=1)


def test_wrapper_pretrain_fills_the_prior_cache(dev):
    """WrapperModule.pretrain on two small images (the synthetic data set is square: 22 x 22 = 484 points, a multiple of neither 16 nor
    64) returns a PriorCache state with both priors."""
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.model import ForwardModule, WrapperModule, real_nvp_path_connected_net
    torch.manual_seed(1)
    ds = SyntheticPriorDataset(n_images=2, size=22, kind="blob", prior_model_type=real_nvp_path_connected_net, prior_model_args=_PCN_ARGS)
    wrapper = WrapperModule(ForwardModule(), real_nvp_path_connected_net(**_PCN_ARGS), use_segmentation_output_inversion=True).to(dev)
    state = wrapper.pretrain(train_set=ds, test_set=None, device=dev, agent=_Agent(ds, dev), use_progress_bar=False, num_epochs=60, lr=2e-3,
                             reuse_state=False, proper_prior_fit_retrys=0)
    assert sorted(state["cache"]) == ["0", "1"] and state["model_type"].endswith("real_nvp_path_connected_net")
    assert json.loads(state["model_args"])["convex_net_hidden_units"] == 144
    for sd in state["cache"].values():
        assert sd["convex_net.skip.0.ln.weight"].shape == (144, 144)
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert not torch.equal(state["cache"]["0"]["convex_net.input.weight"], state["cache"]["1"]["convex_net.input.weight"])


def test_joint_trainer_takes_the_autograd_route(dev):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.measures import FBMSJointLoss
    from awesome_amd.model import WrapperModule, real_nvp_path_connected_net
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters

    class Seg(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)

        def forward(self, image, *args, **kwargs):
            return self.conv(image)

    torch.manual_seed(5)
    factory = lambda: real_nvp_path_connected_net(**_PCN_ARGS)   # noqa: E731
    ds = SyntheticPriorDataset(n_images=2, size=22, kind="noisy_blob")
    seg = Seg()
    wrapper = WrapperModule(seg, factory(), use_segmentation_output_inversion=True).to(dev)
    bank = PriorBank(lambda: factory().to(dev), n_images=2, device=dev)
    for k in range(2):
        bank.row(k)
    opt = torch.optim.Adam(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    tr = JointTrainer(wrapper, bank, FBMSJointLoss(alpha=1.0, beta=2.0), opt)
    assert tr.fused is False
    before = bank.params.detach().clone()
    (image, _, xy), target = ds[0]
    args = (image[None].to(dev), torch.zeros(1, 1, 1, 1, device=dev), xy[None].to(dev))
    l0, _ = tr.perform_step(0, args, target[None].to(dev))
    assert tr._path == "autograd" and torch.isfinite(l0)
    assert not torch.equal(bank.params[0], before[0]) and torch.equal(bank.params[1], before[1])


# ---- 7. the config ---------------------------------------------------------------------------------------------------------------
def test_run_py_path_connected_wide256(tmp_path):
    override = {"dataset_args": {"size": 32}, "agent_args": {"pretrain_args": {"num_epochs": 20, "prefit_flow_net_identity_num_epochs": 10,
                                                                                "prefit_convex_net_num_epochs": 10,
                                                                                "proper_prior_fit_retrys": 0}}}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--config-path",
                          os.path.join(ROOT, "config", "c2_blob256_path_connected_wide256.yaml"), "--output-folder", str(tmp_path),
                          "--override", json.dumps(override)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    summary = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert summary["images"] == 1 and summary["priors_saved"] == 1
    cache = torch.load(os.path.join(summary["output"], "prior_cache_epoch_0.pth"), weights_only=False)
    sd = cache["cache"]["0"]
    assert sd["convex_net.input.weight"].shape[0] == 256
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
