"""ConvexDiffeomorphismNet over ICNNs of the layer-by-layer path (n_hidden > 130 or more than two hidden layers): the coupling flow in
front of csrc/wide.h, through the C ABI (inrfit_cdn_forward / _loss_grad / _fit / _wide_fit_minibatch) and the module, against the
oracle under float32 torch autograd (oracle/inr_oracle.py: flow1d_forward, convex_diffeo_forward, fit_convex_diffeo).

Shapes: the smallest at which the composition can go wrong - grids of 24 x 20 (480 points) and 23 x 19 (437 points: a multiple of
neither 16 nor 64); ICNN 144 x 1 (the first width past the fused kernels), 131 x 2 (row stride 136 against k-steps of 16), 64 x 3 (deep
but narrow); 4 couplings of width 24 with both per-point backbones; every parameter away from its initial value, weight_g != 1.

Bars: the flow side (deformed coordinates, logits, loss, flow gradients, the fit's trajectory) takes the bars of
tests/test_gpu_flow.py::test_hip_flow_forward_and_cdn_gradients and ::test_hip_cdn_fit_trajectory; the ICNN half's gradients take the
bars of tests/test_gpu_icnn.py::test_wide_and_deep_shapes_on_the_layer_by_layer_path (as tests/test_gpu_pcn_wide.py does).

One borrowed bar does not hold, for the float32 oracle itself (profiles/cdn_wide_parity.md): `scale.<i>.scale.weight_v`, the 1 x 1
weight_v of a weight-normed scale, has an exactly zero gradient (g v / |v| does not depend on a scalar v's size).  float32 autograd
leaves an ulp of rounding there, and Adam turns that into steps of up to lr, so the oracle's own float32 run leaves its float64 run by
up to 6e-3 in 12 steps.  Those entries are compared with the FLOAT64 oracle, within the borrowed bar's absolute floor (for a gradient
1e-7 and four ulps of the two terms that cancel, _cancellation_floor; 3e-4 for a fitted parameter) + 4 e32 + 1e-6 max|float64|, e32 = the float32 oracle's distance from the float64 one over
those entries of the case (the form of tests/minibatch_cases.py::parity_bound)."""
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
SHAPES = [(144, 1), (131, 2), (64, 3)]   # (n_hidden, hidden layers)
K, WIDTH = 4, 24
EUNSUPPORTED = -2


@pytest.fixture(scope="module")
def dev():
    import awesome_amd._lib as L
    L.load()
    return torch.device("cuda:0")


def _case(h, layers, backbone="normal_block", seed=0):
    """(ispec, fspec, state_dict) of a ConvexDiffeomorphismNet with every parameter moved off its initial value."""
    import awesome_amd as A
    from awesome_amd import flow as FL
    from awesome_amd.model import ConvexDiffeomorphismNet
    torch.manual_seed(100 * h + 7 * layers + seed)
    m = ConvexDiffeomorphismNet(n_hidden=h, n_hidden_layers=layers, nf_layers=K, nf_hidden=WIDTH, in_features=2,
                                diffeo_args=dict(backbone=backbone))
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("weight_g") or "scale" in k:
                p.mul_(1.0 + 0.2 * torch.rand_like(p) + 0.05)
            elif k == "linear.bias":
                p.add_(0.1 * torch.randn_like(p))
            elif not k.startswith("convex_net."):
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return A.IcnnSpec(h, 2, layers), FL.FlowSpec(WIDTH, K, backbone), sd


def _split(ispec, fspec, sd, dev):
    from awesome_amd import flow as FL
    ip, fp = FL.split_cdn_state_dict(ispec, fspec, sd, dev)
    return ip[None].contiguous(), fp[None].contiguous()


def _grid(key, dev):
    """(explicit device grid (2, N), shared by every image of a call; oracle rows (N, 2); image grid (1, 2, H, W))."""
    import awesome_amd as A
    H, W = GRIDS[key]
    g = O.positional_grid(W, H)[None] * 1.3 - 0.2
    return A.Grid.from_image_grid(g[0].to(dev)), O.pixelize(g), g


def _zero_gradient(k):
    """The entries with an exactly zero gradient (the module docstring): compared with the float64 oracle."""
    return k.endswith("scale.weight_v")


def _zero_entries_bound(ref32, ref64, floor):
    """floor + 4 e32 + 1e-6 max|float64| over the zero-gradient entries of a case, and e32 itself."""
    keys = [k for k in ref64 if _zero_gradient(k)]
    e32 = max(float((ref32[k].double() - ref64[k]).abs().max()) for k in keys)
    return floor + 4.0 * e32 + 1e-6 * max(float(ref64[k].abs().max()) for k in keys), e32


def _check_zero_entries(got, ref32, ref64, what, floor):
    bound, e32 = _zero_entries_bound(ref32, ref64, floor)
    e_hip = max(float((got[k].double().reshape(ref64[k].shape) - ref64[k]).abs().max()) for k in ref64 if _zero_gradient(k))
    print(f"[zero-gradient entries] {what}: e_hip {e_hip:.3e} e32 {e32:.3e} bar {bound:.3e}")
    assert e_hip <= bound, (what, e_hip, e32, bound)


def _cancellation_floor(sd, ref64):
    """What float32 may leave of an exactly zero d/d weight_v: the chain rule forms it as the difference of two equal terms of size
    T = |g / v| |dL/dw| (|dL/dw| = |dL/dg| for a scalar v), each rounded to float32 - a few ulps of T on top of the borrowed 1e-7."""
    t = max(float((sd[k[:-1] + "g"].double() / sd[k].double()).abs().max() * ref64[k[:-1] + "g"].abs().max()) for k in ref64 if _zero_gradient(k))
    return 1e-7 + 4.0 * 2.0 ** -23 * t


def _check_grads(got, ref, ref64, what="", sd=None):
    """Flow half: the gradient bar of tests/test_gpu_flow.py; ICNN half: the bar of the layer-by-layer shapes (tests/test_gpu_icnn.py);
    the zero-gradient entries against the float64 oracle `ref64` (`sd`: the state the gradients were taken at)."""
    worst = {}
    for k, r in ref.items():
        if _zero_gradient(k):
            continue
        r, g = r.numpy(), got[k].numpy().reshape(r.shape)
        scale = float(np.abs(r).max())
        icnn = k.startswith("convex_net.")
        rtol, atol = (5e-4, 5e-6 * scale + 1e-10) if icnn else (1e-3, 2e-5 * scale + 1e-7)
        half = "icnn" if icnn else "flow"
        worst[half] = max(worst.get(half, 0.0), float((np.abs(g - r) / (atol + rtol * np.abs(r))).max()))
    print(f"[grad error / bar] {what}: " + ", ".join(f"{h} {v:.3f}" for h, v in sorted(worst.items())))
    _check_zero_entries(got, ref, ref64, what, _cancellation_floor(sd, ref64))
    for k, r in ref.items():
        if _zero_gradient(k):
            continue
        r, g = r.numpy(), got[k].numpy().reshape(r.shape)
        scale = float(np.abs(r).max())
        if k.startswith("convex_net."):
            np.testing.assert_allclose(g, r, rtol=5e-4, atol=5e-6 * scale + 1e-10, err_msg=f"{what} {k}")
        else:
            np.testing.assert_allclose(g, r, rtol=1e-3, atol=2e-5 * scale + 1e-7, err_msg=f"{what} {k}")


def _oracle_grads(sd, rows, loss_of, dtype):
    """Gradients of loss_of(logits (N,)) w.r.t. every entry of the state, the oracle's forward in `dtype` -> (loss, logits, grads)."""
    sdo = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    yo = O.convex_diffeo_forward(sdo, rows.to(dtype), K).reshape(-1)
    lo = loss_of(yo, dtype)
    lo.backward()
    return lo.detach(), yo.detach(), {k: v.grad for k, v in sdo.items()}


# ---- 1. forward and loss_grad through the C ABI -----------------------------------------------------------------------------------
def test_c_abi_answers_for_a_layer_by_layer_icnn(dev):
    """The calls that answered INR_EUNSUPPORTED for these shapes: the workspace query now sizes them, inrfit_cdn_forward runs (raw
    ctypes, no wrapper in between); inrfit_cdn_joint_step and inrfit_cdn_fit_minibatch keep refusing them."""
    import ctypes as C
    from awesome_amd import _lib as L
    from awesome_amd import icnn as KK
    lib = L.load()
    ispec, fspec, sd = _case(144, 1)
    grid, rows, _ = _grid("23x19", dev)
    md, fd, gd = ispec.desc(), fspec.desc(), grid.desc()
    need = lib.inrfit_cdn_workspace_bytes(C.byref(md), C.byref(fd), C.byref(gd), 1)
    assert need > lib.inrfit_cdn_workspace_bytes(None, C.byref(fd), C.byref(gd), 1) > 0
    ip, fp = _split(ispec, fspec, sd, dev)
    ws = torch.empty(need // 4 + 1, device=dev)
    out = torch.empty(1, grid.n_points, device=dev)
    args = (C.byref(md), C.byref(fd), ip.data_ptr(), fp.data_ptr(), C.byref(gd), 1, out.data_ptr(), ws.data_ptr())
    assert lib.inrfit_cdn_forward(*args, need - 1, KK._stream_ptr(dev)) == -3            # INR_EWORKSPACE: the carve is checked
    assert lib.inrfit_cdn_forward(*args, need, KK._stream_ptr(dev)) == 0
    yo = O.convex_diffeo_forward(sd, rows, K)
    np.testing.assert_allclose(out[0].cpu().numpy(), yo.reshape(-1).numpy(), rtol=1e-4, atol=3e-5)
    assert lib.inrfit_minibatch_workspace_bytes(C.byref(md), C.byref(fd), 64, 1) == EUNSUPPORTED
    assert lib.inrfit_cdn_wide_minibatch_workspace_bytes(C.byref(md), C.byref(fd), 64, 1) > 0
    fused = KK.IcnnSpec(130, 2, 1).desc()
    assert lib.inrfit_cdn_wide_minibatch_workspace_bytes(C.byref(fused), C.byref(fd), 64, 1) == EUNSUPPORTED


@pytest.mark.parametrize("backbone", ["normal_block", "default"])
@pytest.mark.parametrize("key", list(GRIDS))
@pytest.mark.parametrize("h,layers", SHAPES)
def test_forward_and_loss_grad(dev, h, layers, key, backbone):
    """Deformed coordinates, logits, and for SE, BCE, BCE with class weights and an external dL/dlogits: loss, every flow gradient and
    every ICNN gradient."""
    from awesome_amd import flow as FL
    ispec, fspec, sd = _case(h, layers, backbone)
    assert not ispec.fused() and ispec.supported()
    grid, rows, _ = _grid(key, dev)
    N = rows.shape[0]
    ip, fp = _split(ispec, fspec, sd, dev)
    xd_ref = O.flow1d_forward(sd, torch.nn.functional.linear(rows, sd["linear.weight"], sd["linear.bias"]), K, prefix="diffeo_net.")
    np.testing.assert_allclose(FL.flow_forward(fspec, fp, grid)[0].cpu().numpy(), xd_ref.t().numpy(), rtol=2e-5, atol=2e-6)
    yo = O.convex_diffeo_forward(sd, rows, K)
    y = FL.cdn_forward(ispec, fspec, ip, fp, grid)
    np.testing.assert_allclose(y[0].cpu().numpy(), yo.reshape(-1).numpy(), rtol=1e-4, atol=3e-5)
    g = torch.Generator().manual_seed(9)
    un, dl = torch.rand(N, generator=g), torch.randn(N, generator=g)
    for kind, mode in (("se", "none"), ("bce", "none"), ("bce", "sssdms"), ("external", "none")):
        if kind == "external":
            loss_of, tgt = (lambda y, dt: (y * dl.to(dt)).sum()), dl
        else:
            loss_of = lambda y, dt: O.weighted_loss(torch.sigmoid(y).reshape(1, 1, -1, 1), un.to(dt).reshape(1, 1, -1, 1), kind, mode)  # noqa: E731
            tgt = un
        lo, _, ref = _oracle_grads(sd, rows, loss_of, torch.float32)
        _, _, ref64 = _oracle_grads(sd, rows, loss_of, torch.float64)
        loss, gi, gf = FL.cdn_loss_grad(ispec, fspec, ip, fp, grid, tgt.reshape(1, -1).to(dev), loss=kind, weight_mode=mode)
        if kind != "external":
            assert float(loss[0]) == pytest.approx(float(lo), rel=2e-5)
        got = FL.merge_cdn_state_dict(ispec, fspec, gi[0].cpu(), gf[0].cpu())
        _check_grads(got, ref, ref64, f"{h}x{layers} {key} {backbone} {kind}/{mode}", sd)


# ---- 2-5. the fit -------------------------------------------------------------------------------------------------------------------
def _fit_case(dev, h=144, layers=1, key="23x19", seed=2):
    ispec, fspec, sd = _case(h, layers, seed=seed)
    H, W = GRIDS[key]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    un = (((yy - 0.45 * H) ** 2 + (xx - 0.5 * W) ** 2) > 0.07 * H * W).float()
    grid, rows, image_grid = _grid(key, dev)
    ip, fp = _split(ispec, fspec, sd, dev)
    return ispec, fspec, sd, image_grid, un, ip, fp, grid


def _oracle_fit(sd, image_grid, un, steps, dtype=torch.float32, **kw):
    return O.fit_convex_diffeo({k: v.to(dtype) for k, v in sd.items()}, image_grid.to(dtype), un[None, None].to(dtype), steps, K, **kw)


def _assert_trajectory(ispec, fspec, res, pf, pf64, losses, logits=None, what=""):
    """The bars of tests/test_gpu_flow.py::test_hip_cdn_fit_trajectory; the zero-gradient entries against the float64 loop `pf64`."""
    from awesome_amd import flow as FL
    np.testing.assert_allclose(res.loss_hist[0].cpu().numpy(), np.asarray(losses, np.float32), rtol=5e-4)
    got = FL.merge_cdn_state_dict(ispec, fspec, res.icnn_params[0].cpu(), res.flow_params[0].cpu())
    _check_zero_entries(got, pf, pf64, what, 3e-4)
    for k in pf:
        if not _zero_gradient(k):
            np.testing.assert_allclose(got[k].numpy(), pf[k].numpy(), rtol=5e-3, atol=3e-4, err_msg=k)
    if logits is not None:
        np.testing.assert_allclose(res.logits[0].cpu().numpy(), logits.reshape(-1).numpy(), rtol=5e-3, atol=2e-3)
    return got


@pytest.mark.parametrize("h,layers", [(144, 1), (64, 3)])
def test_fit_trajectory(dev, h, layers):
    """12 Adam steps with weight decay on weight_g against the oracle's loop: loss history, both parameter halves, the final logits."""
    from awesome_amd import flow as FL
    ispec, fspec, sd, image_grid, un, ip, fp, grid = _fit_case(dev, h, layers)
    kw = dict(lr=3e-3, loss_kind="bce", weight_decay_on_weight_g=5e-3)
    pf, losses, logits = _oracle_fit(sd, image_grid, un, 12, **kw)
    pf64, _, _ = _oracle_fit(sd, image_grid, un, 12, torch.float64, **kw)
    res = FL.cdn_fit(ispec, fspec, ip, fp, grid, un.reshape(1, -1).to(dev), 12, lr=3e-3, loss="bce", weight_decay_on_weight_g=5e-3,
                     plateau=None)
    assert int(res.status[0]) == 0
    got = _assert_trajectory(ispec, fspec, res, pf, pf64, losses, logits, what=f"fit {h}x{layers}")
    assert not np.allclose(got["diffeo_net.s.0.in_linear.linear.weight_g"].numpy(), sd["diffeo_net.s.0.in_linear.linear.weight_g"].numpy())
    for k, v in got.items():   # enforce_convexity after every step
        if k.startswith("convex_net.") and k.endswith("ln.weight") and not k.startswith("convex_net.input"):
            assert float(v.min()) >= 0.0, k


def test_fit_in_two_calls_equals_one_call(dev):
    """7 steps, then 5 with step0 = 7 and the returned optimizer states: bit for bit the 12-step fit; a second identical call too."""
    from awesome_amd import flow as FL
    ispec, fspec, sd, _, un, ip, fp, grid = _fit_case(dev)
    t = un.reshape(1, -1).to(dev)
    kw = dict(lr=3e-3, loss="bce", weight_decay_on_weight_g=5e-3, plateau=dict(patience=2, factor=0.5))
    one = FL.cdn_fit(ispec, fspec, ip.clone(), fp.clone(), grid, t, 12, **kw)
    two = FL.cdn_fit(ispec, fspec, ip.clone(), fp.clone(), grid, t, 12, **kw)
    a = FL.cdn_fit(ispec, fspec, ip.clone(), fp.clone(), grid, t, 7, **kw)
    b = FL.cdn_fit(ispec, fspec, a.icnn_params, a.flow_params, grid, t, 5, icnn_opt_state=a.icnn_opt_state,
                   flow_opt_state=a.flow_opt_state, step0=7, **kw)
    for r in (two, b):
        assert torch.equal(r.icnn_params, one.icnn_params) and torch.equal(r.flow_params, one.flow_params)
        assert torch.equal(r.logits, one.logits)
    assert torch.equal(two.loss_hist, one.loss_hist) and torch.equal(torch.cat([a.loss_hist, b.loss_hist], 1), one.loss_hist)
    assert not torch.equal(one.flow_params, fp) and not torch.equal(one.icnn_params, ip)


def test_plateau_reduces_the_learning_rate_of_both_halves(dev):
    """ReduceLROnPlateau(patience 2, factor 0.5) on a loss that stalls (a relative threshold no step reaches): the learning rate halves
    after steps 4, 7 and 10 for BOTH halves - the flow's parameters follow the oracle's loop with the reduced rates, far from the loop
    without them."""
    from awesome_amd import flow as FL
    ispec, fspec, sd, image_grid, un, ip, fp, grid = _fit_case(dev)
    pl = dict(patience=2, factor=0.5, threshold=0.9)
    kw = dict(lr=4e-3, loss_kind="bce", weight_decay_on_weight_g=5e-3)
    pf, losses, _ = _oracle_fit(sd, image_grid, un, 12, plateau=pl, **kw)
    pf64, _, _ = _oracle_fit(sd, image_grid, un, 12, torch.float64, plateau=pl, **kw)
    pn, losses_n, _ = _oracle_fit(sd, image_grid, un, 12, **kw)
    res = FL.cdn_fit(ispec, fspec, ip, fp, grid, un.reshape(1, -1).to(dev), 12, lr=4e-3, loss="bce", weight_decay_on_weight_g=5e-3,
                     plateau=pl)
    got = _assert_trajectory(ispec, fspec, res, pf, pf64, losses, what="fit 144x1, plateau")
    hdr = res.icnn_opt_state[0, 2 * ispec.n_params:]
    assert float(hdr[2]) == pytest.approx(4e-3 * 0.5 ** 3, rel=1e-6)
    # the flow half took the reduced rates: its distance from the constant-rate loop is far above the bar on some flow parameter
    k = "diffeo_net.s.0.in_linear.linear.bias"
    far = float((pf[k] - pn[k]).abs().max())
    assert far > 20 * 3e-4, far
    assert float((got[k] - pf[k]).abs().max()) < 0.1 * far


def test_two_images_nan_target_freezes_both_halves(dev):
    """NaN in image 1's targets: its ICNN and flow rows stay at the parameters before the step, its status is set; image 0's rows are
    bit-equal to a single-image call although both images pass through the one layer-by-layer workspace (0 x NaN in gemm.h's buffer
    mode would leak there)."""
    from awesome_amd import flow as FL
    ispec, fspec, sd, _, un, ip, fp, grid = _fit_case(dev, h=131, layers=2)
    ip2, fp2 = ip.repeat(2, 1).contiguous(), fp.repeat(2, 1).contiguous()
    fp2[1, :2] *= 1.1   # (another deformation for image 1)
    for order in ((0, 1), (1, 0)):   # the bad image behind the good one in the workspace, and in front of it
        good, badi = order
        t = un.reshape(1, -1).repeat(2, 1).to(dev)
        t[badi, 17] = float("nan")
        kw = dict(lr=3e-3, loss="bce", weight_decay_on_weight_g=5e-3, plateau=None)
        r1 = FL.cdn_fit(ispec, fspec, ip2.clone(), fp2.clone(), grid, t, 6, **kw)
        r2 = FL.cdn_fit(ispec, fspec, ip2.clone(), fp2.clone(), grid, t, 6, **kw)
        single = FL.cdn_fit(ispec, fspec, ip2[good:good + 1].clone(), fp2[good:good + 1].clone(), grid, t[good:good + 1].contiguous(), 6, **kw)
        assert int(r1.status[good]) == 0 and int(r1.status[badi]) != 0
        assert torch.equal(r1.icnn_params[badi], ip2[badi]) and torch.equal(r1.flow_params[badi], fp2[badi])
        assert torch.isfinite(r1.icnn_params).all() and torch.isfinite(r1.flow_params).all()
        assert torch.equal(r1.icnn_params[good], single.icnn_params[0]) and torch.equal(r1.flow_params[good], single.flow_params[0])
        assert torch.equal(r1.loss_hist[good], single.loss_hist[0]) and torch.equal(r1.logits[good], single.logits[0])
        assert not torch.equal(r1.icnn_params[good], ip2[good]) and not torch.equal(r1.flow_params[good], fp2[good])
        for a, b in ((r1.icnn_params, r2.icnn_params), (r1.flow_params, r2.flow_params), (r1.logits[good], r2.logits[good])):
            assert torch.equal(a, b)


# ---- 6. the module -----------------------------------------------------------------------------------------------------------------
def _module(dev, h=144, layers=1, seed=3):
    from awesome_amd.model import ConvexDiffeomorphismNet
    ispec, fspec, sd = _case(h, layers, seed=seed)
    m = ConvexDiffeomorphismNet(n_hidden=h, n_hidden_layers=layers, nf_layers=K, nf_hidden=WIDTH, diffeo_args=dict(backbone="normal_block"))
    m.load_state_dict(sd)
    return m.to(dev), sd


@pytest.mark.parametrize("layout", ["image", "rows"])
def test_module_forward_backward(dev, layout):
    """ConvexDiffeomorphismNet(n_hidden=144): forward + backward of a scalar loss on (1, 2, H, W) and on (N, 2), one composite call."""
    m, sd = _module(dev)
    assert not m._generic() and not m._specs()[0].fused()
    H, W = GRIDS["23x19"]
    _, rows, image_grid = _grid("23x19", dev)
    un = torch.rand(H * W, generator=torch.Generator().manual_seed(1))
    out = m(image_grid.to(dev)) if layout == "image" else m(rows.to(dev))
    assert out.shape == ((1, 1, H, W) if layout == "image" else (H * W, 1))
    loss = ((torch.sigmoid(out.reshape(-1)) - un.to(dev)) ** 2).mean()
    loss.backward()
    loss_of = lambda y, dt: ((torch.sigmoid(y) - un.to(dt)) ** 2).mean()   # noqa: E731
    lo, yo, ref = _oracle_grads(sd, rows, loss_of, torch.float32)
    _, _, ref64 = _oracle_grads(sd, rows, loss_of, torch.float64)
    np.testing.assert_allclose(out.detach().reshape(-1).cpu().numpy(), yo.numpy(), rtol=1e-4, atol=3e-5)
    assert float(loss.detach()) == pytest.approx(float(lo), rel=2e-5)
    names = [k for k, _ in m.named_parameters()]
    _check_grads({k: p.grad.cpu() for k, p in m.named_parameters()}, {k: ref[k] for k in names}, {k: ref64[k] for k in names},
                 f"module {layout}", sd)


def test_module_fit_minibatch_equals_the_loop_of_single_steps(dev):
    """fit_minibatch for 5 epochs (one device call: inrfit_cdn_wide_fit_minibatch) against the per-epoch host loop - gather, explicit
    grid, inrfit_cdn_fit(steps = 1, step0 = k): the same bits in both halves and the loss history."""
    import awesome_amd as A
    from awesome_amd import flow as FL
    from awesome_amd import minibatch as MB
    m, sd = _module(dev, seed=4)
    ispec, fspec = m._specs()
    _, rows, _ = _grid("23x19", dev)
    H, W = GRIDS["23x19"]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    labels = (((yy - 0.45 * H) ** 2 + (xx - 0.5 * W) ** 2) < 0.07 * H * W).float().reshape(-1)
    number, epochs, cw = 50, 5, (2.0, 1.0)
    table = MB.class_balanced_batches(labels, epochs, number, torch.Generator().manual_seed(11))
    ip, fp = _split(ispec, fspec, sd, dev)
    opt, hist = [None, None], []
    co, tg = rows.t().contiguous().to(dev), labels.reshape(1, -1).to(dev)
    for k in range(epochs):
        idx = table[k].long().to(dev)
        r = FL.cdn_fit(ispec, fspec, ip, fp, A.Grid.explicit(co[:, idx].contiguous()), tg[:, idx].contiguous(), 1, lr=1e-2, loss="bce",
                       weight_mode="explicit", c_fg=cw[0] / number, c_bg=cw[1] / number, weight_decay_on_weight_g=0.0, clamp=False,
                       icnn_opt_state=opt[0], flow_opt_state=opt[1], step0=k, want_logits=False, plateau=None)
        opt = [r.icnn_opt_state, r.flow_opt_state]
        hist.append(r.loss_hist[:, 0].clone())
    res = m.fit_minibatch(rows.to(dev), labels.to(dev), epochs, lr=1e-2, class_weights=cw, batch_index=table)
    assert int(res.status[0]) == 0
    assert torch.equal(res.icnn_params, ip) and torch.equal(res.flow_params, fp) and torch.equal(res.loss_hist, torch.stack(hist, 1))
    assert not torch.equal(fp[0].cpu(), FL.split_cdn_state_dict(ispec, fspec, sd)[1])
    got = FL.split_cdn_state_dict(ispec, fspec, m.state_dict(), dev)
    assert torch.equal(got[0], ip[0]) and torch.equal(got[1], fp[0])          # the module's parameters were updated in place


_CDN_ARGS = dict(n_hidden=144, n_hidden_layers=1, nf_layers=K, nf_hidden=WIDTH, diffeo_args=dict(backbone="normal_block"))


class _Agent:
    def __init__(self, ds, dev):
        self.training_dataset, self.device, self.logger = ds, dev, None


def _pretrain(dev, **kw):
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.measures import SE, UnariesConversionLoss
    from awesome_amd.model import ConvexDiffeomorphismNet, ForwardModule, WrapperModule
    torch.manual_seed(1)
    ds = SyntheticPriorDataset(n_images=2, size=32, kind="blob", prior_model_type=ConvexDiffeomorphismNet, prior_model_args=_CDN_ARGS)
    wrapper = WrapperModule(ForwardModule(), ConvexDiffeomorphismNet(**_CDN_ARGS), use_segmentation_output_inversion=True).to(dev)
    state = wrapper.pretrain(train_set=ds, test_set=None, device=dev, agent=_Agent(ds, dev), use_progress_bar=False, lr=3e-3,
                             criterion=UnariesConversionLoss(SE("mean")), **kw)
    return state, wrapper.prior_module.pretrain_report


def test_wrapper_pretrain_on_the_device_engine(dev):
    """pretrain(device_fit_layer_by_layer=True) on two 32 x 32 blobs: both images in the batched device engine (inrfit_cdn_fit), the
    prior cache under the reference's key names, the IoU gate passed without a retry."""
    from awesome_amd.model import ConvexDiffeomorphismNet
    state, rep = _pretrain(dev, num_epochs=150, reuse_state=False, device_fit_layer_by_layer=True)
    assert sorted(state["cache"]) == ["0", "1"] and state["model_type"].endswith("ConvexDiffeomorphismNet")
    assert json.loads(state["model_args"])["n_hidden"] == 144
    names = list(ConvexDiffeomorphismNet(**_CDN_ARGS).state_dict().keys())
    for sd in state["cache"].values():
        assert list(sd.keys()) == names and sd["convex_net.skip.0.ln.weight"].shape == (144, 144)
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert all(r["engine"] == "device" and r["status"] == 0 and r["retries"] == 0 and r["iou"] >= 0.5 for r in rep), rep
    assert not torch.equal(state["cache"]["0"]["convex_net.input.weight"], state["cache"]["1"]["convex_net.input.weight"])
    # the warm-started chain (reuse_state: the centre-of-mass translate on the flat row's linear layer) runs on the same engine
    state, rep = _pretrain(dev, num_epochs=150, reuse_state=True, reuse_state_epochs=20, device_fit_layer_by_layer=True)
    assert sorted(state["cache"]) == ["0", "1"] and all(r["engine"] == "device" and r["status"] == 0 for r in rep), rep


def test_wrapper_pretrain_default_stays_on_the_generic_engine(dev):
    state, rep = _pretrain(dev, num_epochs=3, reuse_state=False, proper_prior_fit_threshold=0.0)
    assert sorted(state["cache"]) == ["0", "1"] and all(r["engine"] == "generic" for r in rep), rep


# ---- 7. the config -----------------------------------------------------------------------------------------------------------------
def test_run_py_cdn_wide256(tmp_path):
    """config/c2_blob256_cdn_wide256.yaml shrunk to 64 x 64 in a child process: the pretrain fit on the device engine, the joint epoch
    on the fused route (inrfit_cdn_wide_joint_step)."""
    override = {"dataset_args": {"size": 64}, "agent_args": {"pretrain_args": {"num_epochs": 20, "proper_prior_fit_retrys": 0}}}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--config-path",
                          os.path.join(ROOT, "config", "c2_blob256_cdn_wide256.yaml"), "--output-folder", str(tmp_path),
                          "--override", json.dumps(override)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    summary = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert summary["images"] == 1 and summary["priors_saved"] == 1
    assert summary["joint_epochs"] == 1 and summary["joint_steps_fused"] == 1
    sd = torch.load(os.path.join(summary["output"], "prior_cache_epoch_0.pth"), weights_only=False)["cache"]["0"]
    assert sd["convex_net.input.weight"].shape[0] == 256
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
