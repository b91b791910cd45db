"""The rotation-symmetric prior trained in one device call (inrfit_sym_*, csrc/sym.h) on the GPU: gradients and forward against float64
autograd and the notebook class's own outputs, every fit against the notebook's loop in float64, bit-equality with the per-step host
loop, continuation across the mirror switch, the index clamp, the non-finite freeze, a point at the centre, and the module surface.
The cases, the host loop and the float64 / float32 restatements are tests/sym_cases.py's."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sym_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _state(r):
    return (r.params, r.pose, r.opt_state, r.pose_opt_state)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. gradient parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [False, True], ids=["free", "mirror"])
@pytest.mark.parametrize("h,n", [(130, 1440), (130, 193), (150, 1440), (150, 193)])
def test_loss_and_gradients_match_float64_autograd(dev, h, n, sym):
    """sym_loss_grad against float64 autograd through the oracle's forward: the loss, every network gradient and the three pose
    gradients, each within 4 e32 + 1e-6 max|f64| (e32: float32 autograd's own distance).  This pins the pose gradient's scale, which
    Adam's first steps alone would not."""
    import awesome_amd as A
    import awesome_amd.symmetric as SY
    g = SC.gradient_reference(h, n, sym)
    m = g["module"]
    flat, pose = m.flat_parameters()[None].contiguous().to(dev), m._pose()[None].contiguous().to(dev)
    lo, gn, gp = SY.sym_loss_grad(m.spec, flat, pose, A.Grid.explicit(g["coords"].to(dev)), g["targets"][None].to(dev), sym)
    keep = SC.learned(m.spec)   # (the skip weights are constants: no reference has their gradient)
    d = dict(loss=float((lo[0].double().cpu() - g["loss"]).abs()), net=float((gn[0].double().cpu() - g["net"])[keep].abs().max()),
             pose=float((gp[0].double().cpu() - g["pose"]).abs().max()))
    b = {k: SC.parity_bound(g["e_" + k], g[k]) for k in d}
    print(f"sym gradient parity h={h} n={n} sym={sym}: " + " | ".join(f"{k} {d[k]:.3e} (bound {b[k]:.3e})" for k in d))
    assert all(d[k] <= b[k] for k in d), (d, b)


# ---- 2. forward parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,sp", [("free", False), ("sym", True)])
def test_forward_matches_the_notebook_class(dev, golden_dir, tag, sp):
    import awesome_amd as A
    import awesome_amd.symmetric as SY
    from awesome_amd.model import RotationSymmetricNet
    z = np.load(os.path.join(golden_dir, "teaser_rotation_symmetric.npz"))
    m = RotationSymmetricNet(130)
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")})
    flat, pose = m.flat_parameters()[None].contiguous().to(dev), m._pose()[None].contiguous().to(dev)
    x = torch.from_numpy(z["x"]).to(dev)
    y = SY.sym_forward(m.spec, flat, pose, A.Grid.explicit(x.t()), sp)
    assert tuple(y.shape) == (1, x.shape[0])
    np.testing.assert_allclose(y[0].cpu().numpy()[:, None], z[tag + ".y"], rtol=1e-5, atol=1e-5)


def test_separable_grid_equals_the_explicit_one(dev):
    """The pose kernels read a separable grid (xs [W], ys [H], point = row W + column) or explicit planes: the same numbers, so the
    same bits, forward and gradients."""
    import awesome_amd as A
    import awesome_amd.symmetric as SY
    m = SC.case("sym32").modules[0]
    flat, pose = m.flat_parameters()[None].contiguous().to(dev), m._pose()[None].contiguous().to(dev)
    xs, ys = (torch.arange(23) / 23.0 - 0.5).to(dev), (torch.arange(19) / 19.0 - 0.4).to(dev)
    sep = A.Grid.separable(xs, ys)
    exp = A.Grid.explicit(torch.stack([xs.repeat(19), ys.repeat_interleave(23)]))
    tg = SC.likelihood(exp.coords.cpu())[None].to(dev)
    for sp in (False, True):
        assert torch.equal(SY.sym_forward(m.spec, flat, pose, sep, sp), SY.sym_forward(m.spec, flat, pose, exp, sp))
        a, b = SY.sym_loss_grad(m.spec, flat, pose, sep, tg, sp), SY.sym_loss_grad(m.spec, flat, pose, exp, tg, sp)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and SC.finite(*a)


# ---- 3. fit parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.ALL_CASES)
def test_fit_within_the_float32_restatements_error_of_float64(dev, name):
    """The one call against the notebook's loop in float64: pose, network and loss history each within their own 4 e32 + 1e-6 max|f64|.

    Measured (profiles/symmetric_parity.md): see the table there."""
    r64 = SC.references(name)
    r = SC.device_call(SC.case(name), dev)
    assert int(r.status.abs().max()) == 0
    got = dict(pose=r.pose, net=r.params, hist=r.loss_hist)
    d = {k: float((got[k].double().cpu() - r64[k]).abs().max()) for k in got}
    b = {k: SC.parity_bound(r64["e_" + k], r64[k]) for k in got}
    print(f"sym parity {name}: " + " | ".join(f"{k} {d[k]:.3e} (e32 {r64['e_' + k]:.3e}, bound {b[k]:.3e}, ratio {d[k] / b[k]:.3f})"
                                              for k in ("pose", "net", "hist")))
    assert all(d[k] <= b[k] for k in d), (d, b)


# ---- 4. bit equality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.MINIBATCH_CASES)
def test_equals_the_per_step_host_loop_bit_for_bit(dev, name):
    c = SC.case(name)
    r = SC.device_call(c, dev)
    prm, pose, opt, popt, hist = SC.host_loop(c, dev)
    assert int(r.status.abs().max()) == 0 and SC.finite(r.loss_hist)
    assert torch.equal(r.params, prm), "parameters"
    assert torch.equal(r.pose, pose), "pose"
    assert torch.equal(r.opt_state, opt) and torch.equal(r.pose_opt_state, popt), "optimizer states"
    assert torch.equal(r.loss_hist, hist), "loss history"
    start = SC.initial(c, dev)
    assert not torch.equal(r.params, start[0]) and bool((r.pose != start[1]).all())      # (both did train)
    again = SC.device_call(c, dev)
    assert _same(_state(r), _state(again)) and torch.equal(r.loss_hist, again.loss_hist), "two identical calls"


@pytest.mark.parametrize("name", ["sym130x2", "sym150", "sym130_full"])
def test_continuation_across_the_switch_equals_one_call(dev, name):
    c = SC.case(name)
    whole = SC.device_call(c, dev, rows=(0, 6))
    first = SC.device_call(c, dev, rows=(0, 2))
    second = SC.device_call(c, dev, rows=(2, 6), state=_state(first))
    assert _same(_state(whole), _state(second))
    assert torch.equal(whole.loss_hist, torch.cat([first.loss_hist, second.loss_hist], 1))


def test_the_switch_changes_the_run(dev):
    """symmetry_from_step: negative = never, 0 = always; both differ from the case's switch at step 3 from the step they part on."""
    import dataclasses
    c = SC.case("sym32")
    at3 = SC.device_call(c, dev)
    never = SC.device_call(dataclasses.replace(c, kw={**c.kw, "symmetry_from_step": -1}), dev)
    always = SC.device_call(dataclasses.replace(c, kw={**c.kw, "symmetry_from_step": 0}), dev)
    assert torch.equal(at3.loss_hist[:, :3], never.loss_hist[:, :3]) and not torch.equal(at3.loss_hist[:, 3], never.loss_hist[:, 3])
    assert not torch.equal(at3.loss_hist[:, 0], always.loss_hist[:, 0])


# ---- 5. the clamp ---------------------------------------------------------------------------------------------------------------------
def test_indices_are_clamped_into_the_pool(dev):
    """Entries -1 and n_pool behave as 0 and n_pool - 1.  The pool tensors are interior slices of larger allocations, so a missing
    clamp reads a wrong number (the neighbouring plane or the guard values), not unmapped memory."""
    c = SC.case("sym32")
    n_pool = c.pool_coords.shape[1]
    pad_c = torch.full((2 * n_pool + 128,), 7.0, device=dev)
    pad_t = torch.full((n_pool + 128,), 0.25, device=dev)
    co_in = pad_c[64:64 + 2 * n_pool].view(2, n_pool)
    tg_in = pad_t[64:64 + n_pool].view(1, n_pool)
    co_in.copy_(c.pool_coords.to(dev))
    tg_in.copy_(c.pool_targets.to(dev))
    assert co_in.is_contiguous() and co_in.data_ptr() == pad_c.data_ptr() + 256
    bad = c.index[:4].clone()
    bad[0, 3], bad[1, 0], bad[2, 150], bad[3, 191] = -1, n_pool, -1, n_pool
    good = bad.clone()
    good[0, 3], good[1, 0], good[2, 150], good[3, 191] = 0, n_pool - 1, 0, n_pool - 1
    out = [SC.device_call(c, dev, rows=(0, 4), index=table, coords=co_in, targets=tg_in) for table in (bad, good)]
    assert _same(_state(out[0]), _state(out[1])) and torch.equal(out[0].loss_hist, out[1].loss_hist)
    assert SC.finite(out[0].loss_hist)


# ---- 6. non-finite --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sym130x2", "sym150"])
def test_non_finite_loss_freezes_network_and_pose(dev, name):
    c = SC.case(name)
    used = [set(c.index[k].tolist()) for k in range(6)]
    only3 = sorted(used[3] - used[0] - used[1] - used[2] - used[4] - used[5])
    assert only3, "the case's table has a pixel that only step 3 draws"
    tg = c.pool_targets.clone()
    tg[0, only3[0]] = float("nan")
    r6 = SC.device_call(c, dev, targets=tg)
    r3 = SC.device_call(c, dev, rows=(0, 3), targets=tg)
    assert int(r6.status[0]) == 1 and int(r3.status.abs().max()) == 0
    assert not bool(torch.isfinite(r6.loss_hist[0, 3])) and SC.finite(r6.loss_hist[0, :3])
    assert torch.equal(r6.loss_hist[0, :3], r3.loss_hist[0])
    P = SC.spec(c).n_params
    assert torch.equal(r6.params[0], r3.params[0]) and torch.equal(r6.pose[0], r3.pose[0])
    assert torch.equal(r6.opt_state[0, :2 * P], r3.opt_state[0, :2 * P]) and torch.equal(r6.pose_opt_state[0], r3.pose_opt_state[0])
    if c.n_images > 1:   # the other image trains on: its own six steps
        ref = SC.device_call(c, dev)
        assert int(r6.status[1]) == 0 and torch.equal(r6.params[1], ref.params[1]) and torch.equal(r6.pose[1], ref.pose[1])


# ---- 7. the centre point --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sym32", "sym150"])
def test_a_point_at_the_centre_is_left_out_of_the_pose_gradient(dev, name):
    """A pool that holds -offset exactly (r == 0), drawn in every step: torch's gradient is NaN there, the kernel's stated guard gives
    it no share.  The first step equals the step without that point's pose share: finite everywhere."""
    c = SC.case(name)
    co = c.pool_coords.clone()
    prm, pose = SC.initial(c, dev)
    co[:, 0] = -pose[0, :2].cpu()                        # the float32 offset negated: x + offset == 0 exactly
    index = c.index.clone()
    index[:, 0] = 0
    r = SC.device_call(c, dev, state=(prm, pose, None, None), index=index, coords=co)
    assert int(r.status.abs().max()) == 0
    assert SC.finite(r.params, r.pose, r.pose_opt_state, r.loss_hist)
    assert bool((r.pose != SC.initial(c, dev)[1]).all())


# ---- 8. the module --------------------------------------------------------------------------------------------------------------------
def test_module_fit_minibatch(dev):
    import inspect
    from awesome_amd.model import RotationSymmetricNet
    c = SC.case("sym150")
    torch.manual_seed(SC.MODULE_SEED)
    net = RotationSymmetricNet(150)
    with torch.no_grad():
        net.offset.copy_(torch.tensor([SC.OFFSET]))
        net.orientation.fill_(SC.ORIENTATION)
    net = net.to(dev)
    assert torch.equal(net.flat_parameters().cpu(), c.modules[0].flat_parameters())       # the case's own seed
    assert inspect.signature(net.fit_minibatch).parameters["symmetry_from_epoch"].default == 502
    pixels, labels = c.pool_coords.t().contiguous(), c.pool_targets[0]
    before = {k: v.data_ptr() for k, v in net.state_dict().items()}
    assert set(before) == {"offset", "orientation", "W0.weight", "W0.bias", "W1.weight", "W1.bias", "W2.weight", "W2.bias"}
    state = {}
    res = net.fit_minibatch(pixels, labels, 2, symmetry_from_epoch=SC.SWITCH, batch_index=c.index[:2], state=state)
    res2 = net.fit_minibatch(pixels, labels, 4, symmetry_from_epoch=SC.SWITCH, batch_index=c.index[2:], state=state)
    assert state["epoch"] == 6 and tuple(res.loss_hist.shape) == (1, 2) and tuple(res2.loss_hist.shape) == (1, 4)
    assert set(state) == {"opt_state", "pose_opt_state", "epoch"}
    ref = SC.device_call(c, dev)
    assert torch.equal(net.flat_parameters(), ref.params[0]) and torch.equal(net._pose(), ref.pose[0])   # in place, to the flat result
    assert torch.equal(torch.cat([res.loss_hist, res2.loss_hist], 1), ref.loss_hist)
    assert {k: v.data_ptr() for k, v in net.state_dict().items()} == before
    # forward under no_grad (inrfit_sym_forward) against the autograd forward (pose in torch) on the same input
    x = pixels.to(dev)
    for sp in (False, True):
        with torch.no_grad():
            y0 = net(x, sp)
        y1 = net(x, sp)
        assert tuple(y0.shape) == (x.shape[0], 1) and y1.requires_grad and not y0.requires_grad
        np.testing.assert_allclose(y0.cpu().numpy(), y1.detach().cpu().numpy(), rtol=1e-5, atol=1e-5)
    # the draw of its own: `number` per class and epoch, seeded; the default switch lies beyond these epochs
    net.fit_minibatch(pixels, labels, 2, number=96, generator=torch.Generator().manual_seed(5))
    assert SC.finite(net.flat_parameters(), net._pose())
