"""GPU parity of the L = 1 step kernel after its layer-0 gradient moved from the matrix pipe to per-lane VALU chains (a transpose
between lane groups and tiles, then one FMA chain per parameter) and the leftover outputs of the backward product to one k-step
(icnn_step.h).  The per-lane accumulators live ACROSS the chunks of a workgroup, so next to the ragged 19 x 23 grid of the
every-parameter test there is a 131 x 127 one: 16 637 points = 260 chunks on the library's 256 slabs, i.e. four workgroups
accumulate over two chunks and the others over one.  Widths with (130) and without (64, 32) leftover units, both input counts,
and two widths that run zero-padded on the 130 kernel (100; 129, whose one real leftover unit sits next to a padded one - the
padded path has no odd leftover count of its own).  Checker: the CPU oracle, never the HIP path itself."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import inr_oracle as O  # noqa: E402  (checker only)

SHAPES = [(130, 2), (130, 3), (64, 2), (32, 3), (100, 2), (129, 2)]
GRIDS = [(19, 23), (131, 127)]          # (height, width)


@pytest.fixture(scope="module")
def amd():
    import awesome_amd as A
    assert torch.cuda.is_available()
    return A


_CASES = {}


def _case(A, h, C, hw):
    """One problem per (shape, grid), built once and left unchanged: parameters, grid, unaries, and the oracle's loss / gradients."""
    key = (h, C, hw)
    if key not in _CASES:
        H_, W_ = hw
        torch.manual_seed(1000 * h + 10 * C + H_)
        spec = A.IcnnSpec(n_hidden=h, in_features=C, n_layers=1)
        assert spec.supported()
        p = {k: (torch.rand(shp) - 0.45) * 0.3 for k, shp in spec.keys_shapes()}
        grid_t = O.positional_grid(W_, H_) if C == 2 else O.positional_grid(W_, H_, 0.4, 1.0)
        un = torch.from_numpy(np.random.RandomState(h + C + H_).rand(1, 1, H_, W_).astype(np.float32))
        yy, xx = torch.meshgrid(torch.arange(H_), torch.arange(W_), indexing="ij")
        disc = (((yy - 0.45 * H_) ** 2 + (xx - 0.4 * W_) ** 2) > (0.3 * min(H_, W_)) ** 2).float()[None, None]
        lo, go = O.loss_and_grads(p, grid_t[None], un, "se")
        _CASES[key] = dict(spec=spec, p=p, grid_t=grid_t, un=un, disc=disc, loss=float(lo), grads=go)
    return _CASES[key]


def _dev_inputs(A, c):
    dev = torch.device("cuda:0")
    flat = A.pack_state_dict(c["spec"], c["p"], dev)[None].contiguous()
    return dev, flat, A.Grid.from_image_grid(c["grid_t"].to(dev))


def test_second_grid_gives_some_workgroups_two_chunks(amd):
    n = 131 * 127
    slabs = amd._lib.load().inrfit_slabs_per_image(n, 1)
    chunks = (n + 63) // 64
    assert slabs == 256 and chunks == 260 and slabs < chunks < 2 * slabs


@pytest.mark.parametrize("hw", GRIDS)
@pytest.mark.parametrize("h,C", SHAPES)
def test_loss_and_every_parameter_gradient(amd, h, C, hw):
    """`loss_grad` against the oracle, every parameter, at the bar of test_every_compiled_shape_every_parameter_gradient."""
    A = amd
    c = _case(A, h, C, hw)
    dev, flat, grid = _dev_inputs(A, c)
    loss, g = A.loss_grad(c["spec"], flat, grid, c["un"].reshape(1, -1).to(dev), loss="se")
    print(f"h {h} C {C} grid {hw}: loss rel err {abs(float(loss[0]) - c['loss']) / abs(c['loss']):.2e}")
    got = A.unpack_params(c["spec"], g[0].cpu())
    assert set(got) == set(c["grads"])
    for k, ref in c["grads"].items():
        ref = ref.numpy()
        err = float(np.abs(got[k].numpy() - ref).max()) / (float(np.abs(ref).max()) + 1e-30)
        print(f"   {k}: max |err| / max |ref| {err:.2e}")
    assert float(loss[0]) == pytest.approx(c["loss"], rel=2e-5)
    for k, ref in c["grads"].items():
        ref = ref.numpy()
        np.testing.assert_allclose(got[k].numpy(), ref, rtol=2e-4, atol=2e-4 * float(np.abs(ref).max()) + 1e-10, err_msg=k)


@pytest.mark.parametrize("hw", GRIDS)
@pytest.mark.parametrize("h,C", SHAPES)
def test_coordinate_gradient_kernels(amd, h, C, hw):
    """The dx instantiations: `backward(..., want_dcoords=True)` for an external dL/dlogits against autograd through the oracle's
    forward, at the bars of test_coordinate_gradient."""
    A = amd
    c = _case(A, h, C, hw)
    dev, flat, _ = _dev_inputs(A, c)
    coords = c["grid_t"].reshape(C, -1)
    N = coords.shape[1]
    dlog = torch.from_numpy(np.random.RandomState(7 + h).randn(N).astype(np.float32))
    xr = coords.t().clone().requires_grad_(True)
    pr = {k: v.clone().requires_grad_(True) for k, v in c["p"].items()}
    (O.icnn_forward(pr, xr)[:, 0] * dlog).sum().backward()
    grads, dco = A.icnn.backward(c["spec"], flat, A.Grid.explicit(coords.to(dev)), dlog[None].to(dev), want_dcoords=True)
    ref = xr.grad.t().numpy()
    np.testing.assert_allclose(dco[0].cpu().numpy(), ref, rtol=2e-4, atol=2e-6 * float(np.abs(ref).max()))
    g = A.unpack_params(c["spec"], grads[0].cpu())
    for k in pr:
        r = pr[k].grad.numpy()
        np.testing.assert_allclose(g[k].numpy(), r, rtol=2e-4, atol=2e-6 * float(np.abs(r).max()) + 1e-9, err_msg=k)


@pytest.mark.parametrize("hw", GRIDS)
@pytest.mark.parametrize("h,C", SHAPES)
def test_adam_clamp_trajectory_and_repeatability(amd, h, C, hw):
    """25 Adam + clamp steps against the oracle's fit at the bars of test_any_hidden_width_up_to_130_runs_zero_padded; a second,
    identical call gives the same bits (the sums over lane groups, waves and slabs have a fixed order)."""
    A = amd
    c = _case(A, h, C, hw)
    dev, flat, grid = _dev_inputs(A, c)
    un = c["disc"]
    pf, losses, _ = O.fit_icnn(c["p"], c["grid_t"][None], un, 25, lr=2e-3)
    res = A.fit(c["spec"], flat.clone(), grid, un.reshape(1, -1).to(dev), 25, lr=2e-3)
    again = A.fit(c["spec"], flat.clone(), grid, un.reshape(1, -1).to(dev), 25, lr=2e-3)
    assert torch.equal(res.params, again.params) and torch.equal(res.loss_hist, again.loss_hist)
    got_l = res.loss_hist[0].cpu().numpy()
    print(f"h {h} C {C} grid {hw}: loss curve max rel err {float(np.abs(got_l / np.asarray(losses, np.float32) - 1).max()):.2e}")
    np.testing.assert_allclose(got_l, np.asarray(losses, np.float32), rtol=2e-4)
    gotp = A.unpack_params(c["spec"], res.params[0].cpu())
    for k in pf:
        np.testing.assert_allclose(gotp[k].numpy(), pf[k].numpy(), rtol=5e-4, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("h,C", SHAPES)
def test_one_joint_step(amd, h, C):
    """One `inrfit_joint_step` (the train kernel with the align term switched on at run time: AwesomeImageLoss with its extra penalty)
    for every shape at the joint tests' smallest size, 48 x 48, against the oracle: forward, the composite loss, autograd, one Adam
    step, the clamp.  Bars of test_icnn_joint_step_with_extra_penalty_matches_oracle: loss terms rel 2e-5, d loss / d seg, the prior's
    logits, the updated row - and both Adam moments, which unlike the row (every parameter moves by about lr in a first Adam step)
    carry the size of every gradient."""
    A = amd
    from awesome_amd import _lib as L
    from awesome_amd import joint as J
    dev = torch.device("cuda:0")
    S, lr, gamma, alpha, beta = 48, 1e-3, 0.1, 0.7, 100.0
    spec = A.IcnnSpec(n_hidden=h, in_features=C, n_layers=1)
    g = torch.Generator().manual_seed(300 + h + C)
    p0 = {k: (torch.rand(shp, generator=g) - 0.45) * 0.3 for k, shp in spec.keys_shapes()}
    n = S * S
    seg = torch.rand(n, generator=g) * 0.9 + 0.05
    tgt = (torch.rand(n, generator=g) > 0.7).float()
    grid = (O.positional_grid(S, S) if C == 2 else O.positional_grid(S, S, 0.4, 1.0))[None]
    # ---- oracle
    pt = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    seg_t = seg.clone().requires_grad_(True)
    logits_ref = O.icnn_forward_image(pt, grid).reshape(-1)
    prior = torch.sigmoid(logits_ref)
    crit = O.weighted_loss(seg_t, tgt, kind="bce", mode="none")
    pcrit = O.weighted_loss(prior, tgt, kind="bce", mode="none")
    align = torch.mean((prior - (seg_t > 0.5).float()) ** 2)
    loss_ref = gamma * (crit + alpha * pcrit) + beta * align
    loss_ref.backward()
    p1 = {k: v.detach().clone() for k, v in p0.items()}
    st = O.AdamState(p1)
    O.adam_step(p1, {k: pt[k].grad for k in p0}, st, lr)
    O.icnn_enforce_convexity(p1)
    # ---- the fused step
    desc = J.joint_desc(kind="bce", weight_mode="none", alpha=alpha, beta=beta, form=L.JOINT_AWESOME_IMAGE, prior_kind="bce",
                        prior_weight_mode="none", gamma=gamma, extra_penalty=True)
    row = A.pack_state_dict(spec, p0, dev).clone()
    P = spec.n_params
    opt = torch.zeros(2 * P + 8, device=dev)
    res = J.joint_step(spec, row, opt, A.Grid.from_image_grid(grid.to(dev)), seg.to(dev), tgt.to(dev), desc, step=1, lr=lr, optimizer="adam")
    lo = res.loss.cpu()
    assert int(res.status[0]) == 0
    np.testing.assert_allclose(lo[0].item(), loss_ref.item(), rtol=2e-5)
    np.testing.assert_allclose(lo[1].item(), crit.item(), rtol=2e-5)
    np.testing.assert_allclose(lo[2].item(), align.item(), rtol=2e-5)
    ds_ref = seg_t.grad.numpy()
    np.testing.assert_allclose(res.dseg.cpu().numpy(), ds_ref, rtol=5e-5, atol=1e-7 * float(np.abs(ds_ref).max()))
    np.testing.assert_allclose(res.prior_logits.cpu().numpy(), logits_ref.detach().numpy(), rtol=0, atol=5e-6)
    np.testing.assert_allclose(row.cpu().numpy(), A.pack_state_dict(spec, p1).numpy(), rtol=1e-3, atol=2e-5)
    for got, ref in ((opt[:P], st.m), (opt[P:2 * P], st.v)):
        ref = A.pack_state_dict(spec, ref).numpy()
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * float(np.abs(ref).max()))
