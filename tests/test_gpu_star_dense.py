"""The star-shape prior's dense full-batch fits (inrfit_star_fit_dense / inrfit_star_loss_grad_dense, csrc/star.h) on the GPU, against
the float64 loop of tests/star_dense_cases.py (oracle.star_shaped_forward / weighted_loss, torch's optimizers and ReduceLROnPlateau):
loss and every gradient at the small and the tile-straddling sizes, 12-step trajectories with the plateau's decisions, continuation,
a pixel on the centre, the non-finite freeze, both meanings of the returned logits, determinism and the quality of a real fit."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import star_dense_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _spec(h):
    from awesome_amd import star as S
    return S.StarSpec(h)


def _problem(h, n_images, x, per_image, seed):
    """n_images states (different parameters), targets (different stars, every second image soft) and coordinates."""
    sds = [SC.make_state(h, seed + 7 * i, offset=(0.02 + 0.01 * i, -0.04 + 0.015 * i)) for i in range(n_images)]
    xs = [x + (0.003 * i if per_image else 0.0) for i in range(n_images)]
    ts = [SC.star_targets(xs[i], centre=(0.03 - 0.02 * i, -0.05 + 0.03 * i), k=5 - i, soft=bool(i % 2)) for i in range(n_images)]
    return sds, xs, ts


# ---- 1. loss and every gradient -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_images,per_image", [(1, False), (3, False), (3, True)], ids=["one", "three-shared", "three-own-grids"])
@pytest.mark.parametrize("height,width", [(24, 20), (33, 29)])
@pytest.mark.parametrize("h", [1, 33, 130])
def test_loss_and_gradients_match_float64(dev, h, height, width, n_images, per_image):
    """SE and BCE, each with every weight mode.  Bars: loss rel 2e-5 / abs 1e-7, gradients rtol 5e-4 with atol 5e-4 max|ref|."""
    from awesome_amd import star as S
    x = SC.grid_rows(height, width)
    sds, xs, ts = _problem(h, n_images, x, per_image, 1000 + h)
    flat = torch.stack([SC.flat_of(sd) for sd in sds]).to(dev)
    coords = (torch.stack(xs) if per_image else x).to(dev)
    targets = torch.stack(ts).to(dev)
    for kind, mode in itertools.product(SC.KINDS, SC.MODES):
        loss, grads = S.star_loss_grad_dense(_spec(h), flat, coords, targets, loss=kind, weight_mode=mode, ratio=SC.RATIO, c_fg=SC.C_FG,
                                             c_bg=SC.C_BG)
        for i in range(n_images):
            rl, rg = SC.ref_loss_grads(sds[i], xs[i], ts[i], kind, mode)
            assert float(loss[i]) == pytest.approx(rl, rel=2e-5, abs=1e-7), (kind, mode, i)
            SC.assert_grads_close(h, grads[i], rg, what=f"{kind}/{mode} image {i}")


@pytest.mark.parametrize("tiles,extra", [(1, 5), (2, 1)], ids=["T+5", "2T+1"])
def test_gradients_across_tile_borders(dev, tiles, extra):
    """N = T + 5 and N = 2 T + 1 explicit coordinate rows, h = 8: every sum crosses a tile border.  The same bars as above; where they
    do not hold, 4 x the error of the same computation in float32 on the CPU against float64 (summation order is what is left) -
    the measured figures are printed and kept in profiles/star_dense_parity.md."""
    from awesome_amd import star as S
    h, T = 8, S.dense_tile_points()
    n = tiles * T + extra
    g = torch.Generator().manual_seed(31 + n)
    x = (torch.rand(n, 2, generator=g) - 0.5)
    sd = SC.make_state(h, 77)
    t = SC.star_targets(x, soft=True)
    flat = SC.flat_of(sd)[None].to(dev)
    for kind, mode in itertools.product(SC.KINDS, SC.MODES):
        loss, grads = S.star_loss_grad_dense(_spec(h), flat, x.to(dev), t[None].to(dev), loss=kind, weight_mode=mode, ratio=SC.RATIO,
                                             c_fg=SC.C_FG, c_bg=SC.C_BG)
        rl, rg = SC.ref_loss_grads(sd, x, t, kind, mode)
        dev_g = SC.unflatten(h, grads[0].cpu())
        err = max(float((dev_g[k].double() - rg[k].reshape(dev_g[k].shape)).abs().max() / rg[k].abs().max().clamp_min(1e-30))
                  for k in SC.PARAM_ORDER)
        print(f"\nstar dense N={n} {kind}/{mode}: loss rel {abs(float(loss[0]) - rl) / abs(rl):.2e}, worst gradient error / max|ref| {err:.2e}")
        assert float(loss[0]) == pytest.approx(rl, rel=2e-5, abs=1e-7), (kind, mode)
        try:
            SC.assert_grads_close(h, grads[0], rg, what=f"{kind}/{mode}")
        except AssertionError:
            _, g32 = SC.ref_loss_grads(sd, x, t, kind, mode, dtype=torch.float32)
            for k in SC.PARAM_ORDER:
                own = float((g32[k].double() - rg[k]).abs().max())       # float32's own error on this tensor
                got = float((dev_g[k].double() - rg[k].reshape(dev_g[k].shape)).abs().max())
                print(f"  {kind}/{mode} {k}: device {got:.3e}, float32 on the CPU {own:.3e}, bar {4 * own:.3e}")
                assert got <= 4.0 * own, (kind, mode, k, got, own)


# ---- 2. trajectories ------------------------------------------------------------------------------------------------------------------
_PLATEAU = dict(patience=2, factor=0.5)
_TRAJ = [("adam", "se", "none"), ("adamax", "bce", "sssdms"), ("adam", "se", "equal")]
# (the seeds: torch's own float32 loop stays within 1 % of the parameter bars against float64 on these cases, and at h = 130 the
#  plateau halves the rate inside the 12 steps in both precisions - properties of the reference, measured on the CPU)
_SHAPES = [(33, 29, 33, 133), (24, 20, 130, 200)]


def _header_lr(res, P):
    return res.opt_state[:, 2 * P + 2].cpu().numpy()


@pytest.mark.parametrize("first", [0, 5, -1], ids=["centre-free", "centre-from-5", "centre-never"])
@pytest.mark.parametrize("optimizer,kind,mode", _TRAJ, ids=["adam-se-none", "adamax-bce-sssdms", "adam-se-equal"])
@pytest.mark.parametrize("height,width,h,seed", _SHAPES, ids=["33x29-h33", "24x20-h130"])
def test_twelve_steps_follow_the_float64_loop(dev, height, width, h, seed, optimizer, kind, mode, first):
    from awesome_amd import star as S
    x = SC.grid_rows(height, width)
    sd = SC.make_state(h, seed)
    t = SC.star_targets(x, soft=kind == "bce")
    ref = SC.RefFit(sd, x, t, kind, mode, optimizer, 1e-2, _PLATEAU, first).run(12)
    spec = _spec(h)
    res = S.star_fit_dense(spec, SC.flat_of(sd)[None].to(dev), x.to(dev), t[None].to(dev), 12, lr=1e-2, loss=kind, weight_mode=mode,
                           optimizer=optimizer, plateau=_PLATEAU, offset_first_step=first)
    assert int(res.status[0]) == 0
    np.testing.assert_allclose(res.loss_hist[0].cpu().numpy(), np.asarray(ref.losses), rtol=5e-4)
    out, want = SC.unflatten(h, res.params[0].cpu()), ref.state()
    for k in SC.PARAM_ORDER:
        np.testing.assert_allclose(out[k].numpy(), want[k].numpy().reshape(out[k].shape), rtol=5e-3, atol=2e-4, err_msg=k)
    assert float(out["W2_r.weight"].min()) >= 0.0
    if first < 0:
        assert torch.equal(out["offset"], sd["offset"])
    assert _header_lr(res, spec.n_params)[0] == np.float32(ref.lr)
    if h == 130:
        assert ref.lr < 1e-2     # the plateau's decisions are really exercised


def test_learning_rate_after_every_call_and_continuation_bits(dev):
    """12 steps in one call and as 5 + 7 continued through opt_state / step0: the same bits; the header's learning rate after every call
    is the reference scheduler's."""
    from awesome_amd import star as S
    height, width, h, seed = _SHAPES[1]
    x, sd = SC.grid_rows(height, width), SC.make_state(h, seed)
    t = SC.star_targets(x)
    spec = _spec(h)
    kw = dict(lr=1e-2, loss="se", weight_mode="none", optimizer="adam", plateau=_PLATEAU, offset_first_step=3)
    whole = S.star_fit_dense(spec, SC.flat_of(sd)[None].to(dev), x.to(dev), t[None].to(dev), 12, **kw)
    ref = SC.RefFit(sd, x, t, "se", "none", "adam", 1e-2, _PLATEAU, 3)
    a = S.star_fit_dense(spec, SC.flat_of(sd)[None].to(dev), x.to(dev), t[None].to(dev), 5, **kw)
    assert _header_lr(a, spec.n_params)[0] == np.float32(ref.run(5).lr)
    b = S.star_fit_dense(spec, a.params, x.to(dev), t[None].to(dev), 7, opt_state=a.opt_state, step0=5, **kw)
    assert _header_lr(b, spec.n_params)[0] == np.float32(ref.run(7).lr) and ref.lr < 1e-2
    assert torch.equal(b.params, whole.params) and torch.equal(b.opt_state, whole.opt_state)
    assert torch.equal(torch.cat([a.loss_hist, b.loss_hist], 1), whole.loss_hist) and torch.equal(b.logits, whole.logits)


# ---- 3. a pixel exactly on the centre ---------------------------------------------------------------------------------------------------
def test_a_pixel_on_the_centre_contributes_nothing_to_the_centres_gradient(dev):
    from awesome_amd import star as S
    h = 33
    x = SC.grid_rows(24, 20)
    sd = SC.make_state(h, 55)
    sd["offset"] = -x[250][None].clone()            # r = 0 at pixel 250, exactly
    assert bool(((x + sd["offset"]) == 0).all(1).sum() == 1)
    t = SC.star_targets(x, centre=tuple(x[250].tolist()))
    loss, grads = S.star_loss_grad_dense(_spec(h), SC.flat_of(sd)[None].to(dev), x.to(dev), t[None].to(dev))
    assert bool(torch.isfinite(grads).all()) and bool(torch.isfinite(loss).all())
    rl, rg = SC.ref_loss_grads(sd, x, t, "se", "none", mask_centre=True)
    assert all(bool(torch.isfinite(v).all()) for v in rg.values())
    assert float(loss[0]) == pytest.approx(rl, rel=2e-5, abs=1e-7)
    SC.assert_grads_close(h, grads[0], rg)
    res = S.star_fit_dense(_spec(h), SC.flat_of(sd)[None].to(dev), x.to(dev), t[None].to(dev), 3, offset_first_step=0)
    assert int(res.status[0]) == 0 and bool(torch.isfinite(res.params).all())
    assert not torch.equal(res.params[0, :2].cpu(), sd["offset"].reshape(-1))     # the centre is free and moved


# ---- 4. a non-finite loss freezes one image ---------------------------------------------------------------------------------------------
def test_a_nan_target_freezes_its_image_alone(dev):
    from awesome_amd import star as S
    h = 33
    x = SC.grid_rows(24, 20)
    sds, _, ts = _problem(h, 3, x, False, 300)
    ts[1] = ts[1].clone()
    ts[1][123] = float("nan")
    spec = _spec(h)
    flat0 = torch.stack([SC.flat_of(sd) for sd in sds]).to(dev)
    opt0 = S.new_dense_opt_state(spec, 3, dev)
    opt0[:, :2 * spec.n_params] = 0.01 * torch.randn(3, 2 * spec.n_params, generator=torch.Generator().manual_seed(1)).abs().to(dev)
    kw = dict(lr=1e-2, optimizer="adamax", plateau=_PLATEAU, offset_first_step=0)
    res = S.star_fit_dense(spec, flat0.clone(), x.to(dev), torch.stack(ts).to(dev), 6, opt_state=opt0.clone(), **kw)
    assert res.status.cpu().tolist() == [0, 1, 0]
    P = spec.n_params
    assert torch.equal(res.params[1], flat0[1]) and torch.equal(res.opt_state[1, :2 * P], opt0[1, :2 * P])
    assert bool(torch.isnan(res.loss_hist[1]).all())
    two = S.star_fit_dense(spec, flat0[[0, 2]].clone(), x.to(dev), torch.stack([ts[0], ts[2]]).to(dev), 6, opt_state=opt0[[0, 2]].clone(), **kw)
    assert two.status.cpu().tolist() == [0, 0]
    assert torch.equal(res.params[[0, 2]], two.params) and torch.equal(res.opt_state[[0, 2]], two.opt_state)
    assert torch.equal(res.loss_hist[[0, 2]], two.loss_hist) and torch.equal(res.logits[[0, 2]], two.logits)
    assert not torch.equal(res.params[0], flat0[0])


# ---- 5. which logits come back ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [True, False], ids=["last-forward", "final-parameters"])
def test_returned_logits(dev, gate):
    from awesome_amd import star as S
    height, width, h, seed = _SHAPES[0]
    x, sd = SC.grid_rows(height, width), SC.make_state(h, seed)
    t = SC.star_targets(x)
    ref = SC.RefFit(sd, x, t, "se", "none", "adam", 1e-2, None, 0).run(6)
    res = S.star_fit_dense(_spec(h), SC.flat_of(sd)[None].to(dev), x.to(dev), t[None].to(dev), 6, lr=1e-2, offset_first_step=0,
                           gate_logits=gate)
    want, other = (ref.last_forward, ref.final_logits()) if gate else (ref.final_logits(), ref.last_forward)
    got = res.logits[0].cpu().double()
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 2e-4 * scale
    assert float((got - other).abs().max()) > 20 * 2e-4 * scale      # the two are told apart by a wide margin
    if not gate:       # ... and are the forward of the returned parameters
        assert torch.equal(res.logits[0], S.star_forward(_spec(h), res.params[0], x.to(dev)))


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------------------
def test_two_runs_across_tiles_give_the_same_bits(dev):
    from awesome_amd import star as S
    h, n = 8, 2 * S.dense_tile_points() + 1
    x = (torch.rand(n, 2, generator=torch.Generator().manual_seed(5)) - 0.5).to(dev)
    t = SC.star_targets(x.cpu(), soft=True)[None].to(dev)
    sd = SC.make_state(h, 9)
    runs = [S.star_fit_dense(_spec(h), SC.flat_of(sd)[None].to(dev), x, t, 4, loss="bce", weight_mode="equal", offset_first_step=0)
            for _ in range(2)]
    grads = [S.star_loss_grad_dense(_spec(h), SC.flat_of(sd)[None].to(dev), x, t, loss="bce", weight_mode="equal") for _ in range(2)]
    assert torch.equal(runs[0].params, runs[1].params) and torch.equal(runs[0].opt_state, runs[1].opt_state)
    assert torch.equal(runs[0].loss_hist, runs[1].loss_hist) and torch.equal(runs[0].logits, runs[1].logits)
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert bool(torch.isfinite(runs[0].params).all()) and not torch.equal(runs[0].params[0].cpu(), SC.flat_of(sd))


# ---- 7. a real fit ------------------------------------------------------------------------------------------------------------------------
def test_fit_of_a_five_armed_star_passes_the_gate_and_is_star_shaped(dev):
    """33 x 29, h = 33, r0 = 0.27, a = 0.09, centre (0.45, 0.55) on the unit grid; Adam 1e-2, SE / none, 600 steps, the centre started on
    the foreground mean and free from step 0.  The reference loop on the CPU ends at IoU 0.950 (float32) / 0.959 (float64); the gate is
    the project's proper_prior_fit_threshold = 0.5.  The device's figure is printed (profiles/star_dense_parity.md keeps it)."""
    from awesome_amd import star as S
    from awesome_amd.model.star_net import foreground_mean
    from oracle import inr_oracle as O
    height, width, h = 33, 29, 33
    x = SC.grid_rows(height, width) + 0.5                      # the unit grid
    t = SC.star_targets(x, centre=(0.45, 0.55), r0=0.27, a=0.09, k=5)
    sd = SC.make_state(h, 600, offset=(0.0, 0.0))
    sd["offset"] = -foreground_mean(x.t().contiguous(), t)[None]
    spec = _spec(h)
    res = S.star_fit_dense(spec, SC.flat_of(sd)[None].to(dev), x.to(dev), t[None].to(dev), 600, lr=1e-2, offset_first_step=0)
    assert int(res.status[0]) == 0
    iou = O.miou_binary((torch.sigmoid(res.logits[0].cpu()) > 0.5).float(), (t > 0.5).float(), invert=True)
    print(f"\nstar dense fit quality: device foreground IoU {iou:.3f} (CPU reference loop: 0.950 float32 / 0.959 float64)")
    assert iou >= 0.5
    centre = -res.params[0, :2]
    reenter = SC.star_rays_reenter(lambda pts: S.star_forward(spec, res.params[0], pts), centre, dev)
    assert reenter <= 0.05, f"{reenter:.3f} of the rays re-enter the region: not star-shaped"
