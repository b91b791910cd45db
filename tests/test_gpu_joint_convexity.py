"""The fused joint step for the convexity benchmark's losses (JointTrainer(fused_convexity_losses=True), inrfit_joint_prior_step):
AwesomeImageLoss, AwesomeImageLossJoint, AwesomeLoss and AwesomeLossJoint split into a segmentation share evaluated in torch (any
criterion; GradientPenaltyLoss's second-order penalty included) and the prior's share in the step kernel (masked data term + hard /
soft align term).  Checked against JointTrainer's autograd path from identical starting points - losses, segmentation-parameter
gradients and weights, prior rows, the shared moments - and at the C ABI against the existing fused step and closed forms.
Tolerances as in tests/test_gpu_joint.py.

Targets outside [0, 1] never reach torch's BCELoss here (torch refuses them); the image cases mask the noneclass 2 on both channels,
and the plain-BCELoss-on-2 prior form is checked at the C ABI."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _ImageSeg(torch.nn.Module):
    """conv over (image, features): the gradient penalties (xygrad on the features, rgbgrad on the image) see both inputs."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(2, 1, 3, padding=1)

    def forward(self, image, feat, *args, **kwargs):
        return self.conv(torch.cat([image, feat], dim=1))


class _PixelSeg(torch.nn.Module):
    def __init__(self, f=5):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(f, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))

    def forward(self, x, *args, **kwargs):
        return self.net(x)


PRIORS = {"h130_l1": lambda: __import__("awesome_amd.model", fromlist=["ConvexNet"]).ConvexNet(n_hidden=130, in_channels=2),
          "h64_l2": lambda: __import__("awesome_amd.model", fromlist=["ConvexNextNet"]).ConvexNextNet(n_hidden=64, in_features=2,
                                                                                                      n_hidden_layers=2)}


def _gpl(penalty):
    from awesome_amd.measures import GradientPenaltyLoss
    return GradientPenaltyLoss(torch.nn.BCELoss(), apply_gradient_penalty=penalty, xygrad=0.01, rgbgrad=0.01, noneclass=2.0)


def _loss(which, sp=0.8):
    from awesome_amd.measures import AwesomeImageLoss, AwesomeImageLossJoint, AwesomeLoss, AwesomeLossJoint, GradientPenaltyLoss
    if which == "image":       # the class calls its criteria without kwargs: the penalty stays off, the noneclass mask on
        return AwesomeImageLoss(criterion=_gpl(False), prior_criterion=GradientPenaltyLoss(torch.nn.BCELoss(), noneclass=2.0),
                                alpha=0.7, beta=100.0, gamma=0.1)
    if which == "image_joint":
        return AwesomeImageLossJoint(criterion=_gpl(True), alpha=0.7, beta=3.0, gamma=0.2)
    if which == "pixel":
        return AwesomeLoss(alpha=0.6, scribble_percentage=sp)
    return AwesomeLossJoint(alpha=0.6, beta=3.0, gamma=0.2, scribble_percentage=sp)


def _data(dev, pixel, n_items=2, H=20, W=23, n=1003, sp=0.8, seed=4):
    g = torch.Generator().manual_seed(seed)
    items = []
    for _ in range(n_items):
        if pixel:
            x = torch.rand(1, n, 5, generator=g)
            n_scr = int(n * sp // 1)
            t = (torch.rand(1, n_scr, 1, generator=g) > 0.6).float()
            items.append(((x.to(dev),), t.to(dev)))
        else:
            img = torch.rand(1, 1, H, W, generator=g).to(dev).requires_grad_(True)
            feat = torch.rand(1, 1, H, W, generator=g).to(dev).requires_grad_(True)
            ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
            xy = torch.stack([xs, ys])[None].to(dev)
            t = torch.randint(0, 3, (1, 1, H, W), generator=g).float()    # 0 / 1 and the noneclass 2
            items.append(((img, feat, xy), t.to(dev)))
    return items


def _run(dev, which, prior, fused, schedule, opt_type=torch.optim.Adam, lr=2e-3, sp=0.8, n=1003, toggle=None, seed=4):
    """Joint steps from identical starting points.  schedule: [(steps, phase)], phase in before / after / map.  toggle: {step index:
    fused_convexity_losses} switched before that step (the moment hand-over).  -> dict of what the comparison needs."""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    pixel = which.startswith("pixel")
    torch.manual_seed(seed)
    factory = PRIORS[prior]
    seg = _PixelSeg() if pixel else _ImageSeg()
    wrapper = (WrapperModule(seg, factory(), prior_arg_mode="xy_c_preattached", input_mode="pixel") if pixel
               else WrapperModule(seg, factory())).to(dev)
    items = _data(dev, pixel, n=n, sp=sp, seed=seed)
    bank = PriorBank(lambda: factory().to(dev), n_images=len(items), device=dev)
    for k in range(len(items)):
        bank.row(k)
    opt = opt_type(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=lr)
    crit = _loss(which, sp)
    tr = JointTrainer(wrapper, bank, crit, opt, fused=fused, fused_convexity_losses=True)
    losses, paths, s = [], [], 0
    for steps, phase in schedule:
        crit.extra_penalty = phase == "after"
        if hasattr(crit, "map_initially_on_segmentation"):
            crit.map_initially_on_segmentation = phase == "map"
        for _ in range(steps):
            if toggle and s in toggle:
                tr.fused_convexity_losses = toggle[s]
            i = s % len(items)
            inputs, target = items[i]
            loss, out = tr.perform_step(i, inputs, target)
            losses.append(float(loss))
            paths.append(tr._path)
            s += 1
    if tr._fused_plan is not None and tr._path == "fused":
        k1, k2 = tr._moment_keys()
        mom = torch.cat([torch.cat([m.reshape(-1), v.reshape(-1)]) for _, m, v in tr._flat_moment_views(tr._fused_plan)])
    else:
        k1, k2 = ("exp_avg", "exp_inf") if opt_type is torch.optim.Adamax else ("exp_avg", "exp_avg_sq")
        mom = torch.cat([torch.cat([opt.state[p][k1].reshape(-1), opt.state[p][k2].reshape(-1)])
                         for p in _ordered_parameters(wrapper.prior_module)])
    return dict(losses=losses, paths=paths, out=out.detach().cpu(), rows=bank.params.detach().cpu().clone(),
                seg_w=[p.detach().cpu().clone() for p in seg.parameters()],
                seg_g=[p.grad.detach().cpu().clone() for p in seg.parameters()], mom=mom.detach().cpu(), trainer=tr)


def _assert_same(f, a):
    np.testing.assert_allclose(f["losses"], a["losses"], rtol=2e-5, atol=1e-7)
    for wf, wa in zip(f["seg_w"], a["seg_w"]):
        np.testing.assert_allclose(wf.numpy(), wa.numpy(), rtol=2e-4, atol=2e-6)
    for gf, ga in zip(f["seg_g"], a["seg_g"]):
        np.testing.assert_allclose(gf.numpy(), ga.numpy(), rtol=1e-3, atol=2e-5 * float(ga.abs().max()) + 1e-9)
    np.testing.assert_allclose(f["rows"].numpy(), a["rows"].numpy(), rtol=1e-3, atol=2e-5)
    m = a["mom"].abs().max()
    np.testing.assert_allclose(f["mom"].numpy(), a["mom"].numpy(), rtol=1e-3, atol=2e-4 * float(m))
    np.testing.assert_allclose(f["out"].numpy(), a["out"].numpy(), rtol=1e-4, atol=2e-5)


CASES = [(w, p, o) for w in ("image", "image_joint", "pixel", "pixel_joint") for p in ("h130_l1", "h64_l2") for o in ("adam", "adamax")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(c) for c in CASES])
def test_fused_convexity_step_matches_autograd(dev, case):
    """10 joint steps, the extra-penalty hook firing at step 5 (AwesomeImageLossJoint: 3 more with map_initially_on_segmentation
    before): every step fused, and everything the step touches matches the autograd path."""
    which, prior, o = case
    opt_type = torch.optim.Adam if o == "adam" else torch.optim.Adamax
    schedule = [(5, "before"), (5, "after")] + ([(3, "map")] if which == "image_joint" else [])
    f = _run(dev, which, prior, True, schedule, opt_type=opt_type)
    a = _run(dev, which, prior, False, schedule, opt_type=opt_type)
    total = sum(s for s, _ in schedule)
    assert f["paths"] == ["fused"] * total and a["paths"] == ["autograd"] * total
    assert int(f["trainer"].last_status[0]) == 0
    _assert_same(f, a)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["pixel", "pixel_joint"])
@pytest.mark.parametrize("sp", [0.8, 1.0])
def test_pixel_mode_scribble_percentage(dev, which, sp):
    """Pixel mode, n = 997 (no multiple of any tile), scribble_percentage 0.8 and 1.0 (the align term is absent at 1.0)."""
    schedule = [(2, "before"), (3, "after")]
    f = _run(dev, which, "h130_l1", True, schedule, sp=sp, n=997)
    a = _run(dev, which, "h130_l1", False, schedule, sp=sp, n=997)
    assert f["paths"] == ["fused"] * 5
    _assert_same(f, a)


@pytest.mark.gpu
def test_moments_hand_over_between_paths(dev):
    """Steps 0-2 autograd (the keyword switched off), 3-6 fused, 7-8 autograd again: the shared moments follow each step."""
    schedule = [(5, "before"), (4, "after")]
    toggle = {0: False, 3: True, 7: False}
    f = _run(dev, "image_joint", "h130_l1", True, schedule, toggle=toggle)
    a = _run(dev, "image_joint", "h130_l1", False, schedule)
    assert f["paths"] == ["autograd"] * 3 + ["fused"] * 4 + ["autograd"] * 2
    _assert_same(f, a)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["image_joint", "pixel_joint"])
def test_joint_losses_without_a_joint_desc_build_fused(dev, which):
    """AwesomeImageLossJoint / AwesomeLossJoint have no inrfit_joint_step form: with the keyword, fused=True builds and steps fused."""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ConvexNet, WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    pixel = which.startswith("pixel")
    seg = _PixelSeg() if pixel else _ImageSeg()
    wrapper = (WrapperModule(seg, ConvexNet(), prior_arg_mode="xy_c_preattached", input_mode="pixel") if pixel
               else WrapperModule(seg, ConvexNet())).to(dev)
    bank = PriorBank(lambda: ConvexNet().to(dev), n_images=1, device=dev)
    opt = torch.optim.Adam(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    with pytest.raises(ValueError):
        JointTrainer(wrapper, bank, _loss(which), opt, fused=True)
    tr = JointTrainer(wrapper, bank, _loss(which), opt, fused=True, fused_convexity_losses=True)
    inputs, target = _data(dev, pixel, n_items=1)[0]
    loss, out = tr.perform_step(0, inputs, target)
    assert tr._path == "fused" and bool(torch.isfinite(loss))
    assert out.shape == ((1, 1003, 2) if pixel else (1, 2, 20, 23))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------


def _abi_state(dev, h=130, nl=1, S=24, seed=1):
    import awesome_amd as A
    spec = A.IcnnSpec(n_hidden=h, in_features=2, n_layers=nl)
    g = torch.Generator().manual_seed(seed)
    p0 = {k: (torch.rand(shp, generator=g) - 0.45) * 0.3 for k, shp in spec.keys_shapes()}
    row = A.pack_state_dict(spec, p0, dev).clone()
    grid = A.Grid.linspace(S, S, dev)
    seg = (torch.rand(S * S, generator=g) * 0.9 + 0.05).to(dev)
    return spec, row, grid, seg, g


@pytest.mark.gpu
def test_plain_bce_prior_on_targets_with_2(dev):
    """AwesomeImageLoss's default prior BCELoss reads targets of 2 as they are (no mask): the prior step equals the prior half of
    the existing AWESOME_IMAGE joint step (same state, same targets) and the closed form on its own logits."""
    from awesome_amd import _lib as L
    from awesome_amd import joint as J
    spec, row, grid, seg, g = _abi_state(dev)
    n = seg.numel()
    tgt = torch.randint(0, 3, (n,), generator=g).float().to(dev)
    alpha = 0.7
    row_a, opt_a = row.clone(), torch.zeros(2 * spec.n_params + 8, device=dev)
    row_b, opt_b = row.clone(), torch.zeros_like(opt_a)
    d_old = J.joint_desc(kind="bce", weight_mode="none", alpha=alpha, form=L.JOINT_AWESOME_IMAGE, prior_kind="bce", prior_weight_mode="none")
    old = J.joint_step(spec, row_a, opt_a, grid, seg, tgt, d_old, step=1, lr=1e-3)
    new = J.joint_prior_step(spec, row_b, opt_b, grid, seg, tgt, J.joint_prior_desc("bce", c_data=alpha), step=1, lr=1e-3)
    assert int(new.status[0]) == 0 and int(old.status[0]) == 0
    assert torch.equal(new.prior_logits, old.prior_logits)
    p = torch.sigmoid(new.prior_logits.double())
    t = tgt.double()
    ref = alpha * torch.mean(-(t * torch.clamp(torch.log(p), min=-100) + (1 - t) * torch.clamp(torch.log(1 - p), min=-100)))
    assert float(new.loss[1]) == pytest.approx(float(ref), rel=2e-5)
    assert float(new.loss[0]) == pytest.approx(float(old.loss[0] - old.loss[1]), rel=2e-5)   # no seg_term: the prior's share
    np.testing.assert_allclose(row_b.cpu().numpy(), row_a.cpu().numpy(), rtol=1e-4, atol=1e-6)
    P2 = 2 * spec.n_params    # the moments (the header's loss bookkeeping holds each call's own loss column)
    np.testing.assert_allclose(opt_b[:P2].cpu().numpy(), opt_a[:P2].cpu().numpy(), rtol=1e-3, atol=1e-9)
    assert float(new.dseg.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("nl,h", [(1, 130), (2, 64)])
def test_masked_data_term_and_soft_align_closed_form(dev, nl, h):
    """data_count < n with the targets holding only data_count values, a noneclass, the soft align on [align_begin, n): loss_out
    and dseg against closed forms on the step's own logits; a NaN prior-side input at a masked point stays out of the sum."""
    from awesome_amd import _lib as L
    from awesome_amd import joint as J
    spec, row, grid, seg, g = _abi_state(dev, h=h, nl=nl, S=23)
    n = seg.numel()
    nd, ab = 401, 130
    tgt = torch.randint(0, 3, (nd,), generator=g).float().to(dev)
    beta, cd = 3.0, 0.35
    st = torch.tensor([0.25], device=dev)
    desc = J.joint_prior_desc("se", "sssdms", noneclass=2.0, data_count=nd, c_data=cd, align_rule=L.ALIGN_SOFT, beta=beta, align_begin=ab)
    opt = torch.zeros(2 * spec.n_params + 8, device=dev)
    res = J.joint_prior_step(spec, row, opt, grid, seg, tgt, desc, step=1, lr=1e-3, seg_term=st)
    p = torch.sigmoid(res.prior_logits.double())
    t = tgt.double()
    keep = t != 2
    pk, tk = p[:nd][keep], t[keep]
    nfg = (tk < 0.5).sum().double()
    w = torch.round(((keep.sum() - nfg) / nfg) / 10) + 1
    wt = torch.where(tk < 0.5, w, torch.ones_like(tk))
    data = cd * torch.sum((tk - pk) ** 2 * wt) / keep.sum()
    s = seg.double()
    align = torch.mean((p[ab:] - s[ab:]) ** 2)
    assert float(res.loss[1]) == pytest.approx(float(data), rel=2e-5)
    assert float(res.loss[2]) == pytest.approx(float(align), rel=2e-5)
    assert float(res.loss[0]) == pytest.approx(float(0.25 + data + beta * align), rel=2e-5)
    assert float(res.loss[3]) == 1.0 and int(res.status[0]) == 0
    dref = torch.zeros_like(s)
    dref[ab:] = -2 * beta * (p[ab:] - s[ab:]) / (n - ab)
    np.testing.assert_allclose(res.dseg.cpu().numpy(), dref.cpu().numpy(), rtol=1e-4, atol=1e-7)


@pytest.mark.gpu
def test_nonfinite_segmentation(dev):
    """A NaN in seg: the hard align counts it as 0 (the step equals the one with 0 there, bit for bit); the soft align freezes the
    row and its moments (status 1).  A NaN segmentation share (seg_term) freezes the row too."""
    from awesome_amd import _lib as L
    from awesome_amd import joint as J
    spec, row, grid, seg, g = _abi_state(dev)
    tgt = (torch.rand(seg.numel(), generator=g) > 0.5).float().to(dev)
    seg_nan, seg_zero = seg.clone(), seg.clone()
    seg_nan[17], seg_zero[17] = float("nan"), 0.0

    def step(s, rule, st=None):
        r, o = row.clone(), torch.zeros(2 * spec.n_params + 8, device=dev)
        res = J.joint_prior_step(spec, r, o, grid, s, tgt, J.joint_prior_desc("bce", c_data=0.1, align_rule=rule, beta=100.0),
                                 step=1, lr=1e-3, seg_term=st)
        return r, o, res

    ra, oa, a = step(seg_nan, L.ALIGN_HARD)
    rb, ob, b = step(seg_zero, L.ALIGN_HARD)
    assert int(a.status[0]) == 0 and torch.isfinite(a.loss).all()
    assert torch.equal(ra, rb) and torch.equal(oa, ob) and torch.equal(a.loss, b.loss)
    rs, os_, s = step(seg_nan, L.ALIGN_SOFT)
    assert int(s.status[0]) == 1 and torch.equal(rs, row) and float(os_[: 2 * spec.n_params].abs().sum()) == 0.0
    rt, ot, t = step(seg, L.ALIGN_NONE, st=torch.tensor([float("nan")], device=dev))
    assert int(t.status[0]) == 1 and torch.equal(rt, row) and not bool(torch.isfinite(t.loss[3]))


@pytest.mark.gpu
def test_fused_convexity_steps_are_deterministic(dev):
    """Two identical 10-step runs (soft align, noneclass, data_count < n; ConvexNet h = 130): bit-equal rows, moments, losses, dseg."""
    from awesome_amd import _lib as L
    from awesome_amd import joint as J
    spec, row0, grid, seg, g = _abi_state(dev, S=64)
    n = seg.numel()
    tgt = torch.randint(0, 3, (3000,), generator=g).float().to(dev)
    desc = J.joint_prior_desc("bce", noneclass=2.0, data_count=3000, c_data=0.2, align_rule=L.ALIGN_SOFT, beta=3.0, align_begin=n - 3000)

    def run():
        row, opt = row0.clone(), torch.zeros(2 * spec.n_params + 8, device=dev)
        out = [J.joint_prior_step(spec, row, opt, grid, seg, tgt, desc, step=t, lr=1e-3) for t in range(1, 11)]
        return row, opt, torch.stack([r.loss.clone() for r in out]), out[-1].dseg.clone()

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_layer_by_layer_shapes_are_refused(dev):
    """A shape without a fused kernel (h = 256): INR_EUNSUPPORTED, nothing launched."""
    import awesome_amd as A
    from awesome_amd import _lib as L
    from awesome_amd import joint as J
    spec = A.IcnnSpec(n_hidden=256, in_features=2, n_layers=1)
    grid = A.Grid.linspace(8, 8, dev)
    row = torch.zeros(spec.n_params, device=dev)
    opt = torch.zeros(2 * spec.n_params + 8, device=dev)
    with pytest.raises(L.InrfitError):
        J.joint_prior_step(spec, row, opt, grid, torch.rand(64, device=dev), torch.rand(64, device=dev), J.joint_prior_desc(), step=1, lr=1e-3)
