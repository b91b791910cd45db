"""The convexity benchmark's CNNNet segmentation step in HIP (awesome_amd.cnnseg, include/inrfit.h inrfit_cnnseg_*; routing:
JointTrainer(fused_convexity_losses=True, fused_segmentation=True)).

At the C ABI the logits, the loss g (BCE + penalties) and every gradient of loss + sum(dseg s) are checked against torch autograd's
double backward on the same module: float64 on the CPU at 64 x 80, fp32 on the GPU at 300 x 300 and 37 x 53 (tile edges).  Bars:
loss rel 2e-5, each gradient's max-abs error <= 1e-4 of that gradient's max.  Through JointTrainer the fused step is compared
with the autograd path from the same start over 10 steps with the extra-penalty hook at step 5, and both with the float64 CPU
reference of those steps (tests/trainer_reference.py), step by step with the backbone forced to the reference's state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gpl(xytype, penalty=True, noneclass=2.0, featgrad=0.02):
    from awesome_amd.measures import GradientPenaltyLoss
    return GradientPenaltyLoss(torch.nn.BCELoss(), apply_gradient_penalty=penalty, xygrad=0.01, rgbgrad=0.01, featgrad=featgrad,
                               xytype=xytype, noneclass=noneclass)


def _problem(H, W, raw, noneclass, seed=0):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(1, 3, H, W, generator=g)
    feat = torch.rand(1, raw, H, W, generator=g)
    t = torch.randint(0, 3 if noneclass is not None else 2, (1, 1, H, W), generator=g).float()
    dseg = torch.randn(1, 1, H, W, generator=g) * 1e-3
    return image, feat, t, dseg


def _net(raw, seed=1):
    from awesome_amd.model import CNNNet
    torch.manual_seed(seed)
    return CNNNet(in_chn=3 + raw, out_chn=1, kernel_size=3, width=16, depth=2, in_type="rgbxy")


def _torch_ref(net, image, feat, t, dseg, crit, g, inversion):
    image = image.clone().requires_grad_(True)
    feat = feat.clone().requires_grad_(True)
    f = net(image, feat)
    sg = torch.sigmoid(f)
    s = 1 - sg if inversion else sg
    share = g * crit(s, t, _input=[image, feat])
    loss = share + (dseg * s).sum()
    grads = torch.autograd.grad(loss, list(net.parameters()))
    return f.detach(), share.detach(), [x.detach() for x in grads]


def _hip(net, image, feat, t, dseg, crit, g, inversion, dev):
    from awesome_amd import cnnseg as CS
    form = CS.criterion_form(crit, {"_input": [image, feat]}, 3, net.in_chn)
    desc = CS.make_desc(net, 3, image.shape[-2], image.shape[-1], form, inversion=inversion, g=g)
    fwd = CS.forward(net, desc, image, feat, t)
    st = CS.step(net, desc, image, feat, t, dseg=dseg, reuse_forward=True)
    alone = CS.step(net, desc, image, feat, t, dseg=dseg, reuse_forward=False)
    assert torch.equal(st.grads, alone.grads) and torch.equal(st.loss, alone.loss)
    return fwd, st


def _compare(fwd, st, ref_f, ref_loss, ref_grads, net):
    assert int(st.status[0]) == 0
    ref_f = ref_f.cpu().double()
    np.testing.assert_allclose(fwd.logits.cpu().double().numpy(), ref_f.reshape(-1).numpy(), rtol=1e-4, atol=1e-5 * float(ref_f.abs().max()))
    assert float(fwd.loss[0]) == pytest.approx(float(ref_loss), rel=2e-5)
    assert float(st.loss[0]) == float(fwd.loss[0])
    off = 0
    for p, r in zip(net.parameters(), ref_grads):
        got = st.grads[off:off + p.numel()].view_as(p).cpu().double()
        off += p.numel()
        r = r.cpu().double()
        err = float((got - r).abs().max())
        assert err <= 1e-4 * float(r.abs().max()) + 1e-12, (tuple(p.shape), err, float(r.abs().max()))


ABI_CASES = [(x, pen, nc, inv) for x in ("xy", "feat", "featxy") for pen in (True, False) for nc in (2.0, None) for inv in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ABI_CASES, ids=[f"{x}-pen{int(p)}-nc{int(n is not None)}-inv{int(i)}" for x, p, n, i in ABI_CASES])
def test_cnnseg_step_matches_float64_autograd(dev, case):
    xytype, pen, nc, inv = case
    raw = 2 if xytype == "xy" else 4
    image, feat, t, dseg = _problem(64, 80, raw, nc)
    net = _net(raw)
    crit = _gpl(xytype, pen, nc)
    ref = _torch_ref(net.double(), image.double(), feat, t.double(), dseg.double(), crit, 0.7, inv)
    net = net.float().to(dev)
    fwd, st = _hip(net, image.to(dev), feat.to(dev), t.to(dev), dseg.to(dev), crit, 0.7, inv, dev)
    _compare(fwd, st, *ref, net)


@pytest.mark.gpu
@pytest.mark.parametrize("HW", [(300, 300), (37, 53)])
@pytest.mark.parametrize("xytype", ["xy", "featxy"])
def test_cnnseg_step_matches_fp32_gpu_autograd(dev, HW, xytype):
    raw = 2 if xytype == "xy" else 4
    image, feat, t, dseg = _problem(*HW, raw, 2.0, seed=5)
    net = _net(raw, seed=2).to(dev)
    crit = _gpl(xytype)
    args = (image.to(dev), feat.to(dev), t.to(dev), dseg.to(dev), crit, 1.0, True)
    ref = _torch_ref(net, *args)
    fwd, st = _hip(net, *args, dev)
    _compare(fwd, st, *ref, net)


@pytest.mark.gpu
def test_cnnseg_step_is_bit_reproducible(dev):
    from awesome_amd import cnnseg as CS
    image, feat, t, dseg = [x.to(dev) for x in _problem(300, 300, 2, 2.0, seed=9)]
    net = _net(2).to(dev)
    crit = _gpl("xy")
    form = CS.criterion_form(crit, {"_input": [image, feat]}, 3, net.in_chn)
    desc = CS.make_desc(net, 3, 300, 300, form, g=0.1)
    a = CS.step(net, desc, image, feat, t, dseg=dseg)
    b = CS.step(net, desc, image, feat, t, dseg=dseg)
    assert torch.equal(a.grads, b.grads) and torch.equal(a.loss, b.loss) and torch.equal(a.seg, b.seg)


@pytest.mark.gpu
def test_unsupported_shapes_keep_the_torch_path(dev):
    from awesome_amd import cnnseg as CS
    from awesome_amd.model import CNNNet
    assert not CS.net_supported(CNNNet(in_chn=5, out_chn=1, kernel_size=5, width=16, depth=2, in_type="rgbxy").to(dev))
    assert not CS.net_supported(CNNNet(in_chn=5, out_chn=1, kernel_size=3, width=32, depth=2, in_type="rgbxy").to(dev))
    assert not CS.net_supported(CNNNet(in_chn=5, out_chn=1, kernel_size=3, width=16, depth=4, in_type="rgbxy").to(dev))
    assert not CS.net_supported(CNNNet(in_chn=5, out_chn=1, kernel_size=3, width=16, depth=2, in_type="rgbxy"))   # CPU
    assert CS.net_supported(CNNNet(in_chn=7, out_chn=1, kernel_size=3, width=16, depth=3, in_type="rgbxy").to(dev))
    assert CS.criterion_form(_gpl("xy"), {}, 3, 5) is None           # the penalty without _input: torch raises
    assert CS.criterion_form(torch.nn.MSELoss(), {}, 3, 5) is None


# ---- through JointTrainer -------------------------------------------------------------------------------------------------------


def _loss(which, xytype):
    from awesome_amd.measures import AwesomeImageLoss, AwesomeImageLossJoint, GradientPenaltyLoss
    if which == "image":
        return AwesomeImageLoss(criterion=_gpl(xytype, featgrad=0.0), prior_criterion=GradientPenaltyLoss(torch.nn.BCELoss(), noneclass=2.0),
                                alpha=1.0, beta=100.0, gamma=0.1)
    return AwesomeImageLossJoint(criterion=_gpl(xytype, featgrad=0.0), alpha=1.0, beta=1.0, gamma=1.0)


def _prior():
    from awesome_amd.model import ConvexNet
    return ConvexNet(n_hidden=130, in_channels=2)


def _trainer_problem(xytype, H, W, nan=False):
    """-> (the backbone, the two items), on the CPU."""
    raw = 2 if xytype == "xy" else 4
    net = _net(raw, seed=7)
    items = []
    for k in range(2):
        image, feat, t, _ = _problem(H, W, raw, 2.0, seed=20 + k)
        if nan and k == 0:
            image[0, 0, 3, 4] = float("nan")
        ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        items.append(((image, feat, torch.stack([xs, ys])[None]), t))
    return net, items


def _trainer_ref(which, xytype, steps=10, hook=5, H=40, W=44):
    """The float64 reference of _run's steps (tests/trainer_reference.py), computed once per case: the same seeded construction on the
    CPU - the wrapper's prior, the bank's probe, then the two rows."""
    from awesome_amd.prior_bank import PriorBank
    from tests import trainer_reference as TR

    def make():
        net, items = _trainer_problem(xytype, H, W)
        torch.manual_seed(11)
        _prior()
        bank = PriorBank(_prior, n_images=2, device="cpu")
        rows0 = torch.stack([bank.row(k) for k in range(2)]).clone()
        items = [((im.requires_grad_(True), ft.requires_grad_(True), xy), t) for (im, ft, xy), t in items]
        return dict(net=net, prior_factory=_prior, rows0=rows0, items=items, make_crit=lambda: _loss(which, xytype), hook=hook, lr=1e-3,
                    steps=steps)
    return TR.reference(("cnnseg", which, xytype, steps, hook, H, W), make)


def _run(dev, which, xytype, fused, steps=10, hook=5, nan=False, H=40, W=44, force=None):
    """force: _trainer_ref of the same arguments - after every step the backbone's gradient is kept and its weights and Adam moments are
    set to the reference's (TR.record_and_force).  awesome_amd.cnnseg reads the weights through the module's own pointers on every call
    and keeps no packed copy, so the in-place overwrite is all the forcing needs.  The prior's rows and moments run free."""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    from tests import trainer_reference as TR
    net, cpu_items = _trainer_problem(xytype, H, W, nan)
    torch.manual_seed(11)
    wrapper = WrapperModule(net, _prior(), use_segmentation_output_inversion=True).to(dev)
    bank = PriorBank(lambda: _prior().to(dev), n_images=2, device=dev)
    for k in range(2):
        bank.row(k)
    items = [((image.to(dev).requires_grad_(True), feat.to(dev).requires_grad_(True), xy.to(dev)), t.to(dev))
             for (image, feat, xy), t in cpu_items]
    rows_init = bank.params.detach().cpu().clone()
    assert force is None or torch.equal(rows_init, force["rows0"])
    opt = torch.optim.Adam(list(net.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    crit = _loss(which, xytype)
    # fused: the whole step in HIP; else the autograd path (WrapperModule forward, criterion, backward, optimizer step)
    tr = JointTrainer(wrapper, bank, crit, opt, fused=fused, fused_convexity_losses=True, fused_segmentation=fused)
    losses, statuses, rec = [], [], TR.new_record()
    for s in range(steps):
        crit.extra_penalty = s >= hook
        inputs, target = items[s % 2]
        loss, out = tr.perform_step(s % 2, inputs, target)
        losses.append(float(loss))
        statuses.append(None if tr.cnnseg_status is None else int(tr.cnnseg_status[0]))
        if force is not None:
            TR.record_and_force(rec, net, opt, force, s)
    if steps == 0:
        return dict(rows=rows_init)
    if tr._path == "fused":
        mom = torch.cat([torch.cat([m.reshape(-1), v.reshape(-1)]) for _, m, v in tr._flat_moment_views(tr._fused_plan)])
    else:
        mom = torch.cat([torch.cat([opt.state[p]["exp_avg"].reshape(-1), opt.state[p]["exp_avg_sq"].reshape(-1)])
                         for p in _ordered_parameters(wrapper.prior_module)])
    seg_mom = torch.cat([opt.state[p][k].reshape(-1) for p in net.parameters() for k in ("exp_avg", "exp_avg_sq")])
    return dict(rec, losses=losses, statuses=statuses, rows=bank.params.detach().cpu().clone(), out=out.detach().cpu(),
                seg_w=[p.detach().cpu().clone() for p in net.parameters()], mom=mom.cpu(), seg_mom=seg_mom.cpu(), tr=tr,
                crit=crit)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["image", "joint"])
@pytest.mark.parametrize("xytype", ["xy", "featxy"])
def test_fused_segmentation_matches_the_autograd_segmentation_share(dev, which, xytype):
    f = _run(dev, which, xytype, True)
    a = _run(dev, which, xytype, False)
    assert f["statuses"] == [0] * 10 and a["statuses"] == [None] * 10
    assert f["tr"]._path == "fused" and a["tr"]._path == "autograd"
    np.testing.assert_allclose(f["losses"], a["losses"], rtol=2e-5)
    for wf, wa in zip(f["seg_w"], a["seg_w"]):
        np.testing.assert_allclose(wf.numpy(), wa.numpy(), rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(f["rows"].numpy(), a["rows"].numpy(), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(f["mom"].numpy(), a["mom"].numpy(), rtol=1e-3, atol=2e-4 * float(a["mom"].abs().max()))
    np.testing.assert_allclose(f["seg_mom"].numpy(), a["seg_mom"].numpy(), rtol=1e-3, atol=2e-4 * float(a["seg_mom"].abs().max()))
    np.testing.assert_allclose(f["out"].numpy(), a["out"].numpy(), rtol=1e-4, atol=2e-5)
    if which == "joint":        # the side effect AwesomeImageLossJoint's call leaves behind
        assert f["crit"].criterion.apply_gradient_penalty is True


B_GRAD = 2e-5    # test_fused_segmentation_matches_float64_step_by_step: four times the autograd step's own 2.7e-6, rounded up to one digit


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["image", "joint"])
@pytest.mark.parametrize("xytype", ["xy", "featxy"])
def test_fused_segmentation_matches_float64_step_by_step(dev, which, xytype):
    """The same four cases against the float64 CPU reference of the ten steps (tests/trainer_reference.py), the backbone forced to the
    reference's weights and Adam moments after every step: the fused step (inrfit_cnnseg_step + the fused L = 1 prior step) and the
    autograd step are each a subject.  Per step the loss at rtol 2e-5 and every parameter tensor's gradient at B_GRAD of the
    reference's max; rows, the prior's moments and the last wrapper output at the bars of the test above.  Exact zeros where the
    reference has them (dead ReLU channels) are asked of the fused step only: torch's convolution backward on the GPU leaves about
    1e-11 max|g| in a few such entries, which are held to B_GRAD like the rest.

    B_GRAD = 2e-5: the float32 torch autograd step, the yardstick, is at most 2.7e-6 from the reference over the four cases on the
    MI355X (profiles/NOTES.md), four times that rounded up to one digit.  The fused step's worst is 9.8e-6, on the output
    convolution's bias at step 2 of the featxy cases: one number, the sum of 1760 per-pixel terms of both signs that cancel to 1 / 495
    of the sum of their magnitudes there, so 9.8e-6 of the result is 2e-8 (a third of 2^-24) of what was summed; every other tensor
    of the fused step stays below 4.2e-6."""
    from tests import trainer_reference as TR
    ref = _trainer_ref(which, xytype)
    for fused in (True, False):
        r = _run(dev, which, xytype, fused, force=ref)
        assert r["statuses"] == ([0] if fused else [None]) * 10 and r["tr"]._path == ("fused" if fused else "autograd")
        TR.check_forced(r, ref, B_GRAD, f"{which}-{xytype} " + ("fused" if fused else "autograd"), zeros_exact=fused)
        np.testing.assert_allclose(r["out"].numpy(), ref["out"].numpy(), rtol=1e-4, atol=2e-5)


@pytest.mark.gpu
def test_fused_segmentation_is_deterministic(dev):
    a = _run(dev, "joint", "featxy", True)
    b = _run(dev, "joint", "featxy", True)
    assert a["losses"] == b["losses"]
    assert torch.equal(a["rows"], b["rows"]) and torch.equal(a["mom"], b["mom"]) and torch.equal(a["seg_mom"], b["seg_mom"])
    for x, y in zip(a["seg_w"], b["seg_w"]):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_nan_input_zeroes_the_segmentation_gradient(dev):
    """A NaN in image 0: the share is NaN, status 1, the gradient zero (every weight stays finite), the prior row frozen."""
    from awesome_amd.agent import JointTrainer
    r0 = _run(dev, "image", "xy", True, steps=0)
    rows0 = r0["rows"]
    r = _run(dev, "image", "xy", True, steps=1, nan=True)
    assert r["statuses"] == [1]
    assert bool(r["tr"].failed)
    for p in r["seg_w"]:
        assert bool(torch.isfinite(p).all())
    assert torch.equal(r["rows"][0], rows0[0])
    with pytest.raises(ValueError):
        r["tr"].raise_if_failed()
    with pytest.raises(ValueError):
        JointTrainer(r["tr"].wrapper, r["tr"].bank, r["crit"], r["tr"].optimizer, fused_segmentation=True)


@pytest.mark.gpu
def test_run_py_cnnnet_config_takes_every_joint_step_fused(tmp_path):
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--config-path", os.path.join(ROOT, "config", "c6_cnnnet_convexity.yaml"),
           "--output-folder", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    summary = json.loads([line for line in res.stdout.splitlines() if line.startswith("{")][-1])
    assert summary["joint_steps_fused"] == summary["joint_epochs"] * summary["images"] > 0
    assert all(np.isfinite(summary["joint_loss_first_last"]))
    assert summary["extra_penalty"] is True
