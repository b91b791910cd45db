"""The convexity benchmark's FCNet segmentation step in HIP (awesome_amd.fcseg, include/inrfit.h inrfit_fcseg_*; routing:
JointTrainer(fused_convexity_losses=True, fused_segmentation=True) in pixel mode).

At the C ABI the logits, the share g * mean BCE(s[:data_count], t) and every parameter gradient of share + sum(dseg * s) are compared
with float64 torch autograd on the CPU.  Bars (tests/test_gpu_cnnseg.py::_compare): logits rtol 1e-4 / atol 1e-5 * max, loss rel 2e-5,
each parameter gradient within 1e-4 * max|g|.

How the rows are drawn (a condition on the inputs, not a measurement): a ReLU whose pre-activation is within float32 rounding of zero
may take the other branch in float32 than in float64, and one such row moves a weight gradient by about 1 / n of its size - more than
the bar at these n.  So a pool of rows is drawn (1.1 n of them, at least 4096 so that the share below means something at small n), the
net is evaluated in float64, every row with a hidden |pre-activation| below 1e-5 * that layer's largest is discarded and the first n of
the rest are kept: the kernel sees exactly n rows and every one is compared.  The discarded share must stay below 1 %.

Through JointTrainer the fused segmentation share is compared with the torch share of the same fused joint step over 5 steps (unfiltered
inputs, the bars of test_gpu_cnnseg.py's trainer comparison)."""
import json
import math
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


def _net(F, depth, seed=1, in_type="rgbxy"):
    from awesome_amd.model import FCNet
    torch.manual_seed(seed)
    return FCNet(in_chn=F, out_chn=1, width=16, depth=depth, in_type=in_type)


def _rows(net, n, F, seed):
    """n rows uniform in [0, 1) none of which sits on a ReLU kink of `net` (module docstring); -> (rows float32, discarded share)."""
    g = torch.Generator().manual_seed(seed)
    m = max(int(math.ceil(1.1 * n)), 4096)
    pool = torch.rand(m, F, generator=g)
    keep = torch.ones(m, dtype=torch.bool)
    with torch.no_grad():
        a = pool.double()
        lins = [l for l in net.linear_layers()]
        for lin in lins[:-1]:
            pre = a @ lin.weight.double().t() + lin.bias.double()
            keep &= (pre.abs() >= 1e-5 * pre.abs().max()).all(dim=1)
            a = torch.relu(pre)
    share = 1.0 - float(keep.sum()) / m
    rows = pool[keep][:n]
    assert rows.shape[0] == n
    return rows.contiguous(), share


def _reference(net, rows, t, dseg, g, inversion, count):
    net64 = _net(net.in_chn, net.depth)
    net64.load_state_dict(net.state_dict())
    net64 = net64.double()
    ic = min(3, net.in_chn)
    x = rows.double()
    f = net64(x[:, :ic], x[:, ic:])
    sg = torch.sigmoid(f)
    s = 1 - sg if inversion else sg
    share = g * torch.nn.functional.binary_cross_entropy(s[:count], t.double())
    loss = share if dseg is None else share + (dseg.double() * s).sum()
    grads = torch.autograd.grad(loss, list(net64.parameters()))
    return f.detach(), share.detach(), [x.detach() for x in grads]


def _compare(fwd, st, ref_f, ref_loss, ref_grads, net, label):
    assert int(st.status[0]) == 0
    ref_f = ref_f.reshape(-1)
    np.testing.assert_allclose(fwd.logits.cpu().double().numpy(), ref_f.numpy(), rtol=1e-4, atol=1e-5 * float(ref_f.abs().max()))
    print(label, "loss", float(fwd.loss[0]), float(ref_loss))
    assert float(fwd.loss[0]) == pytest.approx(float(ref_loss), rel=2e-5)
    assert float(st.loss[0]) == float(fwd.loss[0])
    off = 0
    for p, r in zip(net.parameters(), ref_grads):
        got = st.grads[off:off + p.numel()].view_as(p).cpu().double()
        off += p.numel()
        err = float((got - r).abs().max())
        print(label, tuple(p.shape), "err / max|g|", err / (float(r.abs().max()) + 1e-300))
        assert err <= 1e-4 * float(r.abs().max()) + 1e-12, (label, tuple(p.shape), err, float(r.abs().max()))
    assert off == st.grads.numel()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 4097, 90000])
@pytest.mark.parametrize("F", [1, 5, 8])
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_fcseg_step_matches_float64_autograd(dev, depth, F, n):
    from awesome_amd import fcseg as FS
    net = _net(F, depth, seed=10 * depth + F)
    rows, share = _rows(net, n, F, seed=100 + n % 97 + F)
    print("discarded share", share)
    assert share <= 0.01
    g = torch.Generator().manual_seed(7)
    ic = min(3, F)
    dnet = _net(F, depth)
    dnet.load_state_dict(net.state_dict())
    dnet = dnet.to(dev)
    image, feat = rows[:, :ic].contiguous().to(dev), (rows[:, ic:].contiguous().to(dev) if F > ic else None)
    for count in sorted({0, int(math.floor(0.8 * n))}):
        cnt = count or n
        t = torch.randint(0, 2, (cnt, 1), generator=g).float()
        for inversion in (False, True):
            for with_dseg in (False, True):
                dseg = torch.randn(n, 1, generator=g) * 1e-3 if with_dseg else None
                ref = _reference(net, rows, t, dseg, 0.7, inversion, cnt)
                desc = FS.make_desc(dnet, ic, n, data_count=count, inversion=inversion, g=0.7)
                fwd = FS.forward(dnet, desc, image, feat, t.to(dev))
                dd = None if dseg is None else dseg.to(dev)
                st = FS.step(dnet, desc, image, feat, t.to(dev), dseg=dd, reuse_forward=True)
                alone = FS.step(dnet, desc, image, feat, t.to(dev), dseg=dd, reuse_forward=False)
                assert torch.equal(st.grads, alone.grads) and torch.equal(st.loss, alone.loss)
                assert torch.equal(alone.seg, fwd.seg) and torch.equal(alone.logits, fwd.logits)
                sg = torch.sigmoid(ref[0].reshape(-1))
                np.testing.assert_allclose(fwd.seg.cpu().double().numpy(), (1 - sg if inversion else sg).numpy(), rtol=1e-5, atol=1e-6)
                _compare(fwd, st, *ref, dnet, f"d{depth} F{F} n{n} count{count} inv{int(inversion)} dseg{int(with_dseg)}")


@pytest.mark.gpu
def test_fcseg_forward_without_a_target_is_the_evaluation_forward(dev):
    from awesome_amd import fcseg as FS
    net = _net(5, 3).to(dev)
    g = torch.Generator().manual_seed(3)
    image, feat = torch.rand(90000, 3, generator=g).to(dev), torch.rand(90000, 2, generator=g).to(dev)
    desc = FS.make_desc(net, 3, 90000)
    out = FS.forward(net, desc, image, feat)
    assert out.loss is None
    with torch.no_grad():
        ref = net(image, feat).reshape(-1)
    np.testing.assert_allclose(out.logits.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-5 * float(ref.abs().max()))
    np.testing.assert_allclose(out.seg.cpu().numpy(), torch.sigmoid(ref).cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_fcseg_step_is_bit_reproducible(dev):
    from awesome_amd import fcseg as FS
    net = _net(5, 3).to(dev)
    g = torch.Generator().manual_seed(9)
    n = 90000
    image, feat = torch.rand(n, 3, generator=g).to(dev), torch.rand(n, 2, generator=g).to(dev)
    t = torch.randint(0, 2, (72000, 1), generator=g).float().to(dev)
    dseg = (torch.randn(n, generator=g) * 1e-3).to(dev)
    desc = FS.make_desc(net, 3, n, data_count=72000, g=0.1)
    a = FS.step(net, desc, image, feat, t, dseg=dseg)
    b = FS.step(net, desc, image, feat, t, dseg=dseg)
    assert torch.equal(a.grads, b.grads) and torch.equal(a.loss, b.loss) and torch.equal(a.seg, b.seg)
    assert bool(a.grads.abs().sum() > 0)


@pytest.mark.gpu
def test_nan_row_sets_the_status_and_zeroes_the_gradient(dev):
    from awesome_amd import fcseg as FS
    net = _net(5, 3).to(dev)
    g = torch.Generator().manual_seed(5)
    n = 1000
    image, feat = torch.rand(n, 3, generator=g), torch.rand(n, 2, generator=g)
    image[417, 1] = float("nan")
    t = torch.randint(0, 2, (n, 1), generator=g).float().to(dev)
    desc = FS.make_desc(net, 3, n)
    st = FS.step(net, desc, image.to(dev), feat.to(dev), t)      # no exception: the failure is a device flag
    assert int(st.status[0]) == 1
    assert bool((st.grads == 0).all())
    assert not math.isfinite(float(st.loss[0]))


@pytest.mark.gpu
def test_unsupported_shapes_keep_the_torch_path(dev):
    from awesome_amd import fcseg as FS
    from awesome_amd.model import FCNet
    assert FS.net_supported(FCNet(in_chn=8, out_chn=1, width=16, depth=3, in_type="rgbxy").to(dev))
    assert FS.net_supported(FCNet(in_chn=3, out_chn=1, width=16, depth=0, in_type="rgb").to(dev))
    assert not FS.net_supported(FCNet(in_chn=5, out_chn=1, width=32, depth=3, in_type="rgbxy").to(dev))
    assert not FS.net_supported(FCNet(in_chn=5, out_chn=1, width=16, depth=4, in_type="rgbxy").to(dev))
    assert not FS.net_supported(FCNet(in_chn=9, out_chn=1, width=16, depth=3, in_type="rgbxy").to(dev))
    assert not FS.net_supported(FCNet(in_chn=5, out_chn=1, width=16, depth=3, in_type="rgbxy").to(dev).double())


# ---- through JointTrainer -------------------------------------------------------------------------------------------------------

N_SCR, N_RAND, SP = 400, 100, 0.8


def _loss(which):
    from awesome_amd.measures import AwesomeLoss, AwesomeLossJoint
    if which == "awesome":
        return AwesomeLoss(criterion=torch.nn.BCELoss(), alpha=1.0, scribble_percentage=SP)
    return AwesomeLossJoint(criterion=torch.nn.BCELoss(), alpha=1.0, beta=1.0, gamma=1.0, scribble_percentage=SP)


def _run(dev, which, mode, phase, fused_seg, steps=5, nan=False):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ConvexNet, WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    n = N_SCR + N_RAND
    # param_clean_grid: (rgb, xy features, clean xy) rows into an 'rgbxy' net; xy_c_preattached: one (n, 5) input whose first two
    # features are the coordinates, into an 'rgb' net (its whole input is the "image")
    net = _net(5, 3, seed=7, in_type="rgbxy" if mode == "param_clean_grid" else "rgb")
    torch.manual_seed(11)
    wrapper = WrapperModule(net, ConvexNet(n_hidden=130, in_channels=2), use_segmentation_output_inversion=True, input_mode="pixel",
                            prior_arg_mode=mode).to(dev)
    bank = PriorBank(lambda: ConvexNet(n_hidden=130, in_channels=2).to(dev), n_images=2, device=dev)
    for k in range(2):
        bank.row(k)
    items = []
    for k in range(2):
        g = torch.Generator().manual_seed(20 + k)
        rgb, xy = torch.rand(1, n, 3, generator=g), torch.rand(1, n, 2, generator=g)
        t = torch.randint(0, 2, (1, N_SCR, 1), generator=g).float()
        if nan and k == 0:
            rgb[0, 17, 1] = float("nan")
        if mode == "param_clean_grid":
            items.append(((rgb.to(dev), xy.clone().to(dev), xy.to(dev)), t.to(dev)))
        else:
            items.append(((torch.cat([xy, rgb], dim=-1).to(dev),), t.to(dev)))
    rows0 = bank.params.detach().cpu().clone()
    opt = torch.optim.Adam(list(net.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    crit = _loss(which)
    crit.extra_penalty = phase == "after"
    tr = JointTrainer(wrapper, bank, crit, opt, fused=True, fused_convexity_losses=True, fused_segmentation=fused_seg)
    losses, paths, statuses, out = [], [], [], None
    for s in range(steps):
        inputs, target = items[s % 2]
        loss, out = tr.perform_step(s % 2, inputs, target)
        losses.append(float(loss))
        paths.append(tr._path)
        statuses.append(None if tr.cnnseg_status is None else int(tr.cnnseg_status[0]))
    return dict(losses=losses, paths=paths, statuses=statuses, rows=bank.params.detach().cpu().clone(), rows0=rows0,
                out=None if out is None else out.detach().cpu(), seg_w=[p.detach().cpu().clone() for p in net.parameters()], tr=tr,
                crit=crit)


@pytest.mark.gpu
@pytest.mark.parametrize("phase", ["before", "after"])
@pytest.mark.parametrize("mode", ["param_clean_grid", "xy_c_preattached"])
@pytest.mark.parametrize("which", ["awesome", "joint"])
def test_fused_segmentation_matches_the_torch_segmentation_share(dev, which, mode, phase):
    f = _run(dev, which, mode, phase, True)
    a = _run(dev, which, mode, phase, False)
    assert f["paths"] == ["fused"] * 5 and a["paths"] == ["fused"] * 5
    assert f["statuses"] == [0] * 5 and a["statuses"] == [None] * 5       # the HIP share ran in f, the torch share in a
    print(which, mode, phase, "losses", f["losses"], a["losses"])
    np.testing.assert_allclose(f["losses"], a["losses"], rtol=2e-5)
    for wf, wa in zip(f["seg_w"], a["seg_w"]):
        assert not torch.equal(wf, torch.zeros_like(wf))
        np.testing.assert_allclose(wf.numpy(), wa.numpy(), rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(f["rows"].numpy(), a["rows"].numpy(), rtol=1e-3, atol=2e-5)
    assert f["out"].shape == a["out"].shape == (1, N_SCR + N_RAND, 2)
    np.testing.assert_allclose(f["out"].numpy(), a["out"].numpy(), rtol=1e-4, atol=2e-5)
    if which == "joint":        # the side effect AwesomeLossJoint's call leaves behind
        assert f["crit"].criterion.apply_gradient_penalty is True


@pytest.mark.gpu
def test_default_routing_keeps_the_torch_share(dev):
    r = _run(dev, "joint", "param_clean_grid", "before", False, steps=1)
    assert r["statuses"] == [None] and r["tr"]._cnn_grads is None


@pytest.mark.gpu
def test_nan_input_zeroes_the_segmentation_gradient(dev):
    r = _run(dev, "joint", "param_clean_grid", "before", True, steps=1, nan=True)
    assert r["statuses"] == [1] and bool(r["tr"].failed)
    for p in r["seg_w"]:
        assert bool(torch.isfinite(p).all())
    assert torch.equal(r["rows"][0], r["rows0"][0])          # the prior's row is frozen
    with pytest.raises(ValueError):
        r["tr"].raise_if_failed()


@pytest.mark.gpu
def test_run_py_fcnet_config_takes_every_joint_step_fused(tmp_path):
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--config-path", os.path.join(ROOT, "config", "c7_fcnet_convexity.yaml"),
           "--output-folder", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    summary = json.loads([line for line in res.stdout.splitlines() if line.startswith("{")][-1])
    print(summary)
    assert summary["joint_steps_fused"] == summary["joint_epochs"] * summary["images"] > 0
    assert summary["extra_penalty"] is True
    first, last = summary["joint_loss_first_last"]
    assert np.isfinite(first) and np.isfinite(last) and last < first
