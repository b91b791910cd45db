"""The fused joint step with AwesomeImageLoss's extra penalty on (awesome/measures/awesome_image_loss.py:34-53, switched on by the
runner's hook, awesome/run/awesome_runner.py:351-371):

    loss = gamma (crit(seg, t) + alpha pcrit(prior, t)) + beta mean((prior - [seg > 0.5])^2)

The prior's step kernel evaluates both of its data terms in one pass (the align mode of icnn_step.h / icnn_step2.h).  Checked
against the CPU oracle (forward, the loss, autograd gradients, one optimizer step, the clamp) and against JointTrainer's autograd
path from identical starting points.  Tolerances as in tests/test_gpu_joint.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import inr_oracle as O  # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _desc(kind, mode, pkind, pmode, gamma, alpha, beta, extra_penalty=True):
    from awesome_amd import _lib as L
    from awesome_amd import joint as J
    return J.joint_desc(kind=kind, weight_mode=mode, alpha=alpha, beta=beta, form=L.JOINT_AWESOME_IMAGE, prior_kind=pkind,
                        prior_weight_mode=pmode, gamma=gamma, extra_penalty=extra_penalty)


def _device_joint_loss(seg, prior, target, desc, dev):
    """inrfit_joint_loss on [seg, prior] (1, 2, n): loss_out [4]."""
    from awesome_amd import _lib as L
    from awesome_amd import icnn as K
    out = torch.stack([seg, prior]).reshape(1, 2, -1).contiguous()
    lib = L.load()
    ws = torch.empty(int(lib.inrfit_joint_loss_workspace_bytes(seg.numel())) // 4 + 1, device=dev)
    res = torch.empty(4, device=dev)
    rc = lib.inrfit_joint_loss(out.data_ptr(), target.contiguous().data_ptr(), 1, seg.numel(), C.byref(desc), res.data_ptr(), None,
                               ws.data_ptr(), ws.numel() * 4, K._stream_ptr(dev))
    L.check(rc, "inrfit_joint_loss")
    return res


ICNN_CASES = [
    # (ICNN shape, optimizer, seg criterion, prior criterion, gamma, alpha, beta)
    ((130, 1), "adam", ("bce", "none"), ("bce", "none"), 0.1, 0.7, 100.0),
    ((130, 1), "adamax", ("se", "sssdms"), ("bce", "equal"), 0.3, 0.0, 100.0),
    ((130, 1), "adam", ("bce", "none"), ("se", "sssdms"), 2.0, 0.0, 100.0),
    ((130, 1), "adamax", ("bce", "none"), ("se", "sssdms"), 0.1, 1.3, 100.0),
    ((64, 2), "adam", ("se", "sssdms"), ("bce", "equal"), 0.1, 1.3, 100.0),
    ((64, 2), "adamax", ("bce", "none"), ("bce", "none"), 0.3, 0.0, 100.0),
    ((64, 2), "adam", ("bce", "none"), ("se", "sssdms"), 2.0, 0.0, 100.0),
    ((64, 2), "adamax", ("se", "sssdms"), ("bce", "equal"), 0.1, 0.7, 100.0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(ICNN_CASES)))
def test_icnn_joint_step_with_extra_penalty_matches_oracle(dev, case):
    """One inrfit_joint_step with the penalty on (ConvexNet h = 130, ConvexNextNet h = 64 L = 2; Adam / Adamax) against the oracle:
    loss_out, d loss / d seg, the prior's logits, the updated row and both moments; loss_out also against inrfit_joint_loss on
    [seg, sigmoid(prior_logits)].  Segmentation values at 0.5 and one ulp on either side: the indicator is strict."""
    import awesome_amd as A
    from awesome_amd import joint as J
    (h, nl), opt_kind, (kind, mode), (pkind, pmode), gamma, alpha, beta = ICNN_CASES[case]
    H, W, lr = 20, 23, 1e-3
    spec = A.IcnnSpec(n_hidden=h, in_features=2, n_layers=nl)
    g = torch.Generator().manual_seed(100 + case)
    p0 = {k: (torch.rand(shp, generator=g) - 0.45) * 0.3 for k, shp in spec.keys_shapes()}
    n = H * W
    seg = torch.rand(n, generator=g) * 0.9 + 0.05
    half = torch.tensor(0.5)
    seg[3], seg[4], seg[5] = half, torch.nextafter(half, torch.tensor(0.0)), torch.nextafter(half, torch.tensor(1.0))
    tgt = (torch.rand(n, generator=g) > 0.7).float()
    grid = O.positional_grid(W, H)[None]

    # ---- oracle: forward, AwesomeImageLoss with the penalty, autograd, one optimizer step, clamp
    pt = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    seg_t = seg.clone().requires_grad_(True)
    logits_ref = O.icnn_forward_image(pt, grid).reshape(-1)
    prior = torch.sigmoid(logits_ref)
    crit = O.weighted_loss(seg_t, tgt, kind=kind, mode=mode)
    pcrit = O.weighted_loss(prior, tgt, kind=pkind, mode=pmode)
    align = torch.mean((prior - (seg_t > 0.5).float()) ** 2)
    loss_ref = gamma * (crit + alpha * pcrit) + beta * align
    loss_ref.backward()
    p1 = {k: v.detach().clone() for k, v in p0.items()}
    st = O.AdamState(p1)
    (O.adam_step if opt_kind == "adam" else O.adamax_step)(p1, {k: pt[k].grad for k in p0}, st, lr)
    O.icnn_enforce_convexity(p1)

    # ---- the fused step
    desc = _desc(kind, mode, pkind, pmode, gamma, alpha, beta)
    row = A.pack_state_dict(spec, p0, dev).clone()
    P = spec.n_params
    opt = torch.zeros(2 * P + 8, device=dev)
    res = J.joint_step(spec, row, opt, A.Grid.from_image_grid(grid.to(dev)), seg.to(dev), tgt.to(dev), desc, step=1, lr=lr,
                       optimizer=opt_kind)
    lo = res.loss.cpu()
    assert int(res.status[0]) == 0
    np.testing.assert_allclose(lo[0].item(), loss_ref.item(), rtol=2e-5)
    np.testing.assert_allclose(lo[1].item(), crit.item(), rtol=2e-5)
    np.testing.assert_allclose(lo[2].item(), align.item(), rtol=2e-5)
    assert lo[3].item() == 1.0
    lo_dev = _device_joint_loss(seg.to(dev), torch.sigmoid(res.prior_logits), tgt.to(dev), desc, dev).cpu()
    np.testing.assert_allclose(lo.numpy(), lo_dev.numpy(), rtol=2e-5)
    ds_ref = seg_t.grad.numpy()
    np.testing.assert_allclose(res.dseg.cpu().numpy(), ds_ref, rtol=5e-5, atol=1e-7 * float(np.abs(ds_ref).max()))
    np.testing.assert_allclose(res.prior_logits.cpu().numpy(), logits_ref.detach().numpy(), rtol=0, atol=5e-6)
    np.testing.assert_allclose(row.cpu().numpy(), A.pack_state_dict(spec, p1).numpy(), rtol=1e-3, atol=2e-5)
    for got, ref in ((opt[:P], st.m), (opt[P:2 * P], st.v)):
        ref = A.pack_state_dict(spec, ref).numpy()
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * float(np.abs(ref).max()))


# ---- JointTrainer: the fused penalty step against the autograd step -----------------------------------------------------------


class _SegStandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)

    def forward(self, image, *args, **kwargs):
        return self.conv(image)


def _setup(dev, prior_factory, S=48, n=2, seed=5):
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.model import WrapperModule
    from awesome_amd.prior_bank import PriorBank
    torch.manual_seed(seed)
    ds = SyntheticPriorDataset(n_images=n, size=S, kind="noisy_blob")
    items = [ds[i] for i in range(n)]
    seg = _SegStandIn()
    wrapper = WrapperModule(seg, prior_factory(), use_segmentation_output_inversion=True).to(dev)
    bank = PriorBank(lambda: prior_factory().to(dev), n_images=n, device=dev)
    for k in range(n):
        bank.row(k)
    return items, seg, wrapper, bank


def _init_flow_parts(model, bank):
    """Non-zero last layers (zero-initialised flows are the identity) and ActNorm marked initialised, on every row."""
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for i in range(len(bank)):
            with bank.manager(model, i):
                for name, p in model.named_parameters():
                    if ".net.2." in name or "out_linear" in name or "linear2" in name:
                        p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
        for b_name, b in model.named_buffers():
            if b_name.endswith("data_dep_init_done"):
                b.fill_(1.0)


def _run(dev, prior_factory, crit, fused, schedule, lr=2e-3, opt_type=torch.optim.Adam, perturb=None, S=48, n=2):
    """Joint steps from identical starting points; `schedule` [(steps, extra_penalty, lr factor applied first)].
    fused=True: JointTrainer(fused_extra_penalty=True); False: the autograd bridges.  -> (losses, backbone weight, rows, paths, trainer)"""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.prior_bank import _ordered_parameters
    items, seg, wrapper, bank = _setup(dev, prior_factory, S=S, n=n)
    if perturb is not None:
        perturb(wrapper.prior_module, bank)
    opt = opt_type(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=lr)
    trainer = JointTrainer(wrapper, bank, crit, opt, fused=fused, fused_extra_penalty=fused)
    feat = torch.zeros(1, 1, 1, 1, device=dev)
    losses, paths, s = [], [], 0
    for steps, penalty, lr_factor in schedule:
        crit.extra_penalty = penalty
        for group in opt.param_groups:
            group["lr"] *= lr_factor
        for _ in range(steps):
            i = s % len(items)
            (image, _, xy), target = items[i]
            loss, _ = trainer.perform_step(i, (image[None].to(dev), feat, xy[None].to(dev)), target[None].to(dev))
            losses.append(float(loss))
            paths.append(trainer._path)
            s += 1
    return losses, seg.conv.weight.detach().cpu().clone(), bank.params.detach().cpu().clone(), paths, trainer


def _pcn_factory(h=64, flows=4, hidden=16):
    from awesome_amd.model import real_nvp_path_connected_net
    return lambda: real_nvp_path_connected_net(channels=2, hidden_units=hidden, flow_n_flows=flows, flow_output_fn="tanh",
                                               convex_net_hidden_units=h, convex_net_hidden_layers=2)


def _cdn_factory():
    from awesome_amd.model import ConvexDiffeomorphismNet
    return lambda: ConvexDiffeomorphismNet(n_hidden=64, n_hidden_layers=2, nf_layers=4, nf_hidden=24, diffeo_args=dict(backbone="normal_block"))


def _penalty_loss(**kw):
    from awesome_amd.measures import AwesomeImageLoss
    c = AwesomeImageLoss(**kw)
    c.extra_penalty = True
    return c


def _assert_same(a, b):
    lf, wf, rf = a[:3]
    la, wa, ra = b[:3]
    np.testing.assert_allclose(lf, la, rtol=2e-5)
    np.testing.assert_allclose(wf.numpy(), wa.numpy(), rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(rf.numpy(), ra.numpy(), rtol=1e-3, atol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["pcn", "cdn"])
def test_path_connected_joint_step_with_extra_penalty(dev, family):
    """inrfit_pcn_joint_step / inrfit_cdn_joint_step with the penalty on, 4 steps, against the autograd bridges."""
    from awesome_amd.measures import SE, UnariesWeightedLoss
    factory = _pcn_factory() if family == "pcn" else _cdn_factory()
    for crit in (lambda: _penalty_loss(alpha=0.7, gamma=0.1, beta=100.0),
                 lambda: _penalty_loss(criterion=UnariesWeightedLoss(SE("mean"), mode="sssdms"),
                                       prior_criterion=UnariesWeightedLoss(torch.nn.BCELoss(), mode="equal"), alpha=1.3, gamma=0.3, beta=100.0)):
        f = _run(dev, factory, crit(), True, [(4, True, 1.0)], perturb=_init_flow_parts)
        a = _run(dev, factory, crit(), False, [(4, True, 1.0)], perturb=_init_flow_parts)
        assert f[3] == ["fused"] * 4 and a[3] == ["autograd"] * 4
        assert int(f[4].last_status[0]) == 0
        _assert_same(f, a)
        assert not np.allclose(f[2].numpy(), _setup(dev, factory)[3].params.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("opt_type", [torch.optim.Adam, torch.optim.Adamax])
def test_extra_penalty_hook_in_mid_run_stays_fused(dev, opt_type):
    """The runner's hook in mid-run: 5 steps without the penalty, then the penalty on and the lr halved, 3 more steps.  With
    fused_extra_penalty every step takes the fused path; rows and backbone weights match a pure autograd run."""
    from awesome_amd.model import ConvexNextNet
    factory = lambda: ConvexNextNet(n_hidden=64, in_features=2, n_hidden_layers=2)   # noqa: E731
    schedule = [(5, False, 1.0), (3, True, 0.5)]
    f = _run(dev, factory, _penalty_loss(alpha=0.7), True, schedule, opt_type=opt_type)
    a = _run(dev, factory, _penalty_loss(alpha=0.7), False, schedule, opt_type=opt_type)
    assert f[3] == ["fused"] * 8 and a[3] == ["autograd"] * 8
    _assert_same(f, a)


@pytest.mark.gpu
def test_default_trainer_keeps_the_autograd_step_for_the_penalty(dev):
    """fused_extra_penalty defaults to False: the penalty steps keep taking the autograd path."""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ConvexNextNet
    from awesome_amd.prior_bank import _ordered_parameters
    items, seg, wrapper, bank = _setup(dev, lambda: ConvexNextNet(n_hidden=64, in_features=2, n_hidden_layers=2))
    crit = _penalty_loss(alpha=0.7)
    tr = JointTrainer(wrapper, bank, crit, torch.optim.Adam(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3))
    assert tr.fused and not tr.fused_extra_penalty
    (image, _, xy), target = items[0]
    tr.perform_step(0, (image[None].to(dev), torch.zeros(1, 1, 1, 1, device=dev), xy[None].to(dev)), target[None].to(dev))
    assert tr._path == "autograd"


@pytest.mark.gpu
def test_nonfinite_segmentation_with_extra_penalty_freezes_the_row(dev):
    """A NaN in the segmentation output once the penalty is on: status 1, row and moments untouched, raise_if_failed raises."""
    import awesome_amd as A
    from awesome_amd import joint as J
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ConvexNextNet
    from awesome_amd.prior_bank import _ordered_parameters
    torch.manual_seed(0)
    m = ConvexNextNet(n_hidden=64, in_features=2, n_hidden_layers=2)
    row = m.flat_parameters().to(dev)
    keep, S = row.clone(), 32
    grid = A.Grid.linspace(S, S, dev)
    seg = torch.rand(S * S, device=dev) * 0.9 + 0.05
    tgt = (torch.rand(S * S, device=dev) > 0.5).float()
    desc = _desc("bce", "none", "bce", "none", 0.1, 0.7, 100.0)
    opt = torch.zeros(2 * m.spec.n_params + 8, device=dev)
    good = J.joint_step(m.spec, row, opt, grid, seg, tgt, desc, step=1, lr=1e-3)
    assert int(good.status[0]) == 0 and not torch.equal(row, keep) and torch.isfinite(good.loss).all()
    row2, opt2 = keep.clone(), torch.zeros_like(opt)
    seg[11] = float("nan")
    bad = J.joint_step(m.spec, row2, opt2, grid, seg, tgt, desc, step=1, lr=1e-3)
    assert int(bad.status[0]) == 1 and torch.equal(row2, keep) and float(opt2[: 2 * m.spec.n_params].abs().sum()) == 0.0

    class NanSeg(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)

        def forward(self, image, *a, **k):
            out = self.conv(image)
            return out + torch.where(torch.arange(out.numel(), device=out.device).view_as(out) == 5, float("nan"), 0.0)

    items, _, wrapper, bank = _setup(dev, lambda: ConvexNextNet(n_hidden=64, in_features=2, n_hidden_layers=2), S=32)
    wrapper.segmentation_module = NanSeg().to(dev)
    opt_t = torch.optim.Adam(list(wrapper.segmentation_module.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-2)
    tr = JointTrainer(wrapper, bank, _penalty_loss(alpha=0.7), opt_t, fused=True, fused_extra_penalty=True)
    before = bank.params.detach().clone()
    (image, _, xy), target = items[0]
    tr.perform_step(0, (image[None].to(dev), torch.zeros(1, 1, 1, 1, device=dev), xy[None].to(dev)), target[None].to(dev))
    assert tr._path == "fused" and int(tr.last_status[0]) == 1 and torch.equal(bank.params, before)
    with pytest.raises(ValueError, match="Loss is nan or inf!"):
        tr.raise_if_failed()


@pytest.mark.gpu
def test_fused_penalty_steps_are_deterministic(dev):
    """Two identical 10-step fused-penalty runs (64x64, ConvexNextNet h = 130 L = 2): bit-equal rows, moments and losses."""
    import awesome_amd as A
    from awesome_amd import joint as J
    spec = A.IcnnSpec(n_hidden=130, in_features=2, n_layers=2)
    g = torch.Generator().manual_seed(9)
    p0 = {k: (torch.rand(shp, generator=g) - 0.45) * 0.3 for k, shp in spec.keys_shapes()}
    S = 64
    grid = A.Grid.linspace(S, S, dev)
    seg = (torch.rand(S * S, generator=g) * 0.9 + 0.05).to(dev)
    tgt = (torch.rand(S * S, generator=g) > 0.6).float().to(dev)
    desc = _desc("bce", "none", "se", "sssdms", 0.1, 0.7, 100.0)

    def run():
        row = A.pack_state_dict(spec, p0, dev).clone()
        opt = torch.zeros(2 * spec.n_params + 8, device=dev)
        losses = [J.joint_step(spec, row, opt, grid, seg, tgt, desc, step=t, lr=1e-3).loss.clone() for t in range(1, 11)]
        return row, opt, torch.stack(losses)

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("prior", ["c5_pcn", "convexnext_h130_l2"])
def test_fused_penalty_step_at_full_size(dev, prior):
    """One 256x256 step with the penalty on: the c5 path-connected prior (config/c5_refine_noisy256.yaml: 12 flows x 32, ICNN
    130 x 2, Adamax) and ConvexNextNet h = 130 L = 2 (Adam), fused against autograd."""
    from awesome_amd.model import ConvexNextNet
    if prior == "c5_pcn":
        factory, opt_type, perturb = _pcn_factory(h=130, flows=12, hidden=32), torch.optim.Adamax, _init_flow_parts
    else:
        factory, opt_type, perturb = (lambda: ConvexNextNet(n_hidden=130, in_features=2, n_hidden_layers=2)), torch.optim.Adam, None
    f = _run(dev, factory, _penalty_loss(alpha=1.0), True, [(1, True, 1.0)], lr=1e-3, opt_type=opt_type, perturb=perturb, S=256, n=1)
    a = _run(dev, factory, _penalty_loss(alpha=1.0), False, [(1, True, 1.0)], lr=1e-3, opt_type=opt_type, perturb=perturb, S=256, n=1)
    assert f[3] == ["fused"] and a[3] == ["autograd"]
    _assert_same(f, a)


@pytest.mark.gpu
def test_run_py_with_the_fused_extra_penalty(tmp_path):
    """scripts/run.py on c5_refine_noisy256.yaml at the reduced size of tests/test_gpu_host.py, the hook at epoch 1 and
    agent_args.fused_extra_penalty: every joint step takes the fused path."""
    override = {"dataset_args": {"n_images": 2, "size": 64},
                "agent_args": {"joint_epochs": 3, "fused_extra_penalty": True, "pretrain_args": {"num_epochs": 80}},
                "loss_type": "awesome_amd.measures.AwesomeImageLoss", "loss_args": {"alpha": 1.0},
                "use_extra_penalty_hook": True, "extra_penalty_after_n_epochs": 1, "use_reduce_lr_in_extra_penalty_hook": True}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--config-path",
                          os.path.join(ROOT, "config", "c5_refine_noisy256.yaml"), "--output-folder", str(tmp_path),
                          "--override", json.dumps(override)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    summary = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert summary["extra_penalty"] is True and summary["joint_epochs"] == 3
    assert all(np.isfinite(v) for v in summary["joint_loss_first_last"])
    assert summary["joint_steps_fused"] == 3 * summary["images"]


def test_joint_trainer_fused_extra_penalty_argument():
    """CPU: the opt-in keyword, off by default; no fused plan without a device (both paths then autograd)."""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.measures import AwesomeImageLoss
    from awesome_amd.model import ConvexNextNet, WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    factory = lambda: ConvexNextNet(n_hidden=8, in_features=2, n_hidden_layers=1)   # noqa: E731
    wrapper = WrapperModule(_SegStandIn(), factory())
    bank = PriorBank(factory, n_images=1, device="cpu")
    opt = torch.optim.Adam(list(wrapper.segmentation_module.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    assert JointTrainer(wrapper, bank, AwesomeImageLoss(), opt).fused_extra_penalty is False
    tr = JointTrainer(wrapper, bank, AwesomeImageLoss(), opt, fused_extra_penalty=True)
    assert tr.fused_extra_penalty is True and tr._fused_plan is None and not tr.fused
