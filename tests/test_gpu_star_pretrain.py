"""The star-shape prior behind the reference's plugin surface on the GPU: WrapperModule.pretrain with a StarShapedNet prior over synthetic
`kind: star` images (one batched device call, the reuse_state chain, gate + retry, Adamax with the plateau schedule), one joint step of
JointTrainer over a PriorBank of StarShapedNet rows (the autograd route), and config/c8_star64.yaml through scripts/run.py."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, HID = 33, 29, 33


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _Agent:
    """What a prior module's pretrain touches of TorchAgent: training_dataset (+ device, logger)."""

    def __init__(self, ds, dev):
        self.training_dataset, self.device, self.logger = ds, dev, None


def _star_items(n, seed0, prior_args):
    """SyntheticPriorDataset's items at 33 x 29: the `star` kind cut to a non-square window (the dataset itself is square)."""
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.model import StarShapedNet
    ds = SyntheticPriorDataset(n_images=n, size=H, kind="star", seed0=seed0, prior_model_type=StarShapedNet, prior_model_args=prior_args)
    ds._inner.unaries = lambda i, orig=ds._inner.unaries: orig(i)[:, :W].contiguous()
    ds._inner.ground_truth = lambda i, un=ds._inner.unaries: (un(i) > 0.5).float()
    ds._xy = ds._xy[:, :, :W].contiguous()
    return ds


def _setup(dev, n=3, seed0=0, seed=7):
    from awesome_amd.model import ForwardModule, StarShapedNet, WrapperModule
    torch.manual_seed(seed)
    args = dict(n_hidden=HID)
    ds = _star_items(n, seed0, args)
    wrapper = WrapperModule(ForwardModule(), StarShapedNet(**args), use_segmentation_output_inversion=True).to(dev)
    return ds, wrapper, _Agent(ds, dev)


def _item(ds, i, dev):
    """(generated prior state, unaries as the wrapper derives them, coordinate rows) of item i."""
    (_, state), ((image, _, xy), _) = ds[i]
    return state, (1 - torch.sigmoid(image.to(dev))).reshape(-1), xy.reshape(2, -1).t().contiguous().to(dev)


def _flat(state):
    from awesome_amd import star as S
    return S.flatten_state_dict(S.StarSpec(HID), state, "cpu")


def test_pretrain_is_one_batched_call_equal_to_the_direct_fit(dev):
    from awesome_amd import star as S
    from awesome_amd.model import StarShapedNet
    from awesome_amd.model.star_net import foreground_mean
    calls = []
    real = S.star_fit_dense
    ds, wrapper, agent = _setup(dev)
    try:
        S.star_fit_dense = lambda *a, **k: (calls.append(tuple(a[1].shape)), real(*a, **k))[1]
        state = wrapper.pretrain(train_set=ds, test_set=None, device=dev, agent=agent, use_progress_bar=False, num_epochs=120,
                                 reuse_state=False, proper_prior_fit_threshold=0.0)    # (this test is about the call, not the gate)
    finally:
        S.star_fit_dense = real
    assert len(calls) == 1 and calls[0][0] == 3                        # ONE device call for the three images
    assert sorted(state["cache"]) == ["0", "1", "2"] and state["model_type"].endswith("StarShapedNet")
    for k in range(3):
        assert list(state["cache"][str(k)].keys()) == list(StarShapedNet(HID).state_dict().keys()) == list(S.PARAM_ORDER)
    rep = wrapper.prior_module.pretrain_report
    assert all(not r["skipped"] and r["status"] == 0 for r in rep), rep
    # by hand from the same initial states and centres: the defaults are Adam 1e-2, SE / none, no plateau, the centre on the
    # foreground's mean and free after num_epochs // 10 epochs (first step at the next one)
    ds2 = _setup(dev)[0]
    items = [_item(ds2, i, dev) for i in range(3)]
    init = torch.stack([_flat(st) for st, _, _ in items]).to(dev)
    for i, (_, un, rows) in enumerate(items):
        init[i, 0:2] = -foreground_mean(rows.t().contiguous(), un)
    un = torch.stack([u for _, u, _ in items])
    centre0 = init[0, :2].clone()                                      # (the fit updates `init` in place)
    direct = S.star_fit_dense(S.StarSpec(HID), init, items[0][2], un, 120, lr=1e-2, offset_first_step=13, gate_logits=True)
    for i in range(3):
        assert torch.equal(_flat(state["cache"][str(i)]), direct.params[i].cpu()), i
    assert not torch.equal(direct.params[0, :2], centre0)           # ... and the centre was freed inside the 120 epochs


def test_pretrain_reuse_state_chain_shifts_the_centre_with_the_foreground(dev):
    from awesome_amd import star as S
    from awesome_amd.model.star_net import foreground_mean
    ds, wrapper, agent = _setup(dev, n=2)
    state = wrapper.pretrain(train_set=ds, test_set=None, device=dev, agent=agent, use_progress_bar=False, num_epochs=300,
                             reuse_state=True, reuse_state_epochs=40, proper_prior_fit_threshold=0.3)
    rep = wrapper.prior_module.pretrain_report
    # (the reference loop on the CPU reaches IoU 0.76 on frame 0 after these 300 epochs: the chain is not broken by a retry)
    assert [r["retries"] for r in rep] == [0, 0] and all(r["iou"] >= 0.3 for r in rep), rep
    ds2 = _setup(dev, n=2)[0]
    (_, un0, rows), (_, un1, _) = _item(ds2, 0, dev), _item(ds2, 1, dev)
    start = _flat(state["cache"]["0"]).to(dev)
    m0, m1 = foreground_mean(rows.t().contiguous(), un0), foreground_mean(rows.t().contiguous(), un1)
    assert float((m1 - m0).abs().max()) > 1e-3                        # the two stars sit at different places
    start[0:2] -= (m1 - m0)
    direct = S.star_fit_dense(S.StarSpec(HID), start[None].clone(), rows, un1[None], 40, lr=1e-2, offset_first_step=0, gate_logits=True)
    assert torch.equal(_flat(state["cache"]["1"]), direct.params[0].cpu())      # frame 1's fit, shifted, trained reuse_state_epochs


def test_pretrain_retry_takes_the_second_attempt(dev):
    from awesome_amd import star as S
    from awesome_amd.model.star_net import foreground_mean
    ds, wrapper, agent = _setup(dev, n=1)
    first = {k: v.clone() for k, v in ds[0][0][1].items()}
    state = wrapper.pretrain(train_set=ds, test_set=None, device=dev, agent=agent, use_progress_bar=False, num_epochs=30,
                             reuse_state=False, proper_prior_fit_threshold=0.999, proper_prior_fit_retrys=1)
    rep = wrapper.prior_module.pretrain_report
    assert rep[0]["retries"] == 1
    # the state comes from the second attempt: fresh parameters (the cache's key seed is unset: the global generator), the centre
    # re-initialised on the foreground mean - not the first attempt's fit
    ds2 = _setup(dev, n=1)[0]
    _, un, rows = _item(ds2, 0, dev)
    init = _flat(first).to(dev)
    init[0:2] = -foreground_mean(rows.t().contiguous(), un)
    attempt1 = S.star_fit_dense(S.StarSpec(HID), init[None].clone(), rows, un[None], 30, lr=1e-2, offset_first_step=4, gate_logits=True)
    got = _flat(state["cache"]["0"])
    assert not torch.equal(got, attempt1.params[0].cpu())
    assert bool(torch.isfinite(got).all()) and float(got[S.StarSpec(HID).n_params - HID - 1:-1].min()) >= 0.0     # W2_r.weight


def test_pretrain_with_adamax_and_the_plateau_schedule(dev):
    ds, wrapper, agent = _setup(dev, n=1)
    adam = wrapper.pretrain(train_set=ds, test_set=None, device=dev, agent=agent, use_progress_bar=False, num_epochs=60, reuse_state=False)
    ds2, wrapper2, agent2 = _setup(dev, n=1)
    other = wrapper2.pretrain(train_set=ds2, test_set=None, device=dev, agent=agent2, use_progress_bar=False, num_epochs=60,
                              reuse_state=False, optimizer="adamax", use_plateau=True)
    assert wrapper2.prior_module.pretrain_report[0]["status"] == 0
    a, b = _flat(adam["cache"]["0"]), _flat(other["cache"]["0"])
    assert bool(torch.isfinite(b).all()) and not torch.equal(a, b)


class _SegStandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)

    def forward(self, image, *args, **kwargs):
        return self.conv(image)


def test_joint_step_takes_the_autograd_route(dev):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.measures import FBMSJointLoss
    from awesome_amd.model import StarShapedNet, WrapperModule
    from awesome_amd.prior_bank import PriorBank
    torch.manual_seed(11)
    ds = _star_items(2, 3, dict(n_hidden=HID))
    seg = _SegStandIn()
    wrapper = WrapperModule(seg, StarShapedNet(HID), use_segmentation_output_inversion=True).to(dev)
    bank = PriorBank(lambda: StarShapedNet(HID).to(dev), n_images=2, device=dev)
    assert bank.P == HID * HID + 8 * HID + 4
    row0 = bank.row(1).detach().clone()
    crit = FBMSJointLoss(alpha=1.0, beta=2.0)
    opt = torch.optim.Adam(list(seg.parameters()) + list(wrapper.prior_module.parameters()), lr=1e-2)
    trainer = JointTrainer(wrapper, bank, crit, opt)
    assert trainer._fused_plan is None and trainer.fused is False
    with pytest.raises(ValueError):
        JointTrainer(wrapper, bank, crit, opt, fused=True)
    _, ((image, _, xy), target) = ds[1]
    inputs = (image[None].to(dev), torch.zeros(1, 1, 1, 1, device=dev), xy[None].to(dev))
    # the same step by hand on copies
    seg2 = copy.deepcopy(seg)
    prior2 = StarShapedNet(HID).to(dev)
    from awesome_amd import star as S
    prior2.load_state_dict({k: v.to(dev) for k, v in S.unflatten(S.StarSpec(HID), row0).items()})
    wrapper2 = WrapperModule(seg2, prior2, use_segmentation_output_inversion=True).to(dev)
    opt2 = torch.optim.Adam(list(seg2.parameters()) + list(prior2.parameters()), lr=1e-2)
    loss2 = crit(wrapper2(*inputs), target[None].to(dev))
    opt2.zero_grad()
    loss2.backward()
    opt2.step()
    wrapper2.enforce_convexity()
    loss, out = trainer.perform_step(1, inputs, target[None].to(dev))
    assert trainer._path == "autograd" and out.shape == (1, 2, H, W)
    assert float(loss) == pytest.approx(float(loss2.detach()), rel=1e-6)
    want = torch.cat([p.detach().reshape(-1) for p in prior2.parameters()])
    np.testing.assert_allclose(bank.row(1).cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-7)
    assert not torch.equal(bank.row(1), row0) and torch.equal(bank.row(1)[:2], row0[:2])    # (the module's centre is not trainable)
    np.testing.assert_allclose(seg.conv.weight.detach().cpu().numpy(), seg2.conv.weight.detach().cpu().numpy(), rtol=1e-5, atol=1e-7)


def test_config_c8_star64_runs_through_the_entry_point(dev, tmp_path):
    """scripts/run.py --config-path config/c8_star64.yaml: four 64 x 64 stars, every one past the gate (IoU of each saved prior
    against its image's unaries >= proper_prior_fit_threshold = 0.5)."""
    from awesome_amd import star as S
    from awesome_amd.dataset import SyntheticUnariesDataset
    from oracle import inr_oracle as O
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--config-path", os.path.join(ROOT, "config", "c8_star64.yaml"),
                          "--output-folder", str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    summary = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
    assert summary["images"] == 4 and summary["priors_saved"] == 4 and summary["epochs"] == 600
    assert all(r <= 1 for r in summary["retries"])
    saved = torch.load(os.path.join(summary["output"], "pretrain_state.pth"), map_location="cpu", weights_only=False)
    assert saved["model_type"].endswith("StarShapedNet")
    ds = SyntheticUnariesDataset(n_images=4, size=64, kind="star")
    xs = torch.linspace(0, 1, 64)
    rows = torch.stack([xs[None, :].expand(64, 64).reshape(-1), xs[:, None].expand(64, 64).reshape(-1)], 1).contiguous().to(dev)
    spec = S.StarSpec(130)
    for k in range(4):
        flat = S.flatten_state_dict(spec, saved["cache"][str(k)], dev)
        logits = S.star_forward(spec, flat, rows).cpu()
        iou = O.miou_binary((torch.sigmoid(logits) > 0.5).float(), (ds.unaries(k).reshape(-1) > 0.5).float(), invert=True)
        assert iou >= 0.5, (k, iou)
