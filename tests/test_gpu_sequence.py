"""Sequence pretraining with its epochs in one device call (inrfit_pcn_fit_sequence, inrfit_rnvp_fit_identity_sequence) and the
reference's own pre-fit stages (pretrain_args reference_prefits / sequence_device_loop).

The device call enqueues, per batch, the launches of the per-batch host loop - the same kernels with the same launch shapes on the
same numbers in the same order - and its epoch end adds the batch losses the way the host loop does, so device loop and host loop
are compared for EQUAL BITS (a derived bar).  Against the oracle the bars are the project's own for these comparisons
(tests/test_gpu_rnvp.py::test_fit_sequence_minibatches, ::test_learn_flow_identity): losses rtol 5e-4, parameters rtol 5e-3, atol 3e-4."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import inr_oracle as O
from tests import sequence_cases as Q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_RTOL, PARAM_RTOL, PARAM_ATOL = 5e-4, 5e-3, 3e-4


@pytest.fixture(scope="module")
def dev():
    import awesome_amd._lib as L
    L.load()
    return torch.device("cuda:0")


def _same_state(a, b):
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


def _close_to_oracle(module, ref):
    got = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    for k in ref:
        np.testing.assert_allclose(got[k].numpy(), ref[k].numpy(), rtol=PARAM_RTOL, atol=PARAM_ATOL, err_msg=k)


def _orders(kind, epochs, T):
    return Q.identity_orders(epochs, T) if kind == "identity" else Q.shuffled_orders(epochs, T, seed=5)


# ---- 1. the same bits as the host loop ---------------------------------------------------------------------------------------------
DROPS = dict(patience=0, factor=0.3, threshold=0.5)   # no epoch improves by 50 %: the learning rate drops behind every epoch but the first


def _final_lr(losses, lr, plateau):
    """The learning rate torch's scheduler arrives at on these epoch losses (the oracle's restatement of ReduceLROnPlateau)."""
    sched = O.PlateauState(lr, **plateau)
    for el in losses:
        lr = sched.step(el)
    return lr


@pytest.mark.parametrize("plateau", [DROPS, dict(patience=0, factor=0.5), None], ids=["drops", "patience0", "default_plateau"])
@pytest.mark.parametrize("order", ["identity", "shuffled"])
@pytest.mark.parametrize("batch", [2, 1, "T"])
@pytest.mark.parametrize("shape,icnn", [("t5_7x9", "h130_l1"), ("t4_8x10", "h32_l2"), ("t5_7x9", "h32_l2")])
def test_device_loop_equals_host_loop_bit_for_bit(dev, shape, icnn, batch, order, plateau):
    T = Q.SHAPES[shape][0]
    bs = T if batch == "T" else batch
    _, _, coords, uns = Q.frames(shape)
    coords, uns = coords.to(dev), uns.to(dev)
    o = _orders(order, 4, T)
    kw = dict(num_epochs=4, lr=2e-3, flow_weight_decay=1e-2, batch_size=bs, plateau=plateau, orders=o)
    host, start = Q.make_model(dev, icnn)
    device, _ = Q.make_model(dev, icnn)
    device.load_state_dict(start)
    l_host = host.fit_sequence(coords, uns, device_loop=False, **kw)
    l_dev = device.fit_sequence(coords, uns, device_loop=True, **kw)
    print("epoch losses host", l_host, "device", l_dev)
    assert len(l_dev) == 4 and all(np.isfinite(l_dev))
    assert l_dev == l_host
    _same_state(host, device)
    assert not torch.equal(host.state_dict()["convex_net.input.weight"], start["convex_net.input.weight"])
    if plateau is DROPS:
        # the rate did drop INSIDE the run, by the host loop's own losses: three times in four epochs, so the steps of epochs 2, 3 and 4
        # ran at three different reduced rates - taken from the header slot of the next step by the ICNN half and by the RealNVP half
        # of the update, rounded to fp32 where the host loop rounds.  A wrong slot, half or rounding parts the two runs above.
        assert _final_lr(l_host[:1], 2e-3, DROPS) == 2e-3
        assert [_final_lr(l_host[:n], 2e-3, DROPS) for n in (2, 3, 4)] == [2e-3 * 0.3, 2e-3 * 0.3 * 0.3, 2e-3 * 0.3 * 0.3 * 0.3]
        same_rate = Q.make_model(dev, icnn)[0]
        l_flat = same_rate.fit_sequence(coords, uns, device_loop=False, **dict(kw, plateau=False))
        assert l_flat[:2] == l_host[:2] and l_flat[2:] != l_host[2:]   # (and the reduced rate changes the trajectory from epoch 3 on)


def test_learning_rate_drops_on_the_device(dev):
    """Patience 0 and a threshold no epoch meets (a 50 % improvement): the learning rate drops epoch after epoch, and the header's
    learning rate after the call is the one the Python scheduler arrives at in doubles - with a factor that is no float (0.3)."""
    from awesome_amd import rnvp as R
    _, _, coords, uns = Q.frames("t5_7x9")
    m, _ = Q.make_model(dev, "h130_l1")
    ispec, rspec, icnn, flow = m._ordered_params()
    ip, fp = m._flat(icnn).to(dev), m._flat(flow).to(dev)
    res = R.pcn_fit_sequence(ispec, rspec, ip, fp, coords.to(dev), uns.to(dev), Q.identity_orders(5, 5), 2, lr=1e-3,
                             plateau=dict(patience=0, factor=0.3, threshold=0.5))
    losses = [float(v) for v in res.epoch_loss.cpu()]
    sched, lr = O.PlateauState(1e-3, patience=0, factor=0.3, threshold=0.5), 1e-3
    for el in losses:
        lr = sched.step(el)
    hdr = res.icnn_opt_state[0, 2 * ispec.n_params:].cpu()
    assert lr < 1e-3 and float(hdr[2]) == float(np.float32(lr)), (lr, hdr)
    assert int(res.status[0]) == 0


# ---- 2. against the oracle (T = 5, batch 2: a last batch of one frame) ------------------------------------------------------------------
def test_device_loop_against_the_oracle(dev):
    rows, uns_rows, coords, uns = Q.frames("t5_7x9")
    m, start = Q.make_model(dev, "h130_l1")
    masks = O.rnvp_masks(Q.CH, Q.FLOWS)
    pf, ref_losses = O.fit_pcn_minibatch(Q.oracle_state(start), rows, uns_rows, 4, 2, masks, torch.zeros(3), torch.ones(3), lr=2e-3,
                                        flow_weight_decay=1e-2, plateau=DROPS)
    losses = m.fit_sequence(coords.to(dev), uns.to(dev), num_epochs=4, lr=2e-3, flow_weight_decay=1e-2, batch_size=2,
                            plateau=DROPS, device_loop=True)
    print("epoch losses", losses, "oracle", ref_losses)
    assert _final_lr(ref_losses[:3], 2e-3, DROPS) == 2e-3 * 0.3 * 0.3   # the oracle's last epoch ran at the twice reduced rate
    np.testing.assert_allclose(np.asarray(losses), np.asarray(ref_losses), rtol=LOSS_RTOL)
    _close_to_oracle(m, pf)


# ---- 3. the mini-batched identity pre-fit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["t5_7x9", "t4_8x10"])
def test_minibatch_identity_prefit(dev, shape):
    from awesome_amd.model.path_connected_net import PathConnectedNet
    T, H, W = Q.SHAPES[shape]
    x = PathConnectedNet.create_normalized_grid((T, H, W))
    o = Q.shuffled_orders(4, T, seed=9)
    host, start = Q.make_model(dev, "h32_l2", seed=31)
    device, _ = Q.make_model(dev, "h32_l2", seed=31)
    device.load_state_dict(start)
    kw = dict(lr=1e-2, weight_decay=1e-3, max_iter=4, batch_size=2, orders=o)
    h_host = host.learn_flow_identity(x.to(dev), device_loop=False, **kw)
    h_dev = device.learn_flow_identity(x.to(dev), device_loop=True, **kw)
    assert torch.equal(h_host, h_dev) and h_dev.shape == (4,)
    _same_state(host, device)
    frame_rows = [x[t].reshape(Q.CH, -1).t().contiguous() for t in range(T)]
    pf, ref_hist = Q.fit_flow_identity_minibatch(Q.oracle_state(start), frame_rows, o, 2, O.rnvp_masks(Q.CH, Q.FLOWS), torch.zeros(3),
                                                 torch.ones(3), lr=1e-2, weight_decay=1e-3)
    print("loss_hist", h_dev.tolist(), "oracle", ref_hist)
    np.testing.assert_allclose(h_dev.cpu().numpy(), np.asarray(ref_hist, np.float32), rtol=LOSS_RTOL)   # the LAST batch's loss of each epoch
    _close_to_oracle(device, pf)
    for k in ("linear.weight", "linear.bias"):
        assert torch.equal(device.state_dict()[k], start[k])


def test_identity_prefit_without_batch_size_is_the_full_batch_call(dev):
    """batch_size=None: the full-batch behaviour, bit for bit what inrfit_rnvp_fit_identity gives on the same grid."""
    import awesome_amd as A
    from awesome_amd import rnvp as R
    m, start = Q.make_model(dev, "h32_l2", seed=33)
    _, _, coords, _ = Q.frames("t5_7x9")
    grid = A.Grid.explicit(coords.permute(1, 0, 2).reshape(3, -1).contiguous().to(dev))
    _, rspec, _, flow = m._ordered_params()
    fp = m._flat(flow).to(dev)
    hist_direct, _ = R.fit_identity(rspec, fp, grid, steps=6, lr=1e-2, weight_decay=1e-5)
    hist = m.learn_flow_identity(grid, lr=1e-2, weight_decay=1e-5, max_iter=6)
    assert torch.equal(hist, hist_direct[0])
    _, _, _, flow = m._ordered_params()
    got = m._flat(flow).to(dev)
    lin = 2 * rspec.channels
    assert torch.equal(got[0, lin:], fp[0, lin:])


# ---- 4. pretrain() with the reference's pre-fit stages ---------------------------------------------------------------------------------
ARGS = dict(channels=3, hidden_units=32, flow_n_flows=6, flow_output_fn="tanh", convex_net_hidden_units=32, convex_net_hidden_layers=2)
PRE = dict(num_epochs=2, lr=1e-3, batch_size=2, prefit_flow_net_identity=True, prefit_flow_net_identity_num_epochs=3,
           prefit_convex_net=True, prefit_convex_net_num_epochs=8)
SIZE, FRAMES = 10, 5


class _Agent:
    def __init__(self, ds, dev):
        self.training_dataset, self.device, self.logger = ds, dev, None


def _pretrain(dev, seed, **extra):
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.model import ForwardModule, WrapperModule, real_nvp_path_connected_net
    ds = SyntheticPriorDataset(n_images=FRAMES, size=SIZE, kind="sequence")
    torch.manual_seed(seed)
    model = real_nvp_path_connected_net(**ARGS)
    with torch.no_grad():   # couplings away from the zero initialisation, so that every parameter has a gradient from step one
        for k, p in model.named_parameters():
            if k.endswith("net.2.weight") or k.endswith("net.2.bias"):
                p.copy_(0.1 * torch.randn_like(p))
        # ActNorm marked initialised (s = t = 0), as tests/test_gpu_rnvp.py::test_fit_sequence_minibatches does.  Behind the data-dependent
        # init the first Adamax steps of the ActNorm offsets are lr * sign(gradient) on gradients at rounding level: the oracle in fp32
        # is then 4 - 11 bars away from the same oracle in float64 (flows.11.t, measured on the CPU for seeds 17, 19, 23), against
        # 1e-3 of a bar with the init out of the way.  Which batch the init sees is pinned on its own below, bit for bit.
        for a in model.flow_net.net.network.flows:
            if hasattr(a, "data_dep_init_done"):
                a.data_dep_init_done.fill_(1.0)
    model = model.to(dev)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    wrapper = WrapperModule(ForwardModule(), model, use_segmentation_output_inversion=True).to(dev)
    torch.manual_seed(seed + 1)   # the loaders' shuffles
    state = wrapper.pretrain(train_set=ds, test_set=None, device=dev, agent=_Agent(ds, dev), use_progress_bar=False, **dict(PRE, **extra))
    return ds, model, start, state


def test_pretrain_reference_prefits_against_the_oracle(dev):
    """The orchestration - identity pre-fit on the normalized (T, H, W) grid in shuffled mini-batches, convex pre-fit on frames 0 and
    T - 1, the mini-batch epochs - against the oracle's parts in that order: the flow behind the identity pre-fit, the convex net behind
    the convex pre-fit (pretrain() stopped there: the later stages switched off, no epochs), then the final state and the epoch losses."""
    from awesome_amd.model.path_connected_net import PathConnectedNet
    ds, on, start, state = _pretrain(dev, 17, reference_prefits=True, sequence_device_loop=True)
    _, off, start_off, _ = _pretrain(dev, 17, reference_prefits=True, sequence_device_loop=False)
    assert all(torch.equal(v, start_off[k]) for k, v in start.items())
    assert on.pretrain_epoch_losses == off.pretrain_epoch_losses and len(on.pretrain_epoch_losses) == 2
    _same_state(on, off)
    assert list(state.keys()) == list(start.keys())
    # the oracle's parts, in the reference's order
    masks, lo, hi = O.rnvp_masks(3, 6), torch.zeros(3), torch.ones(3)
    x = PathConnectedNet.create_normalized_grid((FRAMES, SIZE, SIZE))
    torch.manual_seed(18)
    o = Q.dataloader_orders(FRAMES, 2, 3, one_loader=True)
    sd, _ = Q.fit_flow_identity_minibatch(Q.oracle_state(start), [x[t].reshape(3, -1).t().contiguous() for t in range(FRAMES)], o, 2, masks,
                                          lo, hi, lr=1e-2, weight_decay=1e-5)
    ref = dict(reference_prefits=True, sequence_device_loop=True, num_epochs=0)
    _, after_identity, _, _ = _pretrain(dev, 17, prefit_convex_net=False, **ref)
    assert after_identity.pretrain_epoch_losses == []
    _close_to_oracle(after_identity, sd)                                       # the flow moved, nothing else did
    for k, v in after_identity.state_dict().items():
        assert k.startswith("flow_net.") or torch.equal(v, start[k]), k
    assert not torch.equal(after_identity.state_dict()["flow_net.net.network.flows.0.s.net.2.weight"],
                           start["flow_net.net.network.flows.0.s.net.2.weight"])
    rows = [ds[i][0][2].reshape(3, -1).t().contiguous() for i in range(FRAMES)]
    uns = [(1 - torch.sigmoid(ds[i][0][0])).reshape(-1, 1) for i in range(FRAMES)]
    ends = torch.cat([rows[0], rows[-1]], 0)
    with torch.no_grad():
        xd = O.pcn_deformation(sd, ends, masks, lo, hi)
    icnn = {k[len("convex_net."):]: v for k, v in sd.items() if k.startswith("convex_net.")}
    icnn, _, _ = O.fit_icnn(icnn, xd.t().reshape(1, 3, 1, -1), torch.cat([uns[0], uns[-1]], 0).reshape(1, 1, 1, -1), 8, lr=1e-3,
                            loss_kind="se", optimizer="adam")
    sd.update({"convex_net." + k: v for k, v in icnn.items()})
    _, after_convex, _, _ = _pretrain(dev, 17, **ref)
    _close_to_oracle(after_convex, sd)                                         # the convex net on frames 0 and T - 1 of the deformed grid
    for k, v in after_convex.state_dict().items():
        assert k.startswith("convex_net.") or torch.equal(v, after_identity.state_dict()[k]), k
    assert not torch.equal(after_convex.state_dict()["convex_net.input.weight"], start["convex_net.input.weight"])
    pf, ref_losses = O.fit_pcn_minibatch(sd, rows, uns, 2, 2, masks, lo, hi, lr=1e-3, flow_weight_decay=1e-5,
                                        plateau=dict(patience=200, factor=0.5))
    print("epoch losses", on.pretrain_epoch_losses, "oracle", ref_losses)
    np.testing.assert_allclose(np.asarray(on.pretrain_epoch_losses), np.asarray(ref_losses), rtol=LOSS_RTOL)
    _close_to_oracle(on, pf)


def test_pretrain_switches_off_is_the_parents_dispatch(dev):
    """Neither switch: pretrain() on the 5-frame sequence equals the stages called by hand on the whole grid, as before."""
    import awesome_amd as A
    from awesome_amd.model import real_nvp_path_connected_net
    ds, model, start, state = _pretrain(dev, 19)
    twin = real_nvp_path_connected_net(**ARGS).to(dev)
    twin.load_state_dict(start)
    frames = [(1 - torch.sigmoid(ds[i][0][0].to(dev))).reshape(-1) for i in range(FRAMES)]
    coords = torch.stack([ds[i][0][2].reshape(3, -1) for i in range(FRAMES)]).to(dev)
    whole = A.Grid.explicit(coords.permute(1, 0, 2).reshape(3, -1).contiguous())
    twin.learn_flow_identity(whole, lr=1e-2, weight_decay=1e-5, max_iter=3)
    twin.learn_convex_net(whole, torch.stack(frames).reshape(1, -1), lr=1e-3, weight_decay=0.0, max_iter=8)
    losses = twin.fit_sequence(coords, torch.stack(frames), num_epochs=2, lr=1e-3, flow_weight_decay=1e-5, batch_size=2)
    assert model.pretrain_epoch_losses == losses
    for k, v in twin.state_dict().items():
        if v.is_floating_point() and not k.endswith("data_dep_init_done"):
            assert torch.equal(v, state[k]), k


def test_zoo_key_holds_the_batch_size(dev):
    """A flow stored by the pre-fit with batch_size=2 is a miss for batch_size=1 and a hit for batch_size=2."""
    from awesome_amd.model import Zoo
    from awesome_amd.model.path_connected_net import PathConnectedNet
    x = PathConnectedNet.create_normalized_grid((4, 8, 10)).to(dev)
    zoo = Zoo(None)
    flows = []
    for bs in (2, 1, 2):
        m, _ = Q.make_model(dev, "h32_l2", seed=41)
        m.learn_flow_identity(x, lr=1e-2, max_iter=2, zoo=zoo, batch_size=bs, orders=Q.identity_orders(2, 4))
        flows.append(torch.cat([p.detach().reshape(-1) for p in m.flow_net.parameters()]))
    assert not torch.equal(flows[0], flows[1])   # fitted again with its own batches
    assert torch.equal(flows[0], flows[2])


def test_actnorm_init_sees_the_first_batch_drawn(dev):
    """With a learning rate of zero nothing but ActNorm's data-dependent init changes the flow: after fit_sequence / the mini-batched
    learn_flow_identity its s and t are those of `inrfit_rnvp_actnorm_init` on the first batch of the given order (frames 3 and 1),
    not on frames 0 and 1 - host loop and device loop alike."""
    import awesome_amd as A
    from awesome_amd import rnvp as R
    from awesome_amd.model.path_connected_net import PathConnectedNet
    _, _, coords, uns = Q.frames("t5_7x9")
    coords, uns = coords.to(dev), uns.to(dev)
    x = PathConnectedNet.create_normalized_grid(Q.SHAPES["t5_7x9"]).to(dev)
    o = torch.tensor([[3, 1, 0, 2, 4]])
    for device_loop in (False, True):
        for stage in ("sequence", "identity"):
            m, _ = Q.make_model(dev, "h32_l2", seed=51)
            for a in m.flow_net.net.network.flows:
                if hasattr(a, "data_dep_init_done"):
                    a.data_dep_init_done.fill_(0.0)
            _, rspec, _, flow = m._ordered_params()
            frames = coords if stage == "sequence" else x.reshape(5, 3, -1)
            want = m._flat(flow).to(dev)
            R.actnorm_init(rspec, want, A.Grid.explicit(frames[[3, 1]].permute(1, 0, 2).reshape(3, -1).contiguous()))
            other = m._flat(flow).to(dev)
            R.actnorm_init(rspec, other, A.Grid.explicit(frames[[0, 1]].permute(1, 0, 2).reshape(3, -1).contiguous()))
            assert not torch.equal(want, other)
            if stage == "sequence":
                m.fit_sequence(coords, uns, num_epochs=1, lr=0.0, batch_size=2, orders=o, device_loop=device_loop)
            else:
                m.learn_flow_identity(x, lr=0.0, max_iter=1, batch_size=2, orders=o, device_loop=device_loop)
            _, _, _, flow = m._ordered_params()
            assert torch.equal(m._flat(flow).to(dev), want), (stage, device_loop)


def test_drawn_orders_host_and_device_loop_agree(dev):
    """orders=None with dataloader_shuffle: both forms draw the same permutations from the generator and initialise an uninitialised
    ActNorm on frames 0 .. batch_size - 1, so the two switches give the same bits."""
    _, _, coords, uns = Q.frames("t5_7x9")
    coords, uns = coords.to(dev), uns.to(dev)
    out = []
    for device_loop in (False, True):
        m, _ = Q.make_model(dev, "h32_l2", seed=61)
        for a in m.flow_net.net.network.flows:
            if hasattr(a, "data_dep_init_done"):
                a.data_dep_init_done.fill_(0.0)
        losses = m.fit_sequence(coords, uns, num_epochs=3, lr=2e-3, batch_size=2, dataloader_shuffle=True,
                                generator=torch.Generator().manual_seed(7), device_loop=device_loop)
        out.append((losses, m))
    assert out[0][0] == out[1][0]
    _same_state(out[0][1], out[1][1])


def test_identity_sequence_continues_with_step0(dev):
    """Two calls of two epochs, the second with step0 = the steps taken and the first one's optimizer state, end where one call of
    four epochs ends (the identity pre-fit has no scheduler state to carry)."""
    from awesome_amd import rnvp as R
    from awesome_amd.model.path_connected_net import PathConnectedNet
    x = PathConnectedNet.create_normalized_grid(Q.SHAPES["t5_7x9"]).reshape(5, 3, -1).contiguous().to(dev)
    o = Q.shuffled_orders(4, 5, seed=11)
    m, _ = Q.make_model(dev, "h32_l2", seed=63)
    _, rspec, _, flow = m._ordered_params()
    whole, split = m._flat(flow).to(dev), m._flat(flow).to(dev)
    h_whole, _ = R.fit_identity_sequence(rspec, whole, x, o, 2, lr=1e-2)
    h1, opt = R.fit_identity_sequence(rspec, split, x, o[:2], 2, lr=1e-2)
    h2, _ = R.fit_identity_sequence(rspec, split, x, o[2:], 2, lr=1e-2, flow_opt_state=opt, step0=6)
    assert torch.equal(torch.cat([h1, h2]), h_whole) and torch.equal(split, whole)


# ---- 5. determinism and scratch -------------------------------------------------------------------------------------------------------
def test_device_loop_repeats_and_reads_no_stale_scratch(dev):
    """Twice the same bits; once more with every scratch allocation pre-filled with NaN (a step that read staging rows behind a
    short last batch, or a workspace byte nobody wrote, would show up as NaN or as other bits)."""
    import awesome_amd._lib as L
    _, _, coords, uns = Q.frames("t5_7x9")
    coords, uns = coords.to(dev), uns.to(dev)
    runs = []
    try:
        for poison in (False, False, True):
            L.POISON = poison
            m, _ = Q.make_model(dev, "h130_l1")
            losses = m.fit_sequence(coords, uns, num_epochs=3, lr=2e-3, batch_size=2, orders=Q.shuffled_orders(3, 5, seed=3), device_loop=True,
                                    plateau=dict(patience=0, factor=0.5))
            assert all(np.isfinite(losses))
            assert all(torch.isfinite(v).all() for v in m.state_dict().values() if v.is_floating_point())
            runs.append((losses, m))
    finally:
        L.POISON = False
    for losses, m in runs[1:]:
        assert losses == runs[0][0]
        _same_state(m, runs[0][1])


# ---- 6. a non-finite loss --------------------------------------------------------------------------------------------------------------
def test_nan_targets_freeze_the_network_and_raise(dev):
    """NaN targets in frame 3 (second batch of the first epoch): the network stays at the parameters in front of that step - one
    step on frames 0 and 1 - for the rest of the call, status is set, and fit_sequence raises the reference's error."""
    from awesome_amd import rnvp as R
    _, _, coords, uns = Q.frames("t5_7x9")
    coords, uns = coords.to(dev), uns.to(dev)
    bad = uns.clone()
    bad[3] = float("nan")
    one, start = Q.make_model(dev, "h130_l1")
    one.fit_sequence(coords[:2].contiguous(), uns[:2].contiguous(), num_epochs=1, lr=2e-3, batch_size=2)   # the step in front of the bad one
    m, _ = Q.make_model(dev, "h130_l1")
    with pytest.raises(ValueError, match="Loss is nan or inf!"):
        m.fit_sequence(coords, bad, num_epochs=2, lr=2e-3, batch_size=2, device_loop=True)
    _same_state(m, one)
    ispec, rspec, icnn, flow = one._ordered_params()
    fresh, _ = Q.make_model(dev, "h130_l1")
    _, _, icnn, flow = fresh._ordered_params()
    res = R.pcn_fit_sequence(ispec, rspec, fresh._flat(icnn).to(dev), fresh._flat(flow).to(dev), coords, bad, Q.identity_orders(2, 5), 2,
                             lr=2e-3, plateau=dict(patience=200, factor=0.5))
    assert int(res.status[0]) == 1 and not bool(torch.isfinite(res.epoch_loss).any())


# ---- 7. the runner ---------------------------------------------------------------------------------------------------------------------
def test_runner_takes_the_reference_config(tmp_path):
    override = {"dataset_args": {"size": 16, "frames": 5},
                "agent_args": {"pretrain_args": {"num_epochs": 6, "prefit_flow_net_identity_num_epochs": 3, "prefit_convex_net_num_epochs": 10}}}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--config-path",
                          os.path.join(ROOT, "config", "c4_sequence128x16_reference.yaml"), "--output-folder", str(tmp_path), "--override",
                          json.dumps(override)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    summary = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert summary["images"] == 1 and summary["priors_saved"] == 1 and summary["epochs"] == 6
    assert summary["sequence_device_loop"] is True
    losses = summary["epoch_losses"]
    assert len(losses) == 6 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
