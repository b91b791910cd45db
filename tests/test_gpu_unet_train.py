"""The UNet's training step in HIP (awesome_amd.unet.unet_train_forward, include/inrfit.h inrfit_unet_train_*, csrc/unet_train.h) against
float64: logits, every parameter's gradient and the updated running statistics of one training-mode forward and backward.

Yardstick, bar and the conditioning of the cases: tests/unet_train_cases.py (the same module's .double() copy on the CPU;
max|hip - f64| <= 4 e_torch + 1e-6 max|f64| per tensor; cases in which no ReLU input and no max-pool tie can change sides between
fp32 and float64).  Measured errors: profiles/unet_train_parity.md."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_train_cases as U   # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _collect(net, logits):
    bns = U.bn_layers(net)
    return dict(logits=logits.detach(), grads=[p.grad for p in net.parameters()], means=[bn.running_mean for bn in bns],
                vars=[bn.running_var for bn in bns])


def _step(case, dev, net=None, strip=None, poison=False):
    """One HIP training step of a copy of the case's module -> (run_torch-shaped result, the module)."""
    from awesome_amd.unet import unet_train_forward
    net = copy.deepcopy(case["net"]).to(dev).train() if net is None else net
    if poison:      # a NaN-filled fresh workspace: whatever the step reads, it has written before
        from awesome_amd import _lib as L
        net.__dict__.pop("_hip_unet_cache", None)
        old, L.POISON = L.POISON, True
    try:
        logits = unet_train_forward(net, case["image"].to(dev), case["feat"].to(dev), strip_points=case["strip"] if strip is None else strip)
        logits.backward(case["dlogits"].to(dev))
    finally:
        if poison:
            L.POISON = old
    return _collect(net, logits), net


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(U.CASES))
def test_parity_with_float64(dev, name):
    case = U.build(name)
    got, net = _step(case, dev)
    assert type(got["logits"]) is torch.Tensor and all(g is not None for g in got["grads"])
    U.compare(got, case, name)
    assert all(int(bn.num_batches_tracked) == 1 for bn in U.bn_layers(net))


@pytest.mark.gpu
def test_reference_fixture(dev, golden_dir):
    """The 37 x 50 width 4 step of the reference's own class (float64, tests/golden/unet_train.npz) as the yardstick; e_torch is our
    class's fp32 CPU pass from the fixture's state_dict against it."""
    from awesome_amd.model import UNet
    fx = np.load(os.path.join(golden_dir, "unet_train.npz"))
    net = UNet(in_chn=4, base_width=int(fx["base_width"]))
    net.load_state_dict({k[len("state/"):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("state/")})
    net.train()
    image, feat, dlogits = (torch.from_numpy(fx[k]) for k in ("image", "feat", "dlogits"))
    names = [str(n) for n in fx["param_names"]]
    assert names == [n for n, _ in net.named_parameters()]
    bn_names = [n for n, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    f64 = dict(logits=torch.from_numpy(fx["logits"]), grads=[torch.from_numpy(fx["grad/" + n]) for n in names],
               means=[torch.from_numpy(fx[f"after/{n}.running_mean"]) for n in bn_names],
               vars=[torch.from_numpy(fx[f"after/{n}.running_var"]) for n in bn_names])
    f32 = U.run_torch(net, image, feat, dlogits, torch.float32)
    z64 = U.run_torch(net, image, feat, dlogits, torch.float64, backward=False)["z"]
    assert U.offenders(f32["z"], z64) == (0, 0)
    case = dict(net=net, image=image, feat=feat, dlogits=dlogits, strip=0, f32=f32, f64=f64)
    U.compare(f32, case, "fp32 CPU torch against the reference fixture")
    got, _ = _step(case, dev)
    U.compare(got, case, "37x50 base 4 against the reference fixture")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["37x50-b8", "64x48-b64-onoff"])
def test_two_steps_give_the_same_bits(dev, name):
    case = U.build(name)
    a, _ = _step(case, dev)
    b, _ = _step(case, dev, poison=True)
    for (n, x, _), (_, y, _) in zip(U.tensors(a, case["net"]), U.tensors(b, case["net"])):
        assert not bool(torch.isnan(y).any()), n            # every element of grads is written
        assert torch.equal(x, y), n


@pytest.mark.gpu
def test_forward_takes_the_hip_route_in_training(dev):
    from awesome_amd.model import UNet
    from awesome_amd.unet import UNetTrainFunction
    case = U.build("37x50-b4")
    net = UNet(in_chn=4, base_width=4, hip_training=True)
    net.load_state_dict(case["net"].state_dict())
    assert "hip_training" not in "".join(net.state_dict())
    net = net.to(dev).train()
    image, feat, dlogits = case["image"].to(dev), case["feat"].to(dev), case["dlogits"].to(dev)
    assert net.hip_train_route(image, feat)
    logits = net(image, feat)
    assert logits.grad_fn is not None and type(logits.grad_fn).__name__ == UNetTrainFunction.__name__ + "Backward"
    logits.backward(dlogits)
    U.compare(_collect(net, logits), case, "UNet.forward with hip_training")
    assert all(int(bn.num_batches_tracked) == 1 for bn in U.bn_layers(net))
    # a single item is batcherized
    net.zero_grad()
    assert type(net(image[0], feat[0]).grad_fn).__name__ == UNetTrainFunction.__name__ + "Backward"


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["batch2", "inputs_require_grad", "momentum_none", "eval", "switch_off"])
def test_every_other_case_goes_to_the_torch_modules(dev, how):
    from awesome_amd.model import UNet
    case = U.build("37x50-b4")
    net = UNet(in_chn=4, base_width=4, hip_training=how != "switch_off")
    net.load_state_dict(case["net"].state_dict())
    net = net.to(dev).train()
    image, feat = case["image"].to(dev), case["feat"].to(dev)
    if how == "batch2":
        image, feat = torch.cat([image, image.flip(-1)]), torch.cat([feat, feat.flip(-1)])
    elif how == "inputs_require_grad":
        image = image.clone().requires_grad_(True)
    elif how == "momentum_none":
        for bn in U.bn_layers(net):
            bn.momentum = None
    elif how == "eval":
        net.eval()
    twin = copy.deepcopy(net)
    assert not net.hip_train_route(image, feat)
    if how == "eval":
        with torch.no_grad():
            assert net.hip_route(image, feat)                # the evaluation route still applies
            out = net(image, feat)
            ref = twin.forward_torch(image, feat)
        assert "packed" in net.__dict__["_hip_unet_cache"] and out.grad_fn is None and out.shape == ref.shape
        return
    out, ref = net(image, feat), twin.forward_torch(image, feat)
    assert "Conv" in type(out.grad_fn).__name__, type(out.grad_fn).__name__      # OutConv's own node: the torch modules ran
    assert torch.equal(out, ref)
    for (n, b), c in zip(net.named_buffers(), twin.buffers()):
        assert torch.equal(b, c), n
    out.sum().backward()
    assert all(p.grad is not None for p in net.parameters())
    if how == "inputs_require_grad":
        assert image.grad is not None


@pytest.mark.gpu
def test_three_adam_steps_track_the_torch_modules(dev):
    """Three Adam steps through the function against three Adam steps of the float64 CPU copy through forward_torch; e_torch: the
    same three steps in fp32 on the CPU.  The bar is applied to every parameter (and running statistic) after the third step."""
    from awesome_amd.model import UNet
    case = U.build("32x32-b4")
    image, feat, dlogits = case["image"], case["feat"], case["dlogits"]

    def three_steps(net, dtype, device, hip):
        net = net.to(dtype).to(device).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        im, fe, dl = (t.to(dtype).to(device) for t in (image, feat, dlogits))
        for _ in range(3):
            opt.zero_grad()
            out = net(im, fe) if hip else net.forward_torch(im, fe)
            out.backward(dl)
            opt.step()
        bns = U.bn_layers(net)
        return dict(logits=out.detach(), grads=[p.detach() for p in net.parameters()], means=[bn.running_mean for bn in bns],
                    vars=[bn.running_var for bn in bns]), net

    def fresh():
        net = UNet(in_chn=4, base_width=4, hip_training=True)
        net.load_state_dict(case["net"].state_dict())
        return net

    f64, _ = three_steps(fresh(), torch.float64, "cpu", False)
    f32, _ = three_steps(fresh(), torch.float32, "cpu", False)
    got, net = three_steps(fresh(), torch.float32, dev, True)
    assert all(int(bn.num_batches_tracked) == 3 for bn in U.bn_layers(net))
    # the parameters stand where compare() expects the gradients; a bias in front of a BatchNorm is an ordinary tensor here
    names = [n for n, _ in net.named_parameters()]
    for k, n in enumerate(["logits"] + names):
        x, r, t = ([d["logits"]] + d["grads"] for d in (got, f64, f32))
        e_torch, e = float((t[k].double() - r[k]).abs().max()), float((x[k].cpu().double() - r[k]).abs().max())
        bar = 4 * e_torch + 1e-6 * float(r[k].abs().max())
        print(f"[unet train adam] {n}: e {e:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}")
        assert e <= bar, f"{n}: e {e:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}"


@pytest.mark.gpu
def test_joint_step_with_the_hip_training_switch(dev):
    """One fused JointTrainer step on a c5-style item (PathConnectedNet prior, FBMSJointLoss, 32 x 32): the gradient the step leaves
    in the UNet's parameters with hip_training=True against the same step with the switch off (the torch modules on the GPU).
    Both trainers first take one step with the switch off and a learning rate of zero - the path-connected prior's data-dependent
    initialisation, which the trainer runs as an autograd step - so the compared step is the fused one (seg.backward(dseg)) from the
    same state.  The bar is the parity bar in relative form, e_torch / max|f64| per tensor taken from the case of the same network and
    shape, since this step's dseg has another scale than the case's dlogits; doubled, because both sides are fp32 passes."""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.measures import FBMSJointLoss
    from awesome_amd.model import UNet, WrapperModule, real_nvp_path_connected_net
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    case = U.build("32x32-b4")
    pargs = dict(channels=2, hidden_units=16, flow_n_flows=4, flow_output_fn="tanh", convex_net_hidden_units=64, convex_net_hidden_layers=2)
    factory = lambda: real_nvp_path_connected_net(**pargs)   # noqa: E731

    def two_steps(hip):
        torch.manual_seed(5)
        (_, _, xy), target = SyntheticPriorDataset(n_images=1, size=32, kind="noisy_blob")[0]
        seg = UNet(in_chn=4, base_width=4)
        seg.load_state_dict(case["net"].state_dict())
        wrapper = WrapperModule(seg, factory(), use_segmentation_output_inversion=True).to(dev).train()
        bank = PriorBank(lambda: factory().to(dev), n_images=1, device=dev)
        bank.row(0)
        opt = torch.optim.Adam(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=0.0)
        tr = JointTrainer(wrapper, bank, FBMSJointLoss(alpha=1.0, beta=2.0), opt)
        args = (case["image"].to(dev), case["feat"].to(dev), xy[None].to(dev))
        tr.perform_step(0, args, target[None].to(dev))
        seg.hip_training = hip
        assert seg.hip_train_route(args[0], args[1]) == hip
        tr.perform_step(0, args, target[None].to(dev))
        assert tr._path == "fused"
        return [p.grad.detach().clone() for p in seg.parameters()]

    off, on = two_steps(False), two_steps(True)
    t64, t32 = U.tensors(case["f64"], case["net"])[1:75], U.tensors(case["f32"], case["net"])[1:75]
    assert len(on) == len(off) == len(t64) == 74
    for k, (a, b) in enumerate(zip(on, off)):
        src = k if t64[k][2] is None else t64[k][2] - 1
        rel = 4 * float((t32[src][1].double() - t64[src][1]).abs().max()) / float(t64[src][1].abs().max()) + 1e-6
        scale = float(off[src].abs().max())
        e = float((a - b).abs().max())
        print(f"[unet train joint] {t64[k][0]}: e {e:.3e}  bar {2 * rel * scale:.3e}")
        assert e <= 2 * rel * scale, f"{t64[k][0]}: e {e:.3e}  bar {2 * rel * scale:.3e}"
