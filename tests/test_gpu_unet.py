"""The UNet backbone's evaluation pass in HIP (awesome_amd.unet, include/inrfit.h inrfit_unet_*, csrc/unet.h) against float64.

Yardstick of every comparison: the same module's .double() copy evaluated by torch on the CPU (for the 17 x 31 / width 64 case also the
reference class's recorded float64 output, tests/golden/unet_eval.npz).  In the same test the error of torch's own fp32 CPU pass against
that yardstick is measured, e_torch = max|fp32 - float64|, and the HIP result must satisfy

    max|hip - float64| <= 4 e_torch + 1e-6 max|float64|

The factor 4 allows for a different but equally long summation order (16-wide k-steps, contractions up to K = 9 217 cut into slices):
a margin over the reference arithmetic's own error, not a number taken from the kernels.  Measured errors: profiles/unet_parity.md.

Every BatchNorm is moved away from the identity (tools/gen_golden_unet.py perturb_batchnorm_), so the fold is exercised."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _net(base_width, out_chn=1, seed=307):
    import gen_golden_unet as G
    from awesome_amd.model import UNet
    torch.manual_seed(seed)
    net = UNet(in_chn=4, out_chn=out_chn, base_width=base_width)
    G.perturb_batchnorm_(net, seed + 1)
    return net.eval()


def _inputs(h, w, seed=309):
    import gen_golden_unet as G
    return G.make_inputs(seed, h, w)


def _references(net, image, feat):
    """(float64 output, fp32 CPU torch output) of the CPU module."""
    with torch.no_grad():
        out64 = copy.deepcopy(net).double()(image.double(), feat.double())
        out32 = net(image, feat)
    return out64, out32


def _check(hip, out64, out32, what):
    """The parity bar of the module docstring; both errors go into the message (and, with -s, to the output)."""
    hip = hip.detach().cpu().double()
    assert hip.shape == out64.shape, (what, tuple(hip.shape), tuple(out64.shape))
    assert bool(torch.isfinite(hip).all()), what
    e_torch = float((out32.double() - out64).abs().max())
    e_hip = float((hip - out64).abs().max())
    bar = 4 * e_torch + 1e-6 * float(out64.abs().max())
    msg = f"{what}: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}  max|f64| {float(out64.abs().max()):.3e}"
    print("[unet parity]", msg)
    assert e_hip <= bar, msg
    return e_hip, e_torch


_state = {}


def _case(dev, h, w, base, out_chn=1):
    """The CPU module and its references, computed once per shape and shared by the tests; the module on the GPU is a copy."""
    key = (h, w, base, out_chn)
    if key not in _state:
        net = _net(base, out_chn)
        image, feat = _inputs(h, w)
        out64, out32 = _references(net, image, feat)
        _state[key] = (net, image, feat, out64, out32)
    net, image, feat, out64, out32 = _state[key]
    return copy.deepcopy(net).to(dev).eval(), image, feat, out64, out32


CASES = [
    # h, w, base_width, strip_points, out_chn
    (16, 16, 8, 0, 1),        # the bottom level is 1 x 1: upsampling starts from one pixel
    (17, 31, 8, 0, 1),        # odd at every level: an asymmetric pad in every Up block, max-pool drops a row and a column
    (17, 31, 64, 0, 1),
    (40, 56, 8, 512, 1),      # strips end inside image rows (512 is no multiple of 56)
    (64, 48, 64, 0, 1),       # the default strip (two strips at full resolution), split-K levels, full channel widths
    (17, 31, 8, 0, 3),        # several output channels
]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,base,strip,out_chn", CASES, ids=[f"{h}x{w}-b{b}-s{s}-o{o}" for h, w, b, s, o in CASES])
def test_parity_with_float64(dev, golden_dir, h, w, base, strip, out_chn):
    from awesome_amd.unet import unet_forward
    net, image, feat, out64, out32 = _case(dev, h, w, base, out_chn)
    with torch.no_grad():
        hip = unet_forward(net, image.to(dev), feat.to(dev), strip_points=strip)
    _check(hip, out64, out32, f"{h}x{w} base {base} strip {strip or 'default'} out {out_chn}")
    if (h, w, base, out_chn) == (17, 31, 64, 1):
        # the fixture's item through the same seeded module: the reference class's own float64 output is the yardstick, too
        fx = np.load(os.path.join(golden_dir, "unet_eval.npz"))
        fimage, ffeat = torch.from_numpy(fx["image"]), torch.from_numpy(fx["feat"])
        with torch.no_grad():
            hip_fx = unet_forward(net, fimage.to(dev), ffeat.to(dev))
        _check(hip_fx, torch.from_numpy(fx["out64"]), torch.from_numpy(fx["out32"]), "17x31 base 64 against the reference fixture")


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(dev):
    from awesome_amd.unet import unet_forward
    net, image, feat, _, _ = _case(dev, 17, 31, 64)        # (levels 1 .. 4 take the split-K product at this size)
    image, feat = image.to(dev), feat.to(dev)
    with torch.no_grad():
        a = unet_forward(net, image, feat).clone()
        net.__dict__.pop("_hip_unet_cache")                 # the second call packs again, into fresh buffers
        b = unet_forward(net, image, feat)
        c = unet_forward(net, torch.cat([image, image]), torch.cat([feat, feat]))
    assert torch.equal(a, b)
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[0])   # the images of a batch run one after the other


@pytest.mark.gpu
def test_changed_weights_are_packed_again(dev):
    from awesome_amd.unet import unet_forward
    net, image, feat, out64, out32 = _case(dev, 17, 31, 8)
    cpu = _state[(17, 31, 8, 1)][0]
    image_d, feat_d = image.to(dev), feat.to(dev)
    with torch.no_grad():
        before = unet_forward(net, image_d, feat_d).clone()
        _check(before, out64, out32, "before the edit")
        # an in-place edit of a buffer
        cpu2 = copy.deepcopy(cpu)
        cpu2.down2.mpconv[1].conv[1].running_mean.add_(0.5)
        net.down2.mpconv[1].conv[1].running_mean.add_(0.5)
        after = unet_forward(net, image_d, feat_d).clone()
        assert not torch.equal(after, before)
        _check(after, *_references(cpu2, image, feat), "after running_mean.add_(0.5)")
        # load_state_dict of other weights
        other = _net(8, seed=911)
        net.load_state_dict(other.state_dict())
        loaded = unet_forward(net, image_d, feat_d)
        assert not torch.equal(loaded, after)
        _check(loaded, *_references(other, image, feat), "after load_state_dict")
        # unchanged weights are not packed again
        packed = net.__dict__["_hip_unet_cache"]["packed"]
        unet_forward(net, image_d, feat_d)
        assert net.__dict__["_hip_unet_cache"]["packed"] is packed


@pytest.mark.gpu
def test_forward_routes_by_mode(dev):
    from awesome_amd.unet import unet_forward
    net, image, feat, _, _ = _case(dev, 17, 31, 8)
    image, feat = image.to(dev), feat.to(dev)
    with torch.no_grad():
        assert torch.equal(net(image, feat), unet_forward(net, image, feat))
        assert torch.equal(net(image[0], feat[0]), unet_forward(net, image, feat))      # a single item is batcherized
    out = net(image, feat)                                  # eval() with grad enabled: torch
    assert out.grad_fn is not None
    net.train()
    out = net(torch.cat([image, image]), torch.cat([feat, feat]))                         # train(): torch, batch statistics
    assert out.grad_fn is not None and "_hip_unet_cache" in net.__dict__
    with torch.no_grad():
        assert not net.hip_route(image, feat)


class _Agent:
    def __init__(self, ds, dev):
        self.training_dataset, self.device, self.logger = ds, dev, None


@pytest.mark.gpu
def test_unaries_of_the_prefit_loop_and_a_fit_on_them(dev):
    """In place: WrapperModule(UNet, ConvexNextNet).eval() on a 32 x 32 RGB + one-feature item - PriorFitMixin._collect turns the image
    into unaries with the HIP pass, and a 50-epoch pretrain on them leaves a finite prior in the cache."""
    from awesome_amd.dataset.prior_dataset import PriorDataset, prior
    from awesome_amd.model import ConvexNextNet, WrapperModule
    args = dict(n_hidden=130, in_features=2, n_hidden_layers=1)
    S = 32
    net = _net(8, seed=521)
    image, feat = _inputs(S, S, seed=523)
    with torch.no_grad():       # spread the logits over both classes, so that the item is not skipped as "no foreground"
        raw = copy.deepcopy(net).double()(image.double(), feat.double())
        net.outc.conv.weight.mul_(2.0 / float(raw.std()))
        net.outc.conv.bias.sub_(float(raw.mean())).mul_(2.0 / float(raw.std()))
    out64, out32 = _references(net, image, feat)
    un64, un32 = 1 - torch.sigmoid(out64), 1 - torch.sigmoid(out32)
    assert 0.2 < float((un64 >= 0.5).double().mean()) < 0.8

    class _Items(PriorDataset):
        returns_index = False

        def __len__(self):
            return 1

        @prior()
        def __getitem__(self, i):
            xs = torch.linspace(0, 1, S)
            xy = torch.stack([xs[None, :].expand(S, S), xs[:, None].expand(S, S)], 0).contiguous()
            return (image[0], feat[0], xy), (un64[0] >= 0.5).float()

    torch.manual_seed(3)
    ds = _Items(prior_model_type=ConvexNextNet, prior_model_args=args)
    wrapper = WrapperModule(copy.deepcopy(net), ConvexNextNet(**args), use_segmentation_output_inversion=True).to(dev).eval()
    images = wrapper.prior_module._collect(ds, ds, wrapper, dev)
    assert len(images) == 1 and not images[0].skip and images[0].unaries.shape == (1, 1, S, S)
    assert "packed" in wrapper.segmentation_module.__dict__["_hip_unet_cache"]        # the HIP pass ran
    _check(images[0].unaries, un64, un32, "unaries of _collect, 32x32 base 8")
    state = wrapper.pretrain(train_set=ds, test_set=None, device=dev, agent=_Agent(ds, dev), use_progress_bar=False, num_epochs=50,
                             reuse_state=False)
    rep = wrapper.prior_module.pretrain_report
    assert len(rep) == 1 and rep[0]["status"] == 0 and not rep[0]["skipped"] and np.isfinite(rep[0]["iou"]), rep   # status 0: finite loss
    assert sorted(state["cache"]) == ["0"]
    assert all(bool(torch.isfinite(v).all()) for v in state["cache"]["0"].values() if v.is_floating_point())


@pytest.mark.gpu
@pytest.mark.parametrize("checkpoint_width", [8, 12])
def test_run_py_builds_the_unet_by_its_reference_name_and_loads_its_checkpoint(tmp_path, checkpoint_width):
    """scripts/run.py with `segmentation_model_type: awesome.model.unet.UNet`: the joint epochs build the mirror from
    segmentation_model_args (width 8), load segmentation_model_state_dict_path into it and train it (torch modules: batch statistics,
    autograd).  A checkpoint of width 12 is refused by load_state_dict, which shows that the file is read."""
    from awesome_amd.model import UNet
    torch.manual_seed(5)
    ckpt = str(tmp_path / "unet.pth")
    torch.save(UNet(in_chn=3, base_width=checkpoint_width).state_dict(), ckpt)
    override = {"segmentation_model_type": "awesome.model.unet.UNet", "segmentation_model_args": {"in_chn": 3, "base_width": 8},
                "segmentation_model_state_dict_path": ckpt, "dataset_args": {"n_images": 1, "size": 64, "features": "xy"},
                "agent_args": {"joint_epochs": 2, "pretrain_args": {"num_epochs": 80}}}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--config-path",
                          os.path.join(ROOT, "config", "c5_refine_noisy256.yaml"), "--output-folder", str(tmp_path / "out"),
                          "--override", json.dumps(override)], capture_output=True, text=True, timeout=600)
    if checkpoint_width != 8:
        assert out.returncode != 0 and "size mismatch" in out.stderr, out.stderr[-2000:]
        return
    assert out.returncode == 0, out.stderr[-3000:]
    summary = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert summary["images"] == 1 and summary["joint_epochs"] == 2 and summary["priors_saved"] == 1
    assert all(np.isfinite(v) for v in summary["joint_loss_first_last"]), summary
