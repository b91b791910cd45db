#!/usr/bin/env python3
"""Time per joint-training step at 256 x 256 with AwesomeImageLoss, one image, through JointTrainer.perform_step (backbone stand-in
forward / backward and its optimizer step included), for three cases:

    fused            the fused step, extra penalty off
    fused_penalty    the fused step, extra penalty on (JointTrainer(fused_extra_penalty=True): the step kernel's align mode)
    autograd_penalty the autograd step, extra penalty on (what JointTrainer takes by default once the runner's hook has fired)

Priors: ConvexNextNet h = 130 L = 1 and L = 2 (Adam), and the path-connected prior of config/c5_refine_noisy256.yaml (RealNVP
12 flows x 32, ICNN 130 x 2, Adamax).  Each case: `--warmup` steps, then `--windows` windows of `--steps` steps between two device
events (no host sync inside a window); the median window is reported, one JSON line per (prior, case).

    python tools/kbench_joint_penalty.py [--steps 200] [--windows 3] [--warmup 20] [--priors h130_l1,h130_l2,c5_pcn]
Under `rocprofv3 --kernel-trace --stats` it gives the per-kernel table of the three paths."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A


class SegStandIn(torch.nn.Module):
    """The backbone stand-in of the joint tests: one 3x3 convolution over the noisy logit image."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)

    def forward(self, image, *args, **kwargs):
        return self.conv(image)


def prior_factory(name):
    from awesome_amd.model import ConvexNextNet, real_nvp_path_connected_net
    if name == "h130_l1":
        return (lambda: ConvexNextNet(n_hidden=130, in_features=2, n_hidden_layers=1)), torch.optim.Adam
    if name == "h130_l2":
        return (lambda: ConvexNextNet(n_hidden=130, in_features=2, n_hidden_layers=2)), torch.optim.Adam
    if name == "c5_pcn":
        return (lambda: real_nvp_path_connected_net(channels=2, hidden_units=32, flow_n_flows=12, flow_output_fn="tanh",
                                                    convex_net_hidden_units=130, convex_net_hidden_layers=2)), torch.optim.Adamax
    raise SystemExit(f"unknown prior {name}")


def run_case(dev, name, case, args):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.measures import AwesomeImageLoss
    from awesome_amd.model import WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    factory, opt_type = prior_factory(name)
    torch.manual_seed(0)
    (image, _, xy), target = SyntheticPriorDataset(n_images=1, size=256, kind="noisy_blob")[0]
    seg = SegStandIn()
    wrapper = WrapperModule(seg, factory(), use_segmentation_output_inversion=True).to(dev)
    bank = PriorBank(lambda: factory().to(dev), n_images=1, device=dev)
    bank.row(0)
    for b_name, b in wrapper.prior_module.named_buffers():   # ActNorm as after the per-image pre-fit: every step may be fused
        if b_name.endswith("data_dep_init_done"):
            b.fill_(1.0)
    crit = AwesomeImageLoss(alpha=1.0)
    crit.extra_penalty = case != "fused"
    opt = opt_type(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-4)
    tr = JointTrainer(wrapper, bank, crit, opt, fused=case != "autograd_penalty", fused_extra_penalty=case == "fused_penalty")
    step_args = (0, (image[None].to(dev), torch.zeros(1, 1, 1, 1, device=dev), xy[None].to(dev)), target[None].to(dev))
    for _ in range(args.warmup):
        tr.perform_step(*step_args)
    path = tr._path
    torch.cuda.synchronize()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            loss, _ = tr.perform_step(*step_args)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    tr.raise_if_failed()
    med = sorted(times)[len(times) // 2]
    return dict(prior=name, case=case, path=path, size=256, steps=args.steps, windows=[round(t, 4) for t in times],
                us_per_step=round(med / args.steps * 1e6, 1), loss_last=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--priors", default="h130_l1,h130_l2,c5_pcn")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.priors.split(","):
        base = None
        for case in ("fused", "fused_penalty", "autograd_penalty"):
            r = run_case(dev, name, case, args)
            base = r["us_per_step"] if case == "fused" else base
            r["vs_fused"] = round(r["us_per_step"] / base, 3)
            r["build"] = A._lib.load().inrfit_build_info().decode()[:40]
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
