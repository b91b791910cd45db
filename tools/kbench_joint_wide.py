#!/usr/bin/env python3
"""Time per joint-training step for priors on the layer-by-layer path, through JointTrainer.perform_step at 256 x 256 with
FBMSJointLoss (config/c5_refine_noisy256.yaml's loss) and a one-convolution stand-in for the backbone:

    convexnext_h256_l1   ConvexNextNet n_hidden 256, one hidden layer (Adam)
    convexnext_h130_l3   ConvexNextNet n_hidden 130, three hidden layers (Adam)
    pcn_c2_wide256       the path-connected prior of config/c2_blob256_path_connected_wide256.yaml: 12 flows x 32 over an ICNN of
                         256 units (Adamax)

Paths, in the same process: `autograd` (the default trainer: WrapperModule forward through the HIP autograd bridges, torch's optimizer,
enforce_convexity) and `fused` (JointTrainer(fused_layer_by_layer=True): inrfit_wide_joint_step / inrfit_pcn_wide_joint_step).

Each case: `--warmup` steps, then `--windows` windows of `--steps` steps between two device events; the median window is reported, one
JSON line each (also appended to profiles/joint_wide_kbench.jsonl), with the autograd route's fastest window beside the fused median
(`fused_below_baseline_min`); the exit status is 1 when any fused median is not below it.

    python tools/kbench_joint_wide.py [--steps 50] [--windows 3] [--warmup 10] [--size 256] [--only fused]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A


class Seg(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)

    def forward(self, image, *args, **kwargs):
        return self.conv(image)


def windows(fn, args):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / args.steps)
    return times, out


def priors():
    from awesome_amd.model import ConvexNextNet, real_nvp_path_connected_net
    return {
        "convexnext_h256_l1": (lambda: ConvexNextNet(n_hidden=256, in_features=2, n_hidden_layers=1), torch.optim.Adam),
        "convexnext_h130_l3": (lambda: ConvexNextNet(n_hidden=130, in_features=2, n_hidden_layers=3), torch.optim.Adam),
        "pcn_c2_wide256": (lambda: real_nvp_path_connected_net(channels=2, hidden_units=32, flow_n_flows=12, flow_output_fn="tanh",
                                                               convex_net_hidden_units=256, convex_net_hidden_layers=2),
                           torch.optim.Adamax),
    }


def run(dev, name, path, args):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.measures import FBMSJointLoss
    from awesome_amd.model import WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    factory, opt_type = priors()[name]
    torch.manual_seed(0)
    ds = SyntheticPriorDataset(n_images=1, size=args.size, kind="noisy_blob")
    (image, _, xy), target = ds[0]
    seg = Seg()
    wrapper = WrapperModule(seg, factory(), use_segmentation_output_inversion=True).to(dev)
    bank = PriorBank(lambda: factory().to(dev), n_images=1, device=dev)
    bank.row(0)
    with torch.no_grad():    # ActNorm marked initialised (its data-dependent first forward is the autograd step's on either path)
        for b_name, b in wrapper.prior_module.named_buffers():
            if b_name.endswith("data_dep_init_done"):
                b.fill_(1.0)
    opt = opt_type(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    tr = JointTrainer(wrapper, bank, FBMSJointLoss(alpha=1.0, beta=2.0, clip_penalty=True), opt, fused_layer_by_layer=path == "fused")
    inputs = (image[None].to(dev), torch.zeros(1, 1, 1, 1, device=dev), xy[None].to(dev))
    tgt = target[None].to(dev)
    times, (loss, _) = windows(lambda: tr.perform_step(0, inputs, tgt), args)
    return dict(bench="joint_step_layer_by_layer", prior=name, size=args.size, path=path, trainer_path=tr._path, steps=args.steps,
                windows_us=[round(t, 1) for t in times], us_per_step=round(sorted(times)[len(times) // 2], 1), loss_last=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--only", default=None, help="run one path only (profiling runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_wide_kbench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    build = A._lib.load().inrfit_build_info().decode()[:40]
    slower = []
    for name in priors():
        base = None
        for path in ("autograd", "fused"):
            if args.only and path != args.only:
                continue
            r = run(dev, name, path, args)
            assert r["trainer_path"] == path, r
            if path == "autograd":
                base = r
            elif base is not None:
                r["baseline_min_us"] = min(base["windows_us"])
                r["vs_autograd"] = round(r["us_per_step"] / base["us_per_step"], 3)
                r["fused_below_baseline_min"] = r["us_per_step"] < min(base["windows_us"])
                if not r["fused_below_baseline_min"]:
                    slower.append(name)
            r["build"] = build
            print(json.dumps(r), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(r) + "\n")
    if slower:
        sys.exit(f"fused step not below the autograd route's fastest window: {slower}")


if __name__ == "__main__":
    main()
