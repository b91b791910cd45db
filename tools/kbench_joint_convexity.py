#!/usr/bin/env python3
"""Time per joint-training step for the convexity benchmark's losses, one image, through JointTrainer.perform_step (segmentation
network forward / backward and its optimizer step included), fused (JointTrainer(fused_convexity_losses=True): the segmentation share
in torch, inrfit_joint_prior_step for the prior's share) against autograd (the prior through the HIP autograd bridges, what every
step of these configs takes by default).  Prior: ConvexNet h = 130 (the configs' ConvexNet, one hidden layer), Adam.  Two cases:

    image   300 x 300 (the configs' patch_size), a small conv segmentation network over (image, features),
            AwesomeImageLossJoint with GradientPenaltyLoss(BCELoss, noneclass 2, xygrad 0.01, rgbgrad 0.01): second-order autograd
            through the segmentation network in both paths
    pixel   FCNet(depth 3, width 16) on (n, 3) pixel features (xy + one semantic feature), AwesomeLossJoint(BCELoss, scribble_percentage 0.8).  n = 16384 is an
            ASSUMED pixel count: no count has been measured for the convexity dataset.

Each (case, phase in before / after the extra-penalty hook, path): `--warmup` steps, then `--windows` windows of `--steps` steps
between two device events; the median window is reported, one JSON line each.

    python tools/kbench_joint_convexity.py [--steps 100] [--windows 3] [--warmup 10] [--cases image,pixel] [--pixels 16384]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A


class ImageSeg(torch.nn.Module):
    """A small conv segmentation network over (image, features)."""

    def __init__(self):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Conv2d(4, 16, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv2d(16, 1, 3, padding=1))

    def forward(self, image, feat, *args, **kwargs):
        return self.net(torch.cat([image, feat], dim=1))


def setup(dev, case, n_pixels):
    from awesome_amd.measures import AwesomeImageLossJoint, AwesomeLossJoint, GradientPenaltyLoss
    from awesome_amd.model import ConvexNet, FCNet, WrapperModule
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    if case == "image":
        S = 300
        seg = ImageSeg()
        wrapper = WrapperModule(seg, ConvexNet(n_hidden=130)).to(dev)
        img = torch.rand(1, 3, S, S, generator=g).to(dev).requires_grad_(True)
        feat = torch.rand(1, 1, S, S, generator=g).to(dev).requires_grad_(True)
        ys, xs = torch.meshgrid(torch.linspace(0, 1, S), torch.linspace(0, 1, S), indexing="ij")
        inputs = (img, feat, torch.stack([xs, ys])[None].to(dev))
        target = torch.randint(0, 3, (1, 1, S, S), generator=g).float().to(dev)
        crit = AwesomeImageLossJoint(criterion=GradientPenaltyLoss(torch.nn.BCELoss(), apply_gradient_penalty=True, xygrad=0.01,
                                                                   rgbgrad=0.01, noneclass=2.0), alpha=1.0, beta=1.0, gamma=1.0)
    else:
        seg = FCNet(in_chn=3, out_chn=1, width=16, depth=3)
        wrapper = WrapperModule(seg, ConvexNet(n_hidden=130), prior_arg_mode="xy_c_preattached", input_mode="pixel").to(dev)
        inputs = (torch.rand(1, n_pixels, 3, generator=g).to(dev),)
        target = (torch.rand(1, int(n_pixels * 0.8 // 1), 1, generator=g) > 0.6).float().to(dev)
        crit = AwesomeLossJoint(alpha=1.0, beta=1.0, gamma=1.0, scribble_percentage=0.8)
    return seg, wrapper, inputs, target, crit


def run_case(dev, case, phase, fused, args):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ConvexNet
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    seg, wrapper, inputs, target, crit = setup(dev, case, args.pixels)
    crit.extra_penalty = phase == "after"
    bank = PriorBank(lambda: ConvexNet(n_hidden=130).to(dev), n_images=1, device=dev)
    bank.row(0)
    opt = torch.optim.Adam(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=2e-2)
    tr = JointTrainer(wrapper, bank, crit, opt, fused=fused, fused_convexity_losses=True)
    for _ in range(args.warmup):
        tr.perform_step(0, inputs, target)
    path = tr._path
    torch.cuda.synchronize()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            loss, _ = tr.perform_step(0, inputs, target)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    med = sorted(times)[len(times) // 2]
    n = inputs[0].shape[-2] * inputs[0].shape[-1] if case == "image" else args.pixels
    return dict(case=case, phase=phase, path=path, n_points=n, steps=args.steps, windows=[round(t, 4) for t in times],
                us_per_step=round(med / args.steps * 1e6, 1), loss_last=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default="image,pixel")
    ap.add_argument("--pixels", type=int, default=16384, help="pixel-mode point count (an assumption, see the module docstring)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    build = A._lib.load().inrfit_build_info().decode()[:40]
    for case in args.cases.split(","):
        for phase in ("before", "after"):
            auto = None
            for fused in (False, True):
                r = run_case(dev, case, phase, fused, args)
                auto = r["us_per_step"] if not fused else auto
                r["vs_autograd"] = round(r["us_per_step"] / auto, 3)
                r["build"] = build
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
