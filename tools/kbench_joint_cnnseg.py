#!/usr/bin/env python3
"""Time per joint-training step of the convexity benchmark's CNNNet configs, one 300 x 300 image, through JointTrainer.perform_step:
CNNNet(depth 2, width 16, kernel 3, 'rgbxy' input of C_in = 5 or 7 channels) + ConvexNet h = 130, AwesomeImageLossJoint with the
configs' GradientPenaltyLoss(BCELoss, noneclass 2, xygrad 0.01, rgbgrad 0.01, featgrad 0), Adam, before and after the extra-penalty
hook.  Three paths:

    autograd     JointTrainer(fused=False): everything in torch (the prior through the HIP autograd bridges)
    prior_share  fused_convexity_losses: the segmentation share in torch (double backward), inrfit_joint_prior_step for the prior
    cnnseg       fused_convexity_losses + fused_segmentation: inrfit_cnnseg_forward / _step around inrfit_joint_prior_step

Each (C_in, phase, path): `--warmup` steps, then `--windows` windows of `--steps` steps between two device events; the median window
is reported, one JSON line each (vs_autograd / vs_prior_share: ratios of the step times).

    python tools/kbench_joint_cnnseg.py [--steps 50] [--windows 3] [--warmup 10] [--cin 5,7]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A

S = 300


def setup(dev, cin):
    from awesome_amd.measures import AwesomeImageLossJoint, GradientPenaltyLoss
    from awesome_amd.model import CNNNet, ConvexNet, WrapperModule
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    seg = CNNNet(in_chn=cin, out_chn=1, kernel_size=3, width=16, depth=2, in_type="rgbxy")
    wrapper = WrapperModule(seg, ConvexNet(n_hidden=130), use_segmentation_output_inversion=True).to(dev)
    img = torch.rand(1, 3, S, S, generator=g).to(dev).requires_grad_(True)
    feat = torch.rand(1, cin - 3, S, S, generator=g).to(dev).requires_grad_(True)
    ys, xs = torch.meshgrid(torch.linspace(0, 1, S), torch.linspace(0, 1, S), indexing="ij")
    inputs = (img, feat, torch.stack([xs, ys])[None].to(dev))
    target = torch.randint(0, 3, (1, 1, S, S), generator=g).float().to(dev)
    crit = AwesomeImageLossJoint(criterion=GradientPenaltyLoss(torch.nn.BCELoss(), apply_gradient_penalty=True, xygrad=0.01,
                                                               rgbgrad=0.01, featgrad=0.0, noneclass=2.0,
                                                               xytype="xy" if cin == 5 else "featxy"), alpha=1.0, beta=1.0, gamma=1.0)
    return seg, wrapper, inputs, target, crit


def run_case(dev, cin, phase, path, args):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ConvexNet
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    seg, wrapper, inputs, target, crit = setup(dev, cin)
    bank = PriorBank(lambda: ConvexNet(n_hidden=130).to(dev), n_images=1, device=dev)
    bank.row(0)
    opt = torch.optim.Adam(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    tr = JointTrainer(wrapper, bank, crit, opt, fused=path != "autograd", fused_convexity_losses=True,
                      fused_segmentation=path == "cnnseg")

    def one():
        crit.extra_penalty = phase == "after"
        return tr.perform_step(0, inputs, target)
    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            loss, _ = one()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    med = sorted(times)[len(times) // 2]
    return dict(cin=cin, phase=phase, path=path, trainer_path=tr._path, n_points=S * S, steps=args.steps,
                windows=[round(t, 4) for t in times], us_per_step=round(med / args.steps * 1e6, 1), loss_last=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cin", default="5,7")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    build = A._lib.load().inrfit_build_info().decode()[:40]
    for cin in (int(c) for c in args.cin.split(",")):
        for phase in ("before", "after"):
            ref = {}
            for path in ("autograd", "prior_share", "cnnseg"):
                r = run_case(dev, cin, phase, path, args)
                ref[path] = r["us_per_step"]
                r["vs_autograd"] = round(r["us_per_step"] / ref["autograd"], 3)
                if path == "cnnseg":
                    r["vs_prior_share"] = round(r["us_per_step"] / ref["prior_share"], 3)
                r["build"] = build
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
