#!/usr/bin/env python3
"""Time per joint-training step of the convexity benchmark's FCNet configs in pixel mode, through JointTrainer.perform_step:
FCNet(depth 3, width 16, 'rgbxy' input of 5 channels) + ConvexNet h = 130, AwesomeLossJoint with a plain BCELoss,
scribble_percentage 0.8, WrapperModule(input_mode='pixel', prior_arg_mode='param_clean_grid'), Adam, before and after the
extra-penalty hook, at n = 16 384 rows (an assumed pixel count of a scribbled item) and 90 000 rows (a whole 300 x 300 image).  Paths:

    prior_share  fused_convexity_losses: the segmentation share in torch, inrfit_joint_prior_step for the prior (the baseline)
    fcseg        + fused_segmentation: inrfit_fcseg_forward / _step around inrfit_joint_prior_step

and the isolated segmentation step: fcseg.step against the torch forward + BCE + backward of the same net on the same rows.

Each case: `--warmup` steps, then `--windows` windows of `--steps` steps between two device events; the median window is reported,
one JSON line each, with the baseline's fastest window beside the fused median (`fused_below_baseline_min`).

    python tools/kbench_joint_fcseg.py [--steps 50] [--windows 3] [--warmup 10] [--rows 16384,90000] [--only fcseg]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A

SP = 0.8


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


def data(dev, n):
    g = torch.Generator().manual_seed(0)
    n_scr = int(n * SP // 1)
    rgb, xy = torch.rand(1, n, 3, generator=g).to(dev), torch.rand(1, n, 2, generator=g).to(dev)
    target = torch.randint(0, 2, (1, n_scr, 1), generator=g).float().to(dev)
    return (rgb, xy.clone(), xy), target


def run_joint(dev, n, phase, path, args):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.measures import AwesomeLossJoint
    from awesome_amd.model import ConvexNet, FCNet, WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    torch.manual_seed(0)
    seg = FCNet(in_chn=5, out_chn=1, width=16, depth=3, in_type="rgbxy")
    wrapper = WrapperModule(seg, ConvexNet(n_hidden=130), use_segmentation_output_inversion=True, input_mode="pixel",
                            prior_arg_mode="param_clean_grid").to(dev)
    inputs, target = data(dev, n)
    crit = AwesomeLossJoint(criterion=torch.nn.BCELoss(), alpha=1.0, beta=1.0, gamma=1.0, scribble_percentage=SP)
    crit.extra_penalty = phase == "after"
    bank = PriorBank(lambda: ConvexNet(n_hidden=130).to(dev), n_images=1, device=dev)
    bank.row(0)
    opt = torch.optim.Adam(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    tr = JointTrainer(wrapper, bank, crit, opt, fused=True, fused_convexity_losses=True, fused_segmentation=path == "fcseg")
    times, (loss, _) = windows(lambda: tr.perform_step(0, inputs, target), args)
    return dict(bench="joint_step", n_rows=n, phase=phase, path=path, trainer_path=tr._path, steps=args.steps,
                windows_us=[round(t, 1) for t in times], us_per_step=round(sorted(times)[len(times) // 2], 1), loss_last=float(loss))


def run_isolated(dev, n, path, args):
    from awesome_amd import fcseg as FS
    from awesome_amd.model import FCNet
    torch.manual_seed(0)
    net = FCNet(in_chn=5, out_chn=1, width=16, depth=3, in_type="rgbxy").to(dev)
    (rgb, feat, _), target = data(dev, n)
    rgb, feat, target = rgb[0], feat[0], target[0]
    cnt = target.shape[0]
    if path == "fcseg":
        desc = FS.make_desc(net, 3, n, data_count=cnt, inversion=True)
        grads = torch.empty(FS.param_count(desc), dtype=torch.float32, device=dev)
        fn = lambda: FS.step(net, desc, rgb, feat, target, reuse_forward=True, grads=grads).loss   # noqa: E731
    else:
        def fn():
            for p in net.parameters():
                p.grad = None
            loss = torch.nn.functional.binary_cross_entropy(1 - torch.sigmoid(net(rgb, feat))[:cnt], target)
            loss.backward()
            return loss
    times, loss = windows(fn, args)
    return dict(bench="segmentation_step", n_rows=n, path=path, steps=args.steps, windows_us=[round(t, 1) for t in times],
                us_per_step=round(sorted(times)[len(times) // 2], 1), loss_last=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", default="16384,90000")
    ap.add_argument("--only", default=None, help="run one path only (profiling runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    build = A._lib.load().inrfit_build_info().decode()[:40]
    for n in (int(c) for c in args.rows.split(",")):
        for phase in ("before", "after"):
            base = None
            for path in ("prior_share", "fcseg"):
                if args.only and path != args.only:
                    continue
                r = run_joint(dev, n, phase, path, args)
                if path == "prior_share":
                    base = r
                elif base is not None:
                    r["baseline_min_us"] = min(base["windows_us"])
                    r["vs_prior_share"] = round(r["us_per_step"] / base["us_per_step"], 3)
                    r["fused_below_baseline_min"] = r["us_per_step"] < min(base["windows_us"])
                r["build"] = build
                print(json.dumps(r), flush=True)
        base = None
        for path in ("torch", "fcseg"):
            if args.only and path != args.only:
                continue
            r = run_isolated(dev, n, path, args)
            if path == "torch":
                base = r
            elif base is not None:
                r["baseline_min_us"] = min(base["windows_us"])
                r["vs_torch"] = round(r["us_per_step"] / base["us_per_step"], 3)
                r["fused_below_baseline_min"] = r["us_per_step"] < min(base["windows_us"])
            r["build"] = build
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
