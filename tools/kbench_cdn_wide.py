#!/usr/bin/env python3
"""Time per optimizer step of ConvexDiffeomorphismNet over ICNNs of the layer-by-layer path at 256 x 256, behind the config flow
(6 couplings, width 130, normal_block; config/c2_blob256_cdn_wide256.yaml):

    cdn_h256_l1   ICNN n_hidden 256, one hidden layer
    cdn_h130_l3   ICNN n_hidden 130, three hidden layers

Two benches, each with both routes in the same process:

    fit          `device`: the device-resident fit (inrfit_cdn_fit, `--steps` steps per call, what
                 pretrain(device_fit_layer_by_layer=True) runs)                    against
                 `generic`: ConvexDiffeomorphismNet._generic_fit (pretrain's default for these shapes: torch.optim.Adam +
                 ReduceLROnPlateau over the module's autograd step, one host round trip per step)
    joint_step   `fused`: JointTrainer(fused_layer_by_layer=True, fused_cdn_layer_by_layer=True): inrfit_cdn_wide_joint_step   against
                 `autograd`: the default trainer (WrapperModule forward through the composite's autograd bridge, torch's optimizer,
                 enforce_convexity); FBMSJointLoss and a one-convolution stand-in for the backbone

Each case: `--warmup` steps, then `--windows` windows of `--steps` steps between two device events; the median window is reported with
the spread of the windows, one JSON line each (also appended to profiles/cdn_wide_kbench.jsonl), with the other route's fastest window
beside the device route's median (`below_baseline_min`); the exit status is 1 when any device median is not below it.

    python tools/kbench_cdn_wide.py [--steps 50] [--windows 3] [--warmup 5] [--size 256] [--bench fit|joint_step]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A

SHAPES = {"cdn_h256_l1": (256, 1), "cdn_h130_l3": (130, 3)}


class Seg(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 1, 3, padding=1)

    def forward(self, image, *args, **kwargs):
        return self.conv(image)


def factory(name):
    from awesome_amd.model import ConvexDiffeomorphismNet
    h, layers = SHAPES[name]
    return lambda: ConvexDiffeomorphismNet(n_hidden=h, n_hidden_layers=layers, nf_layers=6, nf_hidden=130,
                                           diffeo_args=dict(backbone="normal_block"))


def windows(fn, args, per_call=1):
    """`fn` takes `per_call` optimizer steps; -> microseconds per optimizer step of every window, fn's last result."""
    calls = max(1, args.steps // per_call)
    for _ in range(max(1, args.warmup // per_call)):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / (calls * per_call))
    return times, out


def record(bench, name, path, times, args, **extra):
    med = sorted(times)[len(times) // 2]
    return dict(bench=bench, prior=name, size=args.size, path=path, steps=args.steps, windows_us=[round(t, 1) for t in times],
                us_per_step=round(med, 1), spread=round((max(times) - min(times)) / med, 4), **extra)


def run_fit(dev, name, path, args):
    from awesome_amd.dataset import convex_blob_unaries
    torch.manual_seed(0)
    m = factory(name)().to(dev)
    S = args.size
    un = (convex_blob_unaries(S, 0).reshape(1, -1) > 0.5).float().to(dev)
    xs = torch.linspace(0, 1, S, device=dev)
    grid = A.Grid.explicit(torch.stack([xs[None, :].expand(S, S), xs[:, None].expand(S, S)], 0).reshape(2, -1).contiguous())
    if path == "device":
        times, out = windows(lambda: m.fit_images(grid, un, num_epochs=args.steps, lr=3e-3, loss="se"), args, per_call=args.steps)
        loss = float(out.loss_hist[0, -1])
    else:
        from awesome_amd.measures import SE, UnariesConversionLoss
        flat = torch.cat([p.detach().reshape(-1) for _, p in m.named_parameters()])[None].contiguous()
        opts = dict(lr=3e-3, criterion=UnariesConversionLoss(SE("mean")))
        times, out = windows(lambda: m._generic_fit(grid, un, flat, args.steps, opts), args, per_call=args.steps)
        loss = float(((torch.sigmoid(out[1][0]) - un[0]) ** 2).mean())
    return record("fit", name, path, times, args, loss_last=loss)


def run_joint(dev, name, path, args):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.dataset import SyntheticPriorDataset
    from awesome_amd.measures import FBMSJointLoss
    from awesome_amd.model import WrapperModule
    from awesome_amd.prior_bank import PriorBank, _ordered_parameters
    make = factory(name)
    torch.manual_seed(0)
    ds = SyntheticPriorDataset(n_images=1, size=args.size, kind="noisy_blob")
    (image, _, xy), target = ds[0]
    seg = Seg()
    wrapper = WrapperModule(seg, make(), use_segmentation_output_inversion=True).to(dev)
    bank = PriorBank(lambda: make().to(dev), n_images=1, device=dev)
    bank.row(0)
    opt = torch.optim.Adam(list(seg.parameters()) + list(_ordered_parameters(wrapper.prior_module)), lr=1e-3)
    fused = path == "fused"
    tr = JointTrainer(wrapper, bank, FBMSJointLoss(alpha=1.0, beta=2.0, clip_penalty=True), opt, fused_layer_by_layer=fused,
                      fused_cdn_layer_by_layer=fused)
    inputs = (image[None].to(dev), torch.zeros(1, 1, 1, 1, device=dev), xy[None].to(dev))
    tgt = target[None].to(dev)
    times, (loss, _) = windows(lambda: tr.perform_step(0, inputs, tgt), args)
    assert tr._path == path, (tr._path, path)
    return record("joint_step", name, path, times, args, loss_last=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--bench", default=None, choices=["fit", "joint_step"], help="run one bench only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdn_wide_kbench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    build = A._lib.load().inrfit_build_info().decode()[:40]
    slower = []
    for bench, fn, routes in (("fit", run_fit, ("generic", "device")), ("joint_step", run_joint, ("autograd", "fused"))):
        if args.bench and bench != args.bench:
            continue
        for name in SHAPES:
            base = fn(dev, name, routes[0], args)
            r = fn(dev, name, routes[1], args)
            r["baseline_min_us"] = min(base["windows_us"])
            r["vs_" + routes[0]] = round(r["us_per_step"] / base["us_per_step"], 3)
            r["below_baseline_min"] = r["us_per_step"] < min(base["windows_us"])
            if not r["below_baseline_min"]:
                slower.append(f"{bench}:{name}")
            for rec in (base, r):
                rec["build"] = build
                print(json.dumps(rec), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(rec) + "\n")
    if slower:
        sys.exit(f"device route not below the other route's fastest window: {slower}")


if __name__ == "__main__":
    main()
