#!/usr/bin/env python3
"""Time per optimizer step of PathConnectedNet over an ICNN of the layer-by-layer path (n_hidden > 130 or more than two hidden layers),
at 256 x 256, C = 2, RealNVP 12 flows x 32 hidden units, for every --shapes entry h x L:

    pcn_fit    `inrfit_pcn_fit`: RealNVP forward, wide forward / backward with dcoords, ICNN update, seeded RealNVP backward, its update
    autograd   the same step as device-side autograd - get_deformation(differentiable=True) -> ConvexNextNet, SE loss, backward,
               torch.optim.Adamax, enforce_convexity (the only alternative to the call above)
    icnn_fit   the plain layer-by-layer ICNN step (`inrfit_fit`) on the same grid: pcn_fit minus this is the RealNVP's share

Each case: `--warmup` steps, then `--windows` windows of `--steps` steps between two device events; the median window is reported,
one JSON line each.

    python tools/kbench_pcn_wide.py [--steps 20] [--windows 3] [--warmup 3] [--shapes 256x1,130x3] [--size 256]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A
from awesome_amd import rnvp as R


def windows(fn, args):
    fn(args.warmup)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(args.steps)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / args.steps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="256x1,130x3")
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    from awesome_amd.model import real_nvp_path_connected_net
    dev = torch.device("cuda:0")
    S = args.size
    build = A._lib.load().inrfit_build_info().decode()[:40]
    grid = A.Grid.linspace(S, S, dev)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    un = (((yy - 0.45 * S) ** 2 + (xx - 0.5 * S) ** 2) > 0.07 * S * S).float().reshape(1, -1).to(dev)
    xs = torch.linspace(0, 1, S)
    image_grid = torch.stack([xs[None, :].expand(S, S), xs[:, None].expand(S, S)], 0)[None].to(dev)
    for h, L in ((int(a), int(b)) for a, b in (s.split("x") for s in args.shapes.split(","))):
        torch.manual_seed(0)
        m = real_nvp_path_connected_net(channels=2, hidden_units=32, flow_n_flows=12, flow_output_fn="tanh", convex_net_hidden_units=h,
                                        convex_net_hidden_layers=L).to(dev)
        m._actnorm_init_if_needed(m._first_image_coords(grid))
        ispec, rspec, icnn, flow = m._ordered_params()
        ip, fp = m._flat(icnn), m._flat(flow)
        out = dict(bench="pcn_wide_step", n_hidden=h, n_layers=L, size=S, n_flows=12, flow_hidden=32, steps=args.steps, build=build)

        def pcn(n):
            R.pcn_fit(ispec, rspec, ip.clone(), fp.clone(), grid, un, n, lr=1e-3, record_loss=False, want_logits=False)

        def plain(n):
            A.fit(ispec, ip.clone(), grid, un, n, lr=1e-3, optimizer="adamax", plateau=None, record_loss=False, want_logits=False)

        opt = torch.optim.Adamax([{"params": [p for k, p in m.named_parameters() if k.startswith("flow_net.")], "weight_decay": 1e-5},
                                  {"params": [p for k, p in m.named_parameters() if not k.startswith("flow_net.")]}], lr=1e-3)

        def autograd(n):
            for _ in range(n):
                opt.zero_grad(set_to_none=True)
                xd = m.get_deformation(image_grid, differentiable=True)
                loss = ((torch.sigmoid(m.convex_net(xd)).reshape(1, -1) - un) ** 2).mean()
                loss.backward()
                opt.step()
                m.enforce_convexity()

        for name, fn in (("pcn_fit", pcn), ("icnn_fit", plain), ("autograd", autograd)):
            t = windows(fn, args)
            out[name + "_windows_us"] = [round(x, 1) for x in t]
            out[name + "_us_per_step"] = round(sorted(t)[len(t) // 2], 1)
        out["rnvp_share_us"] = round(out["pcn_fit_us_per_step"] - out["icnn_fit_us_per_step"], 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
