#!/usr/bin/env python3
"""Time per full-batch optimizer step of the star-shape prior's dense fit, StarShapedNet(130), on grids of 256 x 256 and 480 x 640
pixels, on two routes over the same image:

    device     all steps in one `inrfit_star_fit_dense` call (csrc/star.h: tiles of inrfit_star_dense_tile_points() points, twelve
               launches per tile, one update launch per step)
    autograd   what the module offered before that call existed: `StarShapedNet.forward` under torch autograd (the polar split in
               torch, everything with a matrix in it through the HIP autograd bridge), MSE on the sigmoid, torch.optim.Adam over every
               parameter (the centre included), W2_r.weight <- relu - full batch.  This route runs no code the dense fit added.

The routes alternate inside one process: `--warmup` steps each, then `--windows` rounds of (device, autograd) windows, a window =
`--steps` steps between two device events.  Reported per size: the median window of each route in us per step and the spread (max -
min) / median of its windows - two routes whose ratio lies within the spreads do not differ.  One JSON line per size, appended to
--out (default profiles/star_dense_kbench.jsonl).

    python tools/kbench_star_dense.py [--steps 30] [--windows 3] [--warmup 5] [--hidden 130] [--sizes 256x256,480x640]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A
import awesome_amd.star as S


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def image(height, width, dev):
    """Unit-grid rows (x, y) and the unaries (fg = 0) of a five-armed star; no pixel coincides with the initial centre."""
    ii, jj = torch.meshgrid(torch.arange(height), torch.arange(width), indexing="ij")
    x = torch.stack([jj.reshape(-1) / (width - 1), ii.reshape(-1) / (height - 1)], 1).float()
    dx, dy = x[:, 0] - 0.47, x[:, 1] - 0.54
    inside = (dx * dx + dy * dy).sqrt() < 0.27 + 0.09 * torch.cos(5 * torch.atan2(dy, dx))
    return x.to(dev), (1.0 - inside.float()).to(dev)


def bench(args, height, width, dev):
    from awesome_amd.model import StarShapedNet
    torch.manual_seed(0)
    net = StarShapedNet(args.hidden).to(dev)
    with torch.no_grad():
        net.offset.copy_(torch.tensor([[-0.4712, -0.5431]]))
    net.offset.requires_grad_(True)
    x, t = image(height, width, dev)
    start = {k: v.detach().clone() for k, v in net.state_dict().items()}
    spec, flat0 = net.star_spec, net.flat_parameters()

    def device(steps):
        S.star_fit_dense(spec, flat0[None].clone(), x, t[None], steps, lr=1e-2, offset_first_step=0, record_loss=False, want_logits=False)

    def autograd(steps):
        net.load_state_dict(start)
        opt = torch.optim.Adam(net.parameters(), lr=1e-2)
        for _ in range(steps):
            opt.zero_grad()
            loss = ((torch.sigmoid(net(x))[:, 0] - t) ** 2).mean()
            loss.backward()
            opt.step()
            net.enforce_star_shape()

    routes = dict(device=device, autograd=autograd)
    for fn in routes.values():
        fn(args.warmup)
    torch.cuda.synchronize()
    tm = {r: [] for r in routes}
    for _ in range(args.windows):
        for r, fn in routes.items():
            tm[r].append(window(fn, args.steps))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    spread = lambda v: (max(v) - min(v)) / med(v)  # noqa: E731
    out = dict(bench="star_dense_step", net=f"StarShapedNet({args.hidden})", grid=f"{height}x{width}", n_pixels=height * width,
               tile_points=S.dense_tile_points(), steps_per_window=args.steps, windows=args.windows,
               build=A._lib.load().inrfit_build_info().decode()[:40])
    for r in routes:
        out[f"{r}_windows_us"] = [round(v, 1) for v in tm[r]]
        out[f"{r}_us_per_step"] = round(med(tm[r]), 1)
        out[f"{r}_spread"] = round(spread(tm[r]), 3)
    out["autograd_over_device"] = round(med(tm["autograd"]) / med(tm["device"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=130)
    ap.add_argument("--sizes", default="256x256,480x640")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_dense_kbench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measures the MI355X; there is no CPU figure")
    for size in args.sizes.split(","):
        height, width = (int(v) for v in size.split("x"))
        line = json.dumps(bench(args, height, width, torch.device("cuda:0")))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
