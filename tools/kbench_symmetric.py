#!/usr/bin/env python3
"""Time per epoch of the rotation-symmetric teaser's training loop (rotation_symmetric.ipynb cell 3) at the notebook's own shape:
RotationSymmetricNet(150), 500 + 500 random pixels of a 150 x 200 pixel pool per epoch, 2 MSE(bg) + 1 MSE(fg), ONE Adam (1e-3) over
pose and network, the mirror switched on inside the run - on three routes over the same index table:

    device     all epochs in one `inrfit_sym_fit_minibatch` call
    host_loop  per epoch: gather by advanced indexing, an explicit Grid, one `sym_fit(steps=1, step0=k)` call
    autograd   the notebook's loop on the module: pose in torch, forward / backward through the HIP autograd bridge, torch.optim.Adam
               over parameters() (what the module offered before the one call existed)

The routes alternate inside one process: `--warmup` epochs each, then `--windows` rounds of (device, host_loop, autograd) windows, a
window = `--steps` epochs between two device events.  Reported: the median window of each route in us per epoch and the spread (max -
min) / median of its windows - two routes whose ratio lies within the spreads do not differ.  One JSON line, appended to --out
(default profiles/symmetric_kbench.jsonl).

    python tools/kbench_symmetric.py [--steps 40] [--windows 3] [--warmup 5] [--hidden 150]"""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
import awesome_amd as A
import awesome_amd.minibatch as MB
import awesome_amd.symmetric as SY


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def pool(h, w, dev):
    """Pixel centres (no coordinate coincides with the centre) and a likelihood mirror-symmetric about a tilted, off-centre axis."""
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    px = torch.stack([(yy.reshape(-1) + 0.5) / h - 0.5, (xx.reshape(-1) + 0.5) / w - 0.5], 1).float()
    a, b = px[:, 0] - 0.03, px[:, 1] + 0.04
    u, v = a * math.cos(0.4) + b * math.sin(0.4), -a * math.sin(0.4) + b * math.cos(0.4)
    lik = torch.sigmoid((1.0 - ((u / 0.36) ** 2 + ((v.abs() - 0.08) / 0.19) ** 2).sqrt()) * 6.0)
    return px.to(dev), torch.where((lik - 0.5).abs() < 0.02, lik + 0.05, lik).float().to(dev)


def bench(args, dev):
    from awesome_amd.model import RotationSymmetricNet
    torch.manual_seed(0)
    net = RotationSymmetricNet(args.hidden).to(dev)
    pixels, labels = pool(150, 200, dev)
    number, total = args.number, args.warmup + args.steps
    switch = args.steps // 2   # the mirror comes on halfway through a window
    table = MB.class_balanced_batches(labels.cpu(), total, number, torch.Generator().manual_seed(1)).to(dev)
    co, tg = pixels.t().contiguous(), labels[None].contiguous()
    start = {k: v.detach().clone() for k, v in net.state_dict().items()}
    flat0, pose0 = net.flat_parameters().to(dev), net._pose().to(dev)
    kw = dict(lr=1e-3, loss="se", weight_mode="explicit", c_fg=2.0 / number, c_bg=1.0 / number, symmetry_from_step=switch,
              record_loss=False)

    def device(steps):
        SY.sym_fit_minibatch(net.spec, flat0[None].clone(), pose0[None].clone(), co, tg, table[:steps], **kw)

    def host_loop(steps):
        flat, pose, so, sp = flat0[None].clone(), pose0[None].clone(), None, None
        for k in range(steps):
            idx = table[k].long()
            r = SY.sym_fit(net.spec, flat, pose, A.Grid.explicit(co[:, idx]), tg[:, idx], 1, opt_state=so, pose_opt_state=sp, step0=k, **kw)
            so, sp = r.opt_state, r.pose_opt_state

    def autograd(steps):
        net.load_state_dict(start)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        for k in range(steps):
            idx = table[k].long()
            opt.zero_grad()
            out = torch.sigmoid(net(pixels[idx], k >= switch))[:, 0]
            t = labels[idx]
            loss = 2.0 * F.mse_loss(out[:number], t[:number]) + 1.0 * F.mse_loss(out[number:], t[number:])
            loss.backward()
            opt.step()

    routes = dict(device=device, host_loop=host_loop, autograd=autograd)
    for fn in routes.values():
        fn(args.warmup)
    torch.cuda.synchronize()
    t = {r: [] for r in routes}
    for _ in range(args.windows):
        for r, fn in routes.items():
            t[r].append(window(fn, args.steps))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    spread = lambda v: (max(v) - min(v)) / med(v)  # noqa: E731
    out = dict(bench="symmetric_epoch", net=f"RotationSymmetricNet({args.hidden})", n_pool=int(pixels.shape[0]), batch=int(table.shape[1]),
               steps_per_window=args.steps, windows=args.windows, build=A._lib.load().inrfit_build_info().decode()[:40])
    for r in routes:
        out[f"{r}_windows_us"] = [round(x, 1) for x in t[r]]
        out[f"{r}_us_per_epoch"] = round(med(t[r]), 1)
        out[f"{r}_spread"] = round(spread(t[r]), 3)
    out["host_over_device"] = round(med(t["host_loop"]) / med(t["device"]), 3)
    out["autograd_over_device"] = round(med(t["autograd"]) / med(t["device"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=150)
    ap.add_argument("--number", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symmetric_kbench.jsonl"))
    args = ap.parse_args()
    line = json.dumps(bench(args, torch.device("cuda:0")))
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
