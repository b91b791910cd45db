#!/usr/bin/env python3
"""Time per optimizer step of the teaser notebooks' pixel-minibatch loops, at the notebooks' own nets and batch sizes:

    convex     ConvexNet(n_hidden=150)                       2000 + 2000 pixels, MSE(bg) + MSE(fg), Adam 1e-2, clamp
    repeating  SineLayerNet(200, n_hidden_layers=0)          500 + 500 pixels, 2 MSE(bg) + 1 MSE(fg)
    fourier    FourierFeatureNet(2 -> 20 -> 3 x 350 -> 3)    DataLoader(batch_size=64, shuffle=True) steps over 2500 pixels: 39 x 64 + 4
    diffeo     ConvexDiffeomorphismNet() (K 4, W 70, 130x1)  1000 + 1000 pixels, 2 BCE(bg) + 1 BCE(fg), Adam over everything

on three routes over the same index table:

    device     all steps in one `inrfit_fit_minibatch` / `inrfit_cdn_fit_minibatch` call
    host_loop  per step: gather by advanced indexing, an explicit Grid, one `fit(steps=1, step0=k)` call
    autograd   the notebook's loop on the module: forward / backward through the HIP autograd bridges, torch.optim.Adam, the projection

The routes alternate inside one process: `--warmup` steps each, then `--windows` rounds of (device, host_loop, autograd) windows, a
window = `--steps` optimizer steps between two device events.  Reported per shape: the median window of each route in us per step and
the spread (max - min) / median of its windows - two routes whose ratio lies within the spreads do not differ.  One JSON line per
shape, appended to --out (default profiles/minibatch_kbench.jsonl).

    python tools/kbench_minibatch.py [--steps 40] [--windows 3] [--warmup 5] [--shapes convex,repeating,fourier,diffeo]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
import awesome_amd as A
import awesome_amd.flow as FL
import awesome_amd.minibatch as MB


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def pool(side, dev, channels=1):
    yy, xx = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
    px = torch.stack([yy.reshape(-1) / side - 0.5, xx.reshape(-1) / side - 0.5], 1).float()
    liks = []
    for ch in range(channels):
        d = ((px[:, 0] - 0.05 * ch) ** 2 + (px[:, 1] + 0.04 * ch) ** 2).sqrt()
        lik = torch.sigmoid((d - 0.3 + 0.03 * ch) * 12.0)
        liks.append(torch.where((lik - 0.5).abs() < 0.02, lik + 0.05, lik))
    return px.to(dev), torch.stack(liks, 1).float().to(dev)   # (N, 2), (N, channels)


def shapes(dev):
    from awesome_amd.model import ConvexDiffeomorphismNet, ConvexNet, FourierFeatureNet, SineLayerNet
    torch.manual_seed(0)
    return {
        "convex": dict(net=ConvexNet(n_hidden=150), side=128, number=2000, weights=(1.0, 1.0), loss="se", lr=1e-2),
        "repeating": dict(net=SineLayerNet(in_features=2, n_hidden=200, n_hidden_layers=0), side=128, number=500, weights=(2.0, 1.0),
                          loss="se", lr=1e-2),
        "fourier": dict(net=FourierFeatureNet(d_in=2, n_hidden=350, n_hidden_layers=3, factor=30.0, d_features=20, d_out=3), side=50,
                        batch_size=64, loss="se", lr=1e-3, channels=3),
        "diffeo": dict(net=ConvexDiffeomorphismNet(), side=128, number=1000, weights=(2.0, 1.0), loss="bce", lr=1e-2),
    }


def bench(name, s, args, dev):
    net = s["net"].to(dev)
    flow = hasattr(net, "diffeo_net")
    pixels, labels = pool(s["side"], dev, s.get("channels", 1))
    n_pool, number = pixels.shape[0], s.get("number")
    total = args.warmup + args.steps
    gen = torch.Generator().manual_seed(1)
    if number:
        table, counts = MB.class_balanced_batches(labels[:, 0].cpu(), total, number, gen).to(dev), None
        w_bg, w_fg = s["weights"]
        kw = dict(weight_mode="explicit", c_fg=w_bg / number, c_bg=w_fg / number)
    else:
        epochs = -(-total // -(-n_pool // s["batch_size"]))
        table, counts = MB.dataloader_batches(n_pool, s["batch_size"], epochs, gen)
        table, counts, kw = table[:total].to(dev), counts[:total].tolist(), dict(weight_mode="none")
    co = pixels.t().contiguous()
    tg = labels.t().contiguous()[None] if labels.shape[1] > 1 else labels.t().contiguous()
    start = {k: v.detach().clone() for k, v in net.state_dict().items()}
    if flow:
        ispec, fspec = net._specs()
        ip0, fp0 = FL.split_cdn_state_dict(ispec, fspec, net.state_dict(), dev)
        kw.update(lr=s["lr"], loss=s["loss"], clamp=False, weight_decay_on_weight_g=0.0)
    else:
        ispec, flat0 = net.spec, net.flat_parameters().to(dev)
        kw.update(lr=s["lr"], loss=s["loss"], optimizer="adam", **dict(getattr(net, "fit_options", None) or dict(clamp=True)))

    def device(steps):
        cn = counts[:steps] if counts is not None else None
        if flow:
            MB.cdn_fit_minibatch(ispec, fspec, ip0[None].clone(), fp0[None].clone(), co, tg, table[:steps], cn, record_loss=False, **kw)
        else:
            MB.fit_minibatch(ispec, flat0[None].clone(), co, tg, table[:steps], cn, record_loss=False, **kw)

    def host_loop(steps):
        if flow:
            ip, fp, so, sf = ip0[None].clone(), fp0[None].clone(), None, None
        else:
            flat, so = flat0[None].clone(), None
        for k in range(steps):
            idx = table[k, :counts[k]].long() if counts is not None else table[k].long()
            grid, t = A.Grid.explicit(co[:, idx]), tg[..., idx]
            if flow:
                r = FL.cdn_fit(ispec, fspec, ip, fp, grid, t, 1, icnn_opt_state=so, flow_opt_state=sf, step0=k, record_loss=False,
                               want_logits=False, **kw)
                so, sf = r.icnn_opt_state, r.flow_opt_state
            else:
                so = A.fit(ispec, flat, grid, t, 1, opt_state=so, step0=k, record_loss=False, want_logits=False, **kw).opt_state

    def autograd(steps):
        net.load_state_dict(start)
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=s["lr"])
        crit = F.mse_loss if s["loss"] == "se" else F.binary_cross_entropy
        for k in range(steps):
            idx = table[k, :counts[k]].long() if counts is not None else table[k].long()
            opt.zero_grad()
            out = torch.sigmoid(net(pixels[idx]))
            t = labels[idx]
            if number:
                loss = s["weights"][0] * crit(out[:number], t[:number]) + s["weights"][1] * crit(out[number:], t[number:])
            else:
                loss = crit(out, t)
            loss.backward()
            opt.step()
            net.enforce_convexity()

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
    out = dict(bench="minibatch_step", shape=name, net=type(net).__name__, n_pool=n_pool,
               batch=int(table.shape[1]), steps_per_window=args.steps, windows=args.windows,
               build=A._lib.load().inrfit_build_info().decode()[:40])
    for r in routes:
        out[f"{r}_windows_us"] = [round(x, 1) for x in t[r]]
        out[f"{r}_us_per_step"] = round(med(t[r]), 1)
        out[f"{r}_spread"] = round(spread(t[r]), 3)
    out["host_over_device"] = round(med(t["host_loop"]) / med(t["device"]), 3)
    out["autograd_over_device"] = round(med(t["autograd"]) / med(t["device"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="convex,repeating,fourier,diffeo")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minibatch_kbench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    all_shapes = shapes(dev)
    for name in args.shapes.split(","):
        line = json.dumps(bench(name, all_shapes[name], args, dev))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
