#!/usr/bin/env python3
"""Time per optimizer step of the sequence pretraining's mini-batch epochs at configs[3]'s shape (C = 3, RealNVP 18 flows x 32 hidden
units, ICNN h = 130 L = 2, T = 16 frames of 128 x 128, batch_size 2: 8 optimizer steps per epoch):

    host_loop    PathConnectedNet.fit_sequence(device_loop=False): one `inrfit_pcn_fit(steps=1)` call per mini-batch behind a gathered
                 copy of the batch, epoch loss and ReduceLROnPlateau in Python (the default path)
    device_loop  fit_sequence(device_loop=True): all epochs in one `inrfit_pcn_fit_sequence` call

The two alternate inside one process: `--warmup` epochs each, then `--windows` rounds of (host window, device window), a window =
`--epochs` epochs between two device events (the host loop's per-epoch read-back of the loss lies inside its window: it is part of
that path).  Reported: the median window of each, their ratio, and the spread (max - min) / median of each side's windows - a ratio
within the spread is no difference.  One JSON line.

    python tools/kbench_sequence.py [--epochs 5] [--windows 3] [--warmup 1] [--size 128] [--frames 16] [--batch-size 2]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A


def window(fn, epochs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(epochs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=2)
    args = ap.parse_args()
    from awesome_amd.dataset import SyntheticSequenceDataset
    from awesome_amd.model import real_nvp_path_connected_net
    dev = torch.device("cuda:0")
    S, T, bs = args.size, args.frames, args.batch_size
    ds = SyntheticSequenceDataset(n_sequences=1, size=S, frames=T)
    coords = ds.coords().reshape(3, T, S * S).permute(1, 0, 2).contiguous().to(dev)
    un = ds.unaries(0).reshape(T, S * S).contiguous().to(dev)
    torch.manual_seed(0)
    m = real_nvp_path_connected_net(channels=3, hidden_units=32, flow_n_flows=18, flow_output_fn="tanh", convex_net_hidden_units=130,
                                    convex_net_hidden_layers=2).to(dev)
    m._actnorm_init_if_needed(coords[:bs].permute(1, 0, 2).reshape(3, -1))
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    steps_per_epoch = (T + bs - 1) // bs

    def run(device_loop):
        def fn(epochs):
            m.load_state_dict(start)
            m.fit_sequence(coords, un, num_epochs=epochs, lr=1e-3, batch_size=bs, device_loop=device_loop)
        return fn

    host, device = run(False), run(True)
    for fn in (host, device):
        fn(args.warmup)
    torch.cuda.synchronize()
    th, td = [], []
    for _ in range(args.windows):
        th.append(window(host, args.epochs) / (args.epochs * steps_per_epoch))
        td.append(window(device, args.epochs) / (args.epochs * steps_per_epoch))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    spread = lambda t: (max(t) - min(t)) / med(t)  # noqa: E731
    out = dict(bench="sequence_step", size=S, frames=T, batch_size=bs, steps_per_epoch=steps_per_epoch, epochs_per_window=args.epochs,
               n_flows=18, flow_hidden=32, n_hidden=130, n_layers=2, build=A._lib.load().inrfit_build_info().decode()[:40],
               host_loop_windows_us=[round(x, 1) for x in th], device_loop_windows_us=[round(x, 1) for x in td],
               host_loop_us_per_step=round(med(th), 1), device_loop_us_per_step=round(med(td), 1),
               host_over_device=round(med(th) / med(td), 3), host_spread=round(spread(th), 3), device_spread=round(spread(td), 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
