#!/usr/bin/env python3
"""Time of the UNet's evaluation pass: the HIP route (awesome_amd.unet.unet_forward) against the same module's torch modules, same
weights, eval() under no_grad, in_chn 4, base_width 64 (the reference's network), at 256 x 256 and 480 x 640.

Method: 20 warm-up calls, then 100 timed calls between two stream synchronisations (host clock), each side; one JSON line per shape
is appended to profiles/unet_kbench.jsonl (`--out`), with the largest difference between the two outputs.

    python tools/kbench_unet.py [--shapes 256x256,480x640] [--warmup 20] [--calls 100] [--out profiles/unet_kbench.jsonl]

The split by layer comes from a kernel trace of the HIP route alone:

    rocprofv3 --kernel-trace --stats -d DIR -o unet -- python tools/kbench_unet.py --trace-run --shapes 480x640
    python tools/kbench_unet.py --split-from DIR --shapes 480x640 --split-out profiles/unet_layer_split_480x640.csv

`--trace-run` runs 3 warm-up and 5 traced passes of one shape and nothing else; `--split-from` reads the dispatches back (rocpd
database or kernel-trace csv), keeps the library's kernels of the last 5 passes in launch order and charges each to its convolution:
the launch sequence of a pass is fixed by the shape (per convolution and strip: gather, product, and the slice sum of a split
product; OutConv last), and is rebuilt here from the same rules as csrc/unet.h."""
import argparse
import csv
import glob
import json
import os
import sqlite3
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IN_CHN, BASE = 4, 64
STRIP, SPLITK_TILES, SPLITK_MIN_K = 2048, 64, 2048          # csrc/unet.h
NAMES = ["inc.0", "inc.3"] + [f"down{i}.{j}" for i in range(1, 5) for j in (0, 3)] + [f"up{i}.{j}" for i in range(1, 5) for j in (0, 3)]
TRACE_WARMUP, TRACE_PASSES = 3, 5


def launch_plan(h, w, in_chn=IN_CHN, b=BASE, strip=STRIP):
    """[(layer name, kind)] of one pass in launch order; kind: gather / product / slice_sum / out."""
    down, up = [b, 2 * b, 4 * b, 8 * b, 8 * b], [4 * b, 2 * b, b, b]
    H, W = [h], [w]
    for _ in range(4):
        H.append(H[-1] // 2)
        W.append(W[-1] // 2)
    convs = [(in_chn, b, 0), (b, b, 0)]
    for l in range(1, 5):
        convs += [(down[l - 1], down[l], l), (down[l], down[l], l)]
    deep = down[4]
    for u in range(4):
        l = 3 - u
        convs += [(down[l] + deep, up[u], l), (up[u], up[u], l)]
        deep = up[u]
    seq = []
    for name, (cin, cout, l) in zip(NAMES, convs):
        hw = H[l] * W[l]
        hwp, kp = (hw + 3) // 4 * 4, (9 * cin + 1 + 15) // 16 * 16
        tiles = ((cout + 127) // 128) * ((hwp + 127) // 128)
        split = hwp <= strip and tiles <= SPLITK_TILES and kp >= SPLITK_MIN_K
        for _ in range(0, hw, strip):
            seq += [(name, "gather"), (name, "product")] + ([(name, "slice_sum")] if split else [])
    return seq + [("outc", "out")]


def make(dev, h, w):
    import torch
    from awesome_amd.model import UNet
    torch.manual_seed(0)
    net = UNet(in_chn=IN_CHN).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    return net, torch.rand(1, 3, h, w, generator=g).to(dev), torch.rand(1, 1, h, w, generator=g).to(dev)


def timed(fn, warmup, calls):
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, out


def bench(args, shapes):
    import torch
    import awesome_amd as A
    from awesome_amd.unet import unet_forward
    dev = torch.device("cuda:0")
    build = A._lib.load().inrfit_build_info().decode()[:40]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for h, w in shapes:
        net, image, feat = make(dev, h, w)
        with torch.no_grad():
            hip_ms, hip = timed(lambda: unet_forward(net, image, feat), args.warmup, args.calls)
            torch_ms, ref = timed(lambda: net.forward_torch(image, feat), args.warmup, args.calls)
        r = dict(bench="unet_eval", height=h, width=w, in_chn=IN_CHN, base_width=BASE, warmup=args.warmup, calls=args.calls,
                 hip_ms=round(hip_ms, 3), torch_ms=round(torch_ms, 3), hip_over_torch=round(hip_ms / torch_ms, 3),
                 max_abs_diff=float((hip - ref).abs().max()), max_abs_out=float(ref.abs().max()), launches_per_pass=len(launch_plan(h, w)),
                 build=build)
        line = json.dumps(r)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def trace_run(shapes):
    import torch
    from awesome_amd.unet import unet_forward
    dev = torch.device("cuda:0")
    h, w = shapes[0]
    net, image, feat = make(dev, h, w)
    with torch.no_grad():
        for _ in range(TRACE_WARMUP + TRACE_PASSES):
            unet_forward(net, image, feat)
    torch.cuda.synchronize()


def dispatches(directory):
    """[(kernel name, ns)] in launch order, from the rocpd database or the kernel-trace csv below `directory`."""
    dbs = glob.glob(os.path.join(directory, "**", "*.db"), recursive=True)
    if dbs:
        rows = list(sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start"))
        return [(n, e - s) for n, s, e in rows]
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no rocpd database and no kernel-trace csv below {directory}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows]


def split(args, shapes):
    h, w = shapes[0]
    plan = launch_plan(h, w)
    own = [(n, t) for n, t in dispatches(args.split_from)
           if any(k in n for k in ("unet_gather_kernel", "unet_out_kernel", "gemm_kernel", "gemm_splitk_sum_kernel"))]
    need = len(plan) * TRACE_PASSES
    if len(own) < need:
        raise SystemExit(f"{len(own)} dispatches of the library's kernels in the trace, {need} expected for {TRACE_PASSES} passes")
    own = own[-need:]
    want = {"gather": "unet_gather_kernel", "product": "gemm_kernel", "slice_sum": "gemm_splitk_sum_kernel", "out": "unet_out_kernel"}
    acc = {}
    for i, (name, ns) in enumerate(own):
        layer, kind = plan[i % len(plan)]
        if want[kind] not in name:
            raise SystemExit(f"dispatch {i} is {name}, the launch plan expects a {kind} of {layer}")
        acc[(layer, kind)] = acc.get((layer, kind), 0) + ns
    total = sum(acc.values())
    rows = [("layer", "gather_us", "product_us", "slice_sum_us", "out_us", "share_percent")]
    for layer in NAMES + ["outc"]:
        us = [acc.get((layer, k), 0) / TRACE_PASSES / 1e3 for k in ("gather", "product", "slice_sum", "out")]
        rows.append((layer, *[f"{v:.1f}" for v in us], f"{100.0 * sum(us) * 1e3 * TRACE_PASSES / total:.1f}"))
    kinds = {k: sum(v for (_, kk), v in acc.items() if kk == k) / TRACE_PASSES / 1e3 for k in want}
    rows.append(("all", *[f"{kinds[k]:.1f}" for k in ("gather", "product", "slice_sum", "out")], "100.0"))
    out = open(args.split_out, "w", newline="") if args.split_out else sys.stdout
    csv.writer(out).writerows(rows)
    print(json.dumps(dict(bench="unet_eval_split", height=h, width=w, kernel_ms_per_pass=round(total / TRACE_PASSES / 1e6, 3),
                          **{f"{k}_ms": round(v / 1e3, 3) for k, v in kinds.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,480x640")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_kbench.jsonl"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--split-from", default=None)
    ap.add_argument("--split-out", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.split_from:
        split(args, shapes)
    elif args.trace_run:
        trace_run(shapes)
    else:
        bench(args, shapes)


if __name__ == "__main__":
    main()
