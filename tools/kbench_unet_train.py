#!/usr/bin/env python3
"""Time of one UNet training step (training-mode forward, then backward from a fixed dlogits): the HIP route
(awesome_amd.unet.unet_train_forward) against the same module's torch modules in train() mode, same weights, in_chn 4, base_width 64
(the reference's network), at 256 x 256 and 480 x 640.

Method: 5 warm-up steps, then 50 timed steps between two stream synchronisations (host clock), each side; one JSON line per shape is
appended to profiles/unet_train_kbench.jsonl (`--out`), with the workspace bytes of the HIP step and the largest difference between
the two sides' logits and gradients.

    python tools/kbench_unet_train.py [--shapes 256x256,480x640] [--warmup 5] [--calls 50] [--out profiles/unet_train_kbench.jsonl]

The split by kernel family comes from a kernel trace of the HIP route alone:

    rocprofv3 --kernel-trace --stats -d DIR -o unet_train -- python tools/kbench_unet_train.py --trace-run --shapes 480x640
    python tools/kbench_unet_train.py --split-from DIR --shapes 480x640

`--trace-run` runs 2 warm-up and 3 traced steps of one shape and nothing else; `--split-from` reads the dispatches back, keeps the
library's kernels and adds them up per family (one more JSON line, times per step)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

IN_CHN, BASE = 4, 64
TRACE_WARMUP, TRACE_PASSES = 2, 3
# kernel family <- substrings of the kernel's name (first match)
FAMILIES = [("gather", ("unet_tgather_kernel", "unet_gather_kernel")), ("product", ("gemm_kernel",)), ("slice_sum", ("gemm_splitk_sum_kernel",)),
            ("dw_reduce", ("unet_dw_reduce_kernel",)), ("batch_stats", ("unet_stats_kernel",)),
            ("bn_backward", ("unet_bn_sums_kernel", "unet_bn_dy_kernel")), ("reader_backward", ("unet_pool_bwd_kernel", "unet_up_bwd_kernel")),
            ("pack", ("unet_pack_kernel", "unet_wt_pack_kernel")), ("outconv", ("unet_tout_kernel", "unet_out_bwd_kernel", "unet_out_dw_kernel"))]


def make(dev, h, w):
    import torch
    from awesome_amd.model import UNet
    torch.manual_seed(0)
    net = UNet(in_chn=IN_CHN).to(dev).train()
    g = torch.Generator().manual_seed(1)
    return (net, torch.rand(1, 3, h, w, generator=g).to(dev), torch.rand(1, 1, h, w, generator=g).to(dev),
            (torch.randn(1, 1, h, w, generator=g) / (h * w)).to(dev))


def step(net, image, feat, dlogits, hip):
    from awesome_amd.unet import unet_train_forward
    for p in net.parameters():
        p.grad = None
    out = unet_train_forward(net, image, feat) if hip else net.forward_torch(image, feat)
    out.backward(dlogits)
    return out


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
    import copy
    import torch
    import awesome_amd as A
    from awesome_amd.unet import make_desc
    dev = torch.device("cuda:0")
    lib = A._lib.load()
    build = lib.inrfit_build_info().decode()[:40]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for h, w in shapes:
        net, image, feat, dlogits = make(dev, h, w)
        twin = copy.deepcopy(net)
        # one step each from the same state: how far the two sides are apart
        a, b = step(net, image, feat, dlogits, True), step(twin, image, feat, dlogits, False)
        dlog = float((a.detach() - b.detach()).abs().max())
        dgrad = max(float((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30)) for p, q in zip(net.parameters(), twin.parameters())
                    if p.dim() == 4)
        torch.cuda.reset_peak_memory_stats(dev)
        hip_ms, _ = timed(lambda: step(net, image, feat, dlogits, True), args.warmup, args.calls)
        hip_peak = torch.cuda.max_memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        torch_ms, _ = timed(lambda: step(twin, image, feat, dlogits, False), args.warmup, args.calls)
        torch_peak = torch.cuda.max_memory_allocated(dev)
        desc = make_desc(net, h, w)
        r = dict(bench="unet_train_step", height=h, width=w, in_chn=IN_CHN, base_width=BASE, warmup=args.warmup, calls=args.calls,
                 hip_ms=round(hip_ms, 3), torch_ms=round(torch_ms, 3), hip_over_torch=round(hip_ms / torch_ms, 3),
                 workspace_bytes=int(lib.inrfit_unet_train_workspace_bytes(C.byref(desc))), hip_peak_allocated_bytes=int(hip_peak),
                 torch_peak_allocated_bytes=int(torch_peak), max_abs_diff_logits=dlog, max_rel_diff_weight_grads=dgrad, build=build)
        line = json.dumps(r)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def trace_run(shapes):
    import torch
    dev = torch.device("cuda:0")
    h, w = shapes[0]
    net, image, feat, dlogits = make(dev, h, w)
    for _ in range(TRACE_WARMUP + TRACE_PASSES):
        step(net, image, feat, dlogits, True)
    torch.cuda.synchronize()


def split(args, shapes):
    from kbench_unet import dispatches
    h, w = shapes[0]
    acc, count = {}, {}
    for name, ns in dispatches(args.split_from):
        fam = next((f for f, keys in FAMILIES if any(k in name for k in keys)), None)
        if fam is None:
            continue
        acc[fam] = acc.get(fam, 0) + ns
        count[fam] = count.get(fam, 0) + 1
    passes = TRACE_WARMUP + TRACE_PASSES      # every step launches the same kernels: the average over all of them
    total = sum(acc.values())
    r = dict(bench="unet_train_split", height=h, width=w, kernel_ms_per_step=round(total / passes / 1e6, 3),
             launches_per_step=sum(count.values()) // passes, **{f"{k}_ms": round(v / passes / 1e6, 3) for k, v in acc.items()})
    line = json.dumps(r)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,480x640")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_train_kbench.jsonl"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--split-from", default=None)
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
