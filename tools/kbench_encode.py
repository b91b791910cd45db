#!/usr/bin/env python3
"""Steady-state optimizer-step time of the layer-by-layer path at 256 x 256: the Fourier-feature notebook shape (2 -> 20 cos features ->
3 x 350 relu -> 3 outputs, frozen features, Adam) next to the ICNN shapes of tools/kbench_wide.py, measured in the same process.

Each shape: a warm-up fit, then `--windows` fits of `--steps` steps each between two device events (a window of >= 1 s at ~1 ms per
step); the median window is reported.  One JSON line per shape with the FLOP count of a step (kept here), TFLOP/s and the share of the
fp32 MFMA peak, and a checksum of the fitted parameters (same library, same inputs -> same bits: the A/B of two builds compares it).

    python tools/kbench_encode.py [--steps 1000] [--windows 3] [--shapes encode,256x1,350x3]
Run it once per build (INRFIT_LIB=... INRFIT_ABI_ANY=1 for another library; an ABI-7 build has no general shapes: leave `encode` out)."""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import awesome_amd as A
from awesome_amd.dataset import convex_blob_unaries

PEAK = 157.3   # TFLOP/s, fp32 MFMA (v_mfma_f32_16x16x4_f32) of the MI355X


def step_flop(h, L, F, O, C=2, frozen_input=True, N=65536):
    """Multiply-adds x 2 of one optimizer step: forward (layer 0, the hidden GEMMs, the head), backward (weight gradients of every
    layer, dZ of every layer above layer 0 - dZ_0 is skipped with frozen features - and the head's dZ_L / output-layer gradient)."""
    fwd = F * C + (h * F + (L - 1) * h * h if L > 0 else 0) + O * (h if L > 0 else F)
    dw = (h * F + (L - 1) * h * h if L > 0 else 0) + O * (h if L > 0 else F)
    dz = ((L - 1) * h * h if L > 0 else 0) + O * (h if L > 0 else F) + (0 if frozen_input or L == 0 else h * F)
    return 2.0 * N * (fwd + dw + dz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--shapes", default="encode,256x1,350x3")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    S = 256
    g = A.Grid.linspace(S, S, dev)
    for name in args.shapes.split(","):
        if name == "encode":
            h, L, F, O = 350, 3, 20, 3
            spec = A.IcnnSpec(h, 2, L, act0="cos", n_features=F, n_out=O)
            torch.manual_seed(0)
            p = {k: (torch.rand(s) - 0.45) * (0.6 / h ** 0.5) for k, s in spec.keys_shapes()}
            p["input.weight"] = 30.0 * torch.randn(F, 2)
            p["input.bias"] = torch.randn(F)
            xs = torch.linspace(0, 1, S)
            yy, xx = torch.meshgrid(xs, xs, indexing="ij")
            tgt = torch.stack([xx, 1 - yy, ((xx - 0.5) ** 2 + (yy - 0.5) ** 2).sqrt()], 0).reshape(1, 3, -1).to(dev)
            kw = dict(clamp=False, freeze_skips=True, freeze_input=True, lr=1e-3)
            flop = step_flop(h, L, F, O)
        else:
            h, L = (int(v) for v in name.split("x"))
            spec = A.IcnnSpec(h, 2, L)
            torch.manual_seed(0)
            p = {k: (torch.rand(s) - 0.45) * (0.6 / h ** 0.5) for k, s in spec.keys_shapes()}
            tgt = convex_blob_unaries(S, 0).reshape(1, -1).to(dev)
            kw = dict(lr=2e-3)
            flop = 3 * (2 * h * 2 + L * (2 * h * h + 2 * h * 2) + 2 * h + 4) * 65536.0   # kbench_wide.py's count: 3 x the forward
        flat = A.pack_state_dict(spec, p, dev)[None].contiguous()
        A.fit(spec, flat.clone(), g, tgt, 20, record_loss=False, want_logits=False, **kw)   # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(args.windows):
            w = flat.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = A.fit(spec, w, g, tgt, args.steps, record_loss=True, want_logits=False, **kw)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        dt = sorted(times)[len(times) // 2] / args.steps
        ck = hashlib.sha256(w.cpu().numpy().tobytes()).hexdigest()[:16]
        print(json.dumps(dict(shape=name, h=h, L=L, n_features=spec.features, n_out=spec.n_out, steps=args.steps, window_s=round(sorted(times)[len(times) // 2], 3),
                              us_per_step=round(dt * 1e6, 1), flop_per_step=flop, tflops=round(flop / dt / 1e12, 2),
                              share_of_peak=round(flop / dt / 1e12 / PEAK, 3), loss_first=float(r.loss_hist[0, 0]),
                              loss_last=float(r.loss_hist[0, -1]), params_sha=ck, build=A._lib.load().inrfit_build_info().decode()[:40])), flush=True)


if __name__ == "__main__":
    main()
