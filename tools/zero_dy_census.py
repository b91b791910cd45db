#!/usr/bin/env python3
"""How much of the headline fit's backward pass multiplies exact zeros: the float32 CPU oracle's loop on bench.py's problem (blob seed
0, 256x256, ConvexNextNet(130, 1) from torch.manual_seed(0), SE, Adam 2e-3, clamp), and every `--every` steps the share of points,
of 16-point wave tiles and of 64-point chunks whose dL/dlogit (torch's autograd, float32) are all exactly zero.  From the chunk map
of icnn_step_kernel (chunk c -> workgroup c % 256) and the measured phase costs of one chunk (profiles/l0_under_dw_ab.txt, section
7: 34.4 k cycles, of which 12.3 k - loop top, forward product, output layer, data term - are needed to know that dy is zero) it
models the chunk-loop time of the slowest and of the mean workgroup under whole-chunk skipping, relative to the dense loop.

CPU only, no kernel of this project runs; the saturation threshold is a property of float32 (sigmoid(y) == 1 from y = 16.64), not of
an exponential's implementation.  About 80 ms per optimizer step on 8 threads.

    python tools/zero_dy_census.py [--steps 2000] [--every 100] [--size 256] [--seed 0]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import inr_oracle as O  # noqa: E402

CHUNK, TILE, WGS = 64, 16, 256
FULL, HEAD = 34.4, 12.3   # k cycles per chunk: all phases; what a skipped chunk still runs


def census(dy):
    n = dy.numel()
    z = (dy == 0).reshape(-1)
    assert n % CHUNK == 0
    tiles = z.reshape(-1, TILE).all(dim=1)
    chunks = z.reshape(-1, CHUNK).all(dim=1)
    cost = torch.where(chunks, torch.tensor(HEAD), torch.tensor(FULL))
    wgs = min(WGS, chunks.numel())
    pad = (-chunks.numel()) % wgs
    per_wg = torch.cat([cost, torch.zeros(pad)]).reshape(-1, wgs).sum(dim=0)      # chunk c -> workgroup c % wgs
    dense = FULL * ((chunks.numel() + wgs - 1) // wgs)
    return (float(z.float().mean()), float(tiles.float().mean()), float(chunks.float().mean()), float(per_wg.max()) / dense,
            float(per_wg.mean()) / dense)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from awesome_amd.dataset import convex_blob_unaries
    from awesome_amd.icnn import IcnnSpec, unpack_params
    from awesome_amd.model import ConvexNextNet
    S = args.size
    torch.manual_seed(args.seed)
    flat = ConvexNextNet(n_hidden=130, in_features=2, n_hidden_layers=1).flat_parameters().detach().cpu()
    p = {k: v.clone().requires_grad_(True) for k, v in unpack_params(IcnnSpec(130, 2, 1), flat).items()}
    grid = O.positional_grid(S, S)[None]
    un = convex_blob_unaries(S, args.seed).reshape(1, 1, S, S).float()
    st = O.AdamState(p)
    print("step  max logit  points  tiles  chunks with every dy == 0 | modelled chunk-loop time: slowest workgroup, mean workgroup")
    shares = []
    for step in range(args.steps):
        for v in p.values():
            v.grad = None
        y = O.icnn_forward_image(p, grid)
        y.retain_grad()
        loss = O.weighted_loss(torch.sigmoid(y), un, "se")
        loss.backward()
        row = census(y.grad)
        shares.append(row[3])
        if step % args.every == 0 or step == args.steps - 1:
            print(f"{step:5d} {float(y.detach().max()):9.1f} {row[0]:7.1%} {row[1]:6.1%} {row[2]:7.1%} | {row[3]:5.2f} {row[4]:5.2f}   loss {float(loss.detach()):.5f}",
                  flush=True)
        O.adam_step(p, {k: v.grad for k, v in p.items()}, st, 2e-3)
        O.icnn_enforce_convexity(p)
    print(f"mean over the {args.steps} steps of the slowest workgroup's modelled chunk-loop time: {sum(shares) / len(shares):.3f} of the dense loop")


if __name__ == "__main__":
    main()
