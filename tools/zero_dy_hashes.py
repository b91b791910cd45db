#!/usr/bin/env python3
"""One SHA-256 per output tensor of the L = 1 step kernel on inputs with exactly-zero dL/dlogit - the cases of
tests/step_zero_dy_cases.py: natural saturation (se, bce), the zero patterns through the vector-Jacobian product with and without
dcoords, the NaN case and the 25-step trajectory - at the tests' launches (slab base set by hand).  tools/driver_hashes.py has no
saturated input; this is its complement for builds that differ in how such chunks are treated.  Two builds that print the same lines
compute the same bits:

    INRFIT_LIB=old/libinrfit.so INRFIT_ABI_ANY=1 python tools/zero_dy_hashes.py > old.txt
    python tools/zero_dy_hashes.py > new.txt && diff old.txt new.txt
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import awesome_amd as A  # noqa: E402
from driver_hashes import show  # noqa: E402
from tests import step_l0_cases as Z  # noqa: E402
from tests import step_zero_dy_cases as Y  # noqa: E402


def main():
    lib = A._lib.load()
    dev = torch.device("cuda:0")

    def inputs(c):
        return A.pack_state_dict(c["spec"], c["p"], dev)[None].contiguous(), A.Grid.explicit(c["coords"].to(dev))

    def at(name):
        assert lib.inrfit_debug_set_slab_base(Z.LAUNCHES[name][0]) == 0

    for h, C in Y.SHAPES:
        for name in Y.SAT_LAUNCHES:
            c = Y.sat_case(h, C, name)
            flat, grid = inputs(c)
            at(name)
            for kind in ("se", "bce"):
                lo, gr = A.loss_grad(c["spec"], flat, grid, (c["un_bce"] if kind == "bce" else c["un"])[None].to(dev), loss=kind)
                show(f"sat h{h} C{C} {name} {kind}", loss=lo, grads=gr)
        for name, pattern in Y.PATTERNS:
            c = Y.pattern_case(h, C, name, pattern)
            flat, grid = inputs(c)
            at(name)
            show(f"pattern h{h} C{C} {name} {pattern}", grads=A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev)))
            gr, dco = A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev), want_dcoords=True)
            show(f"pattern h{h} C{C} {name} {pattern} dx", grads=gr, dcoords=dco)
    c = Y.nan_case()
    flat, grid = inputs(c)
    at("three_each")
    lo, gr = A.loss_grad(c["spec"], flat, grid, c["un"][None].to(dev), loss="se")
    show("nan", loss=lo, grads=gr)
    c = Y.traj_case()
    flat, grid = inputs(c)
    r = A.fit(c["spec"], flat.clone(), grid, c["hard"][None].to(dev), Y.TRAJ_STEPS, lr=2e-3, want_logits=True)
    show("trajectory", params=r.params, opt=r.opt_state, hist=r.loss_hist, logits=r.logits, status=r.status)
    lib.inrfit_debug_set_slab_base(0)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
