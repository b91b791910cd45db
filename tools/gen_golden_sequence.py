"""Fixture of tests/test_sequence_host.py: the reference CLASS's `PathConnectedNet.create_normalized_grid`
(awesome/model/path_connected_net.py:252-296) on small shapes -> tests/golden/normalized_grid_reference.npz (recorded in
tests/golden/PROVENANCE_sequence.txt).

Same recipe as tools/gen_golden_boundary.py: the reference's modules import `toml`, `jsonpickle` and `simple_parsing`, which are not
installed here and take no part in the recorded arithmetic; they are replaced in this process by that file's inert module objects.
Every number written comes out of the reference's own code.  Nothing in the product imports this file; the reference never travels.

Usage:  python tools/gen_golden_sequence.py [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import REF  # noqa: E402
from gen_golden_boundary import _install_inert_modules  # noqa: E402

SHAPES = {"thw_5_7_9": (5, 7, 9), "thw_4_8_10": (4, 8, 10), "thw_2_3_2": (2, 3, 2), "hw_6_5": (6, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    args = ap.parse_args()
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not present; fixtures can only be generated in the build container")
    _install_inert_modules()
    sys.path.insert(0, REF)
    for sub in ("model", "dataset"):  # skip the eager package __init__ files (they pull cv2 / torchvision)
        pkg = types.ModuleType(f"awesome.{sub}")
        pkg.__path__ = [os.path.join(REF, "awesome", sub)]
        sys.modules[f"awesome.{sub}"] = pkg
    from awesome.model.path_connected_net import PathConnectedNet
    out = {k: PathConnectedNet.create_normalized_grid(shp).numpy() for k, shp in SHAPES.items()}
    path = os.path.join(args.out, "normalized_grid_reference.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
