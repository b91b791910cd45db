#!/usr/bin/env python3
"""The sequence of kernel launches of a `rocprofv3 --kernel-trace --output-format csv` run, one line per dispatch in dispatch order:
kernel name, grid, workgroup and LDS size.  Two runs of one script under two builds of the library launch the same kernels in the same
order with the same shapes exactly when these listings are equal (`diff`).

    rocprofv3 --kernel-trace --output-format csv -d out -o run -- python tools/driver_hashes.py
    python tools/kernel_sequence.py out > run.seq
"""
import csv
import glob
import os
import sys


def main(root):
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"no *kernel_trace.csv under {root}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    key = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    cols = [c for c in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z",
                        "LDS_Block_Size", "Scratch_Size") if c in rows[0]]
    for r in rows:
        print(r["Kernel_Name"], *[r[c] for c in cols])


if __name__ == "__main__":
    main(sys.argv[1])
