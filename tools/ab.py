#!/usr/bin/env python3
"""A/B of library builds on one box: `python tools/ab.py main nosgb ...` runs tools/kbench.py once per build (INRFIT_LIB), each in
its own process; "main" = the shipped awesome_amd/csrc/libinrfit.so, anything else = variants/libinrfit_<name>.so.
`--bench`: bench.py (default arguments, the headline fit) instead of kbench.py, one line of ms_per_step / fit_checksum per run, and at
the end every build's range and median; `--reps N`: N alternating rounds (default 2)."""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
reps, bench = 2, "--bench" in argv
if "--reps" in argv:
    i = argv.index("--reps")
    reps = int(argv[i + 1])
    del argv[i:i + 2]
extra = [a for a in argv if a.startswith("--") and a != "--bench"]
names = [a for a in argv if not a.startswith("--")] or ["main"]
ms = {n: [] for n in names}
for rep in range(reps):
    for n in names:
        env = dict(os.environ)
        if n != "main":
            env["INRFIT_LIB"] = os.path.join(ROOT, "variants", f"libinrfit_{n}.so")
            env["INRFIT_ABI_ANY"] = "1"
        if bench:
            cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + extra
        else:
            cmd = [sys.executable, os.path.join(ROOT, "tools", "kbench.py"), "--sizes", "256", "--images", "1", "64", "--fit-steps", "1000"] + extra
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)   # (a hung run ends the A/B)
        for line in out.stdout.splitlines():
            if bench and line.startswith("{"):
                r = json.loads(line)
                ms[n].append(r["ms_per_step"])
                print(f"[{n:10s}] ms_per_step {r['ms_per_step']:9.3f}  value {r['value']}  fit_checksum {r.get('fit_checksum')}", flush=True)
            elif line.startswith("size"):
                print(f"[{n:10s}] {line}", flush=True)
        if out.returncode:
            print(out.stderr[-800:])
            sys.exit(out.returncode)   # (nothing more is started on the GPU after a failed run)
if bench:
    for n in names:
        v = ms[n]
        print(f"[{n:10s}] ms_per_step min {min(v):.3f} median {statistics.median(v):.3f} max {max(v):.3f} (range {max(v) - min(v):.3f}, {len(v)} runs)")
