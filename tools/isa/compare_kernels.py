#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libinrfit.so kernel by kernel: the set of kernel symbols, each kernel's
disassembly (addresses and branch targets dropped: the order of kernels inside the object moves with the order of template
instantiations) and its tools/kernel_stats.py row.  The check of a host-only change.  No GPU needed.

    python tools/isa/compare_kernels.py OLD.so NEW.so
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_stats as ks  # noqa: E402


def bodies(lib):
    with tempfile.TemporaryDirectory() as d:
        co = ks.extract_code_object(lib, d)
        asm = subprocess.run([ks._tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            t = re.sub(r"\s*//.*$", "", line.strip())                 # the address column
            t = re.sub(r"<[^>]*>", "<label>", t)                      # branch targets by symbol + offset: same after the strip below
            out[name].append(t)
    return out


def main(old, new):
    bo, bn = bodies(old), bodies(new)
    so = {k["name"]: k for k in ks.kernel_stats(old)}
    sn = {k["name"]: k for k in ks.kernel_stats(new)}
    kernels_o = {n for n in bo if n in so}
    kernels_n = {n for n in bn if n in sn}
    print(f"kernels: old {len(kernels_o)}, new {len(kernels_n)}; only old {sorted(kernels_o - kernels_n)}; only new {sorted(kernels_n - kernels_o)}")
    differ_body = sorted(n for n in kernels_o & kernels_n if bo[n] != bn[n])
    differ_row = sorted(n for n in kernels_o & kernels_n if so[n] != sn[n])
    print(f"instructions compared: {sum(len(bo[n]) for n in kernels_o & kernels_n)}")
    print(f"kernels with a differing body: {len(differ_body)} {differ_body}")
    print(f"kernels with a differing kernel_stats row: {len(differ_row)} {differ_row}")
    return 0 if kernels_o == kernels_n and not differ_body and not differ_row else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
