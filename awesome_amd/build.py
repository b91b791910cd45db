"""Build libinrfit.so (hipcc, gfx950) in-tree.  `python -m awesome_amd.build`."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "csrc", "inrfit.hip")
OUT = os.path.join(HERE, "csrc", "libinrfit.so")
INCLUDE = os.path.join(ROOT, "include")
MAP = os.path.join(HERE, "csrc", "inrfit.map")


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def needs_build(out: str = OUT) -> bool:
    if not os.path.exists(out):
        return True
    deps = [SRC, MAP, os.path.join(INCLUDE, "inrfit.h")] + [os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc")) if f.endswith(".h")]
    return any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build(force: bool = False, verbose: bool = True, out: str = OUT, extra_flags=()) -> str:
    """Compile the HIP C-ABI library for gfx950.  Cross-compiles without a GPU.  `out` / `extra_flags`: an A/B or stamps variant
    (tools/build_variant.sh), compiled exactly like the library it is compared with."""
    if not force and not needs_build(out):
        return out
    # -ffp-contract=off: every fused multiply-add in the kernels is an explicit fmaf().  With the default (fast) contraction the
    #   compiler decides per build which a*b+c pairs it fuses, and that decision moved with an unrelated switch
    #   (-fno-slp-vectorize): same source, two roundings, and after 2000 chaotic optimizer steps masks 4 pixels apart
    #   ("determinism").  Now the arithmetic is a property of the source; measured cost: none (70.9 vs 70.3-70.8 us).
    # -fno-slp-vectorize: the SLP pass packs the leftover-unit FMAs into v_pk_fma_f32 and pays two v_mov per pack for it;
    # -amdgpu-mfma-vgpr-form: MFMA results in VGPRs where the allocation allows, instead of AGPRs read back with v_accvgpr_read.
    # Together 14 % fewer VALU instructions in the step kernels' chunk loop (every one of them costs MFMA issue slots),
    # no spills left in the L = 2 kernels: step kernel -1 %.
    base = [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fvisibility=hidden", "-shared", "-fPIC", f"-Wl,--version-script={MAP}",
            f"-I{INCLUDE}"]
    tuning = ["-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form"]

    def command(flags):
        shown = " ".join(["-O3", "-ffp-contract=off"] + flags)
        return base + flags + [f'-DINRFIT_BUILD_FLAGS="{shown}"', SRC, "-o", out]

    cmd = command(tuning + list(extra_flags))
    if verbose:
        print("[awesome_amd.build]", " ".join(cmd), flush=True)
    if subprocess.run(cmd, stderr=subprocess.DEVNULL if not verbose else None).returncode != 0:
        # The two tuning switches change instruction selection and register allocation only (-mllvm options are not a stable
        # interface): the fallback build computes the SAME bits (-ffp-contract=off pins the arithmetic) about 1 % slower.  It is
        # loud on purpose, and inrfit_build_info() / the bench line say which build is loaded.
        print("[awesome_amd.build] WARNING: compile with the tuning switches failed; building WITHOUT "
              + " ".join(tuning) + " (same results, ~1 % slower step kernel)", file=sys.stderr, flush=True)
        subprocess.run(command(list(extra_flags)), check=True)
    return out


if __name__ == "__main__":
    # python -m awesome_amd.build [--force] [--out PATH] [-DFLAG=.. ...]
    args = [a for a in sys.argv[1:] if a != "--force"]
    out = os.path.abspath(args.pop(args.index("--out") + 1)) if "--out" in args else OUT
    extra = [a for a in args if a != "--out"]
    print(build(force="--force" in sys.argv or bool(extra), out=out, extra_flags=extra))
