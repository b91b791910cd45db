"""Cases, inputs and exact references for the direct tests of awesome_amd/csrc/gemm.h (tests/test_gpu_gemm.py launches them on the
device through tests/gemm_shim; tests/test_gemm_cases_host.py checks this file itself).  Nothing here touches the GPU.

Integer cases: every input (operands, bias, skip weights, ext columns, relu-mask values) is an integer-valued float in [-3, 3], K <= 4096,
so every partial sum of the product, of the split-K sum, of the HIDDEN epilogue and of the `extsum` column sums is an integer below
2^24 in whatever order it is taken (`max_intermediate`; the host test asserts it on the reference alone) - float32 computes it exactly
and the comparison is equality of values (-0.0 == +0.0).  Real-valued cases are held to the float32 dot-product bound
|C - C64| <= 2 K 2^-24 (|A| . |B|) and to equal bits of two runs.  The periodic mask (MASKP) multiplies an exact integer product that is
non-zero by construction (operands in [1, 3]) by a factor of 0 or +-1 (x omega): |out - store * factor| <= 1e-3 max(1, omega) |store|.

Every array lives inside a larger allocation (`Buf`): two rows and 64 floats of guard on either side.  Around the operands of the
general and V4 modes the guard - and the rest of every row past the logical extent - is NaN.  In buffer mode (GemmArgs::buf) the guard
is the finite sentinel 1e30 and the weight operand (B) carries zeros from its contiguous extent up to the next multiple of 16, as the
comment at GemmArgs::buf requires; what the hardware's range check zeroes is NOT zero in memory.  Outputs are pre-filled with one NaN
bit pattern; whatever the operation does not define must still carry it afterwards."""
import ctypes
import dataclasses
import math
import os
import subprocess
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "gemm_shim")
SHIM_SRC = os.path.join(SHIM_DIR, "gemm_shim.hip")
SHIM_OUT = os.path.join(SHIM_DIR, "libgemm_shim.so")

EPI = {"store": 0, "hidden": 1, "mask": 2, "maskp": 2}   # GemmArgs::epi (MASKP is MASK with a periodic mask_act)
ACT_RELU, ACT_COS, ACT_SIN = 0, 1, 2                      # include/inrfit.h INR_ACT_*
INR_OK, INR_EINVAL = 0, -1
BK, BM, BN, SPLITK_MAX = 16, 128, 128, 16                 # gemm.h; the host test compares them with gemm_shim_const
PATTERN = 0x7FC0BEEF                                      # the NaN every output element starts as
SENTINEL = 1e30
U = 2.0 ** -24
MAX_LAUNCHES = 400

MS = NS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 131, 257]
KS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 130, 131]
FORMS = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0), "TT": (1, 1)}   # (tA, tB); tB: B stored [N][K]


# ---- the shim ------------------------------------------------------------------------------------------------------------------
def _shim_deps():
    csrc = os.path.join(ROOT, "awesome_amd", "csrc")
    return [SHIM_SRC, os.path.join(csrc, "gemm.h"), os.path.join(ROOT, "include", "inrfit.h")] + \
        [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.startswith("icnn_step") and f.endswith(".h")]


def shim_needs_build():
    return not os.path.exists(SHIM_OUT) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_OUT) for d in _shim_deps())


def build_shim(force=False):
    """tests/gemm_shim/libgemm_shim.so, compiled like libinrfit.so (awesome_amd/build.py) without the version script."""
    if not force and not shim_needs_build():
        return SHIM_OUT
    from awesome_amd import build as b
    base = [b.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fvisibility=hidden", "-shared", "-fPIC",
            f"-I{b.INCLUDE}"]
    tuning = ["-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form"]
    tmp = SHIM_OUT + f".{os.getpid()}.tmp"
    if subprocess.run(base + tuning + [SHIM_SRC, "-o", tmp], stderr=subprocess.DEVNULL).returncode != 0:
        print("[gemm_shim] WARNING: compile with the tuning switches failed; building without " + " ".join(tuning), file=sys.stderr, flush=True)
        subprocess.run(base + [SHIM_SRC, "-o", tmp], check=True)
    os.replace(tmp, SHIM_OUT)
    return SHIM_OUT


class ShimArgs(ctypes.Structure):   # GemmShimArgs of tests/gemm_shim/gemm_shim.hip (the shim's own struct; its size is checked at load)
    _fields_ = [(n, ctypes.c_void_p) for n in ("A", "B", "C", "bias", "skip", "ext", "mask", "extsum")] + [("c_split_stride", ctypes.c_longlong)] + \
        [(n, ctypes.c_int) for n in ("tA", "tB", "M", "N", "K", "lda", "ldb", "ldc", "k_per_split", "epi", "ext_ld", "C_in", "ext_copy",
                                     "mask_ld", "mask_act")] + [("omega", ctypes.c_float)] + \
        [(n, ctypes.c_int) for n in ("buf", "c_zero_to", "padA", "padB")]


_LIB = None


def load_shim():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(build_shim())
        P, I = ctypes.c_void_p, ctypes.c_int
        for name, args in (("gemm_shim_args_size", []), ("gemm_shim_const", [I]), ("gemm_shim_splitk_len", [I]),
                           ("gemm_shim_launch", [ctypes.POINTER(ShimArgs)]), ("gemm_shim_splitk", [I] * 5 + [P, I, P, I, P, P]),
                           ("gemm_shim_pick_mode", [ctypes.POINTER(ShimArgs)] + [ctypes.POINTER(I)] * 3)):
            f = getattr(lib, name)
            f.argtypes, f.restype = args, I
        assert lib.gemm_shim_args_size() == ctypes.sizeof(ShimArgs), (lib.gemm_shim_args_size(), ctypes.sizeof(ShimArgs))
        _LIB = lib
    return _LIB


# ---- a case ----------------------------------------------------------------------------------------------------------------------
def r4(x):
    return (x + 3) // 4 * 4


def r16(x):
    return (x + 15) // 16 * 16


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str               # NT / NN / TN / TT / split / hidden / mask / extsum / real
    form: str
    M: int
    N: int
    K: int
    lda: int
    ldb: int
    ldc: int
    mode: int                # the MODE gemm_pick_mode must return for it
    offA: int = 0            # floats past a 16-byte boundary
    offB: int = 0
    offC: int = 0
    padA: int = 0
    padB: int = 0
    buf: int = 0
    kps: int = 0             # k_per_split (0: no split)
    epi: str = "store"
    C_in: int = 0
    ext_copy: int = 0
    ext_ld: int = 0
    ext_off: int = 0
    mask_ld: int = 0
    mask_off: int = 0
    mask_act: int = ACT_RELU
    omega: float = 0.0
    c_zero_to: int = 0
    extsum: bool = False
    real: bool = False
    splitk: bool = False     # through gemm_shim_splitk (gemm_rm_splitk: its own slice length, dense C, the slice-sum kernel)
    positive: bool = False   # operands in [1, 3]: no product is zero

    @property
    def tA(self):
        return FORMS[self.form][0]

    @property
    def tB(self):
        return FORMS[self.form][1]

    @property
    def shapeA(self):        # (stored rows, contiguous logical extent)
        return (self.K, self.M) if self.tA else (self.M, self.K)

    @property
    def shapeB(self):
        return (self.N, self.K) if self.tB else (self.K, self.N)

    @property
    def kslice(self):
        if self.splitk:
            return max(128, r16((self.K + SPLITK_MAX - 1) // SPLITK_MAX))   # gemm_splitk_len; the host test compares it with the shim's
        return self.kps if self.kps > 0 else r16(self.K)

    @property
    def splits(self):
        return (self.K + self.kslice - 1) // self.kslice

    @property
    def c_stride(self):      # floats between the slices of C: two guard rows behind every slice
        return self.M * self.N if self.splitk else (self.M + 2) * self.ldc

    @property
    def tiles(self):
        return ((self.N + BN - 1) // BN, (self.M + BM - 1) // BM, self.splits)

    @property
    def kernel(self):        # which of the seven kernels per mode
        if self.epi == "store":
            return self.form
        return "MASKP" if self.epi == "maskp" else self.epi.upper()

    @property
    def launches(self):
        return 2 if self.real else 1

    def row(self):
        d = dataclasses.asdict(self)
        dflt = {f.name: f.default for f in dataclasses.fields(self)}
        return " ".join(f"{k}={v}" for k, v in d.items() if dflt.get(k, dataclasses.MISSING) != v)

    def validate(self):
        """what keeps every access of the launch inside the case's allocations (checked before anything runs)"""
        for contig, ld, pad in ((self.shapeA[1], self.lda, self.padA), (self.shapeB[1], self.ldb, self.padB)):
            assert ld >= (r4(contig) if pad else contig), self
        assert min(self.M, self.N, self.K) >= 1 and self.K <= 4096, self
        assert self.ldc >= max(self.N + self.ext_copy, self.c_zero_to, self.N), self
        assert self.kslice % BK == 0, self
        assert 0 <= self.C_in <= 3 and (self.epi != "hidden" or self.C_in >= 1), self
        assert self.epi == "store" or not (self.splits > 1 or self.splitk or self.real), self
        assert not self.extsum or (self.epi in ("mask", "maskp") and self.C_in >= 1), self
        if self.epi in ("hidden",) or self.extsum:
            assert self.ext_ld >= 1 + self.C_in, self
        if self.epi in ("mask", "maskp"):
            assert self.mask_ld >= self.N and self.form == "NN", self
            assert (self.epi == "maskp") == (self.mask_act != ACT_RELU) and (self.epi != "maskp" or self.positive), self
        if self.epi == "hidden":
            assert self.form == "NT", self
        if self.buf:         # buffer mode: 16-byte operands, the weight operand (B) zero-padded to 16 k / 16 columns inside its rows
            assert self.mode == 2 and self.padA and self.padB and self.lda % 4 == 0 and self.ldb % 4 == 0 and not (self.offA or self.offB), self
            if self.form in ("NT", "NN"):
                assert self.ldb >= r16(self.shapeB[1]), self
        if self.splitk:
            assert self.ldc == self.N and self.offC == 0 and not self.kps, self


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _ld_off(contig, vec, variant):
    """row stride and base offset that give an operand the widest load `vec`"""
    if vec == 4:
        return (r4(contig) + 4, 0) if variant else (r4(contig), 0)
    if vec == 2:
        return (r4(contig) + 4, 2) if variant else (r4(contig) + 2, 0)     # base 8 bytes off / row stride 2 mod 4
    return (r4(contig) + 4, 1) if variant else (r4(contig) + 1, 0)         # base 4 bytes off / odd row stride


def _mk(name, group, form, M, N, K, mode, vecA=4, vecB=4, variant=0, padA=None, padB=None, ldc=None, lda=None, ldb=None, **kw):
    """a case of MODE `mode`: 0 with the operand widths (vecA, vecB); 1 aligned and padded where the extent asks for it; 2 as wide.h
    launches (padded rows, zero-padded weight rows)"""
    tA, tB = FORMS[form]
    cA, cB = (M if tA else K), (K if tB else N)
    if mode == 0:
        (la, oa), (lb, ob) = _ld_off(cA, vecA, variant & 1), _ld_off(cB, vecB, (variant >> 1) & 1)
        pa = (variant >> 2) & 1 if padA is None else padA
        pb = (variant >> 3) & 1 if padB is None else padB
        buf = 0
    else:
        la, oa, lb, ob = r4(cA) + 4 * (variant & 1), 0, r4(cB) + 4 * ((variant >> 1) & 1), 0
        pa = 1 if (cA & 3 or mode == 2) else (variant >> 2) & 1
        pb = 1 if (cB & 3 or mode == 2) else (variant >> 3) & 1
        buf = int(mode == 2)
        if buf and form in ("NT", "NN"):
            lb = r16(cB) + 16 * ((variant >> 1) & 1)
    c = Case(name=name, group=group, form=form, M=M, N=N, K=K, lda=lda or la, ldb=ldb or lb, ldc=ldc or N + (variant % 3), mode=mode, offA=oa, offB=ob,
             padA=pa, padB=pb, buf=buf, **kw)
    c.validate()
    return c


_GENERAL_WIDTHS = [(4, 2), (4, 1), (2, 4), (2, 2), (2, 1), (1, 4), (1, 2), (1, 1)]   # (4, 4) without padding: the straddle cases below


def _form_cases():
    """every value of every extent with every operand form and mode: twelve cases per pair, the extents dealt by three permutations"""
    out = []
    for fi, form in enumerate(FORMS):
        for mode in range(3):
            for i in range(12):
                M, N, K = MS[i], NS[(5 * i + 3 + fi + mode) % 12], KS[(7 * i + 1 + 2 * fi + mode) % 12]
                va, vb = _GENERAL_WIDTHS[(i + fi) % 8]
                out.append(_mk(f"{form}-m{mode}-{M}x{N}x{K}", form, form, M, N, K, mode, va, vb, variant=i + 3 * fi, offC=(i % 4 == 3) * 1))
        # 16-byte operands whose contiguous extent is no multiple of 4 and may not be read past: scalar loads on the straddling tile only
        out.append(_mk(f"{form}-straddle-131", form, form, 131, 131, 131, 0, 4, 4, variant=0, padA=0, padB=0))
        out.append(_mk(f"{form}-straddle-257x130", form, form, 257, 130, 33, 0, 4, 4, variant=3, padA=0, padB=0))
        out.append(_mk(f"{form}-straddle-8byte", form, form, 129, 131, 17, 0, 2, 2, variant=0, padA=0, padB=0))
        out.append(_mk(f"{form}-padded-8byte", form, form, 129, 131, 17, 0, 2, 2, variant=3, padA=1, padB=1))
        # V4 through padA / padB at 131 and 350
        out.append(_mk(f"{form}-v4-pad-131x350", form, form, 131, 350, 131, 1, variant=0))
        out.append(_mk(f"{form}-v4-pad-350x131", form, form, 350, 131, 350, 1, variant=3))
    return out


def _split_cases():
    out = []
    lens = [(K, kps) for K in (129, 513, 2064) for kps in (16, 128, 512)]
    shapes = [(5, 3), (65, 4), (1, 131), (129, 5), (3, 63), (64, 65), (4, 129), (131, 1), (63, 64)]
    for fi, form in enumerate(FORMS):
        for j, (K, kps) in enumerate(lens):
            M, N = shapes[(j + 2 * fi) % 9]
            mode = (j + fi) % 3
            va, vb = _GENERAL_WIDTHS[(j + 3 * fi) % 8]
            out.append(_mk(f"split-{form}-m{mode}-{M}x{N}x{K}/{kps}", "split", form, M, N, K, mode, va, vb, variant=j + fi, kps=kps))
    # grids whose workgroup count is a multiple of 8 with more than one tile take the XCD re-deal; 3 x 1 x 3 does not
    for form, mode in (("NT", 1), ("NN", 0), ("TN", 2), ("TT", 1)):
        out.append(_mk(f"split-{form}-m{mode}-grid2x2x2", "split", form, 129, 129, 129, mode, 1, 2, variant=1, kps=128))
    for form, mode in (("NT", 0), ("TN", 2), ("NN", 1)):
        out.append(_mk(f"split-{form}-m{mode}-grid3x2x4", "split", form, 131, 257, 513, mode, 2, 1, variant=2, kps=144))
    for form, mode in (("TN", 2), ("TT", 0), ("NT", 2)):
        out.append(_mk(f"split-{form}-m{mode}-grid3x1x3", "split", form, 5, 257, 129, mode, 4, 1, variant=0, kps=48))
    # gemm_rm_splitk: the slice-sum kernel at M N around its block of 256
    for j, (M, N) in enumerate(((1, 1), (15, 17), (16, 16), (1, 257))):
        for form, K in (("TN", 513), ("NN", 2064)):
            mode = int(M % 4 == 0 and N % 4 == 0)   # (V4 without pad flags: contiguous extents that are multiples of 4)
            out.append(_mk(f"splitk-{form}-{M}x{N}x{K}", "split", form, M, N, K, mode, 1, 2, variant=j & 3, padA=0, padB=0, ldc=N, splitk=True,
                           **_dense_lds(form, M, N, K, mode)))
    out.append(_mk("splitk-NT-16x16x129", "split", "NT", 16, 16, 129, 0, 1, 1, variant=0, padA=0, padB=0, ldc=16, splitk=True))
    out.append(_mk("splitk-TT-15x17x513", "split", "TT", 15, 17, 513, 0, 2, 1, variant=0, padA=0, padB=0, ldc=17, splitk=True))
    return out


def _dense_lds(form, M, N, K, mode):
    """gemm_rm_splitk sets no pad flag: V4 needs contiguous extents that are multiples of 4, so mode 1 pads nothing and uses dense-enough rows"""
    if mode == 0:
        return {}
    tA, tB = FORMS[form]
    cA, cB = (M if tA else K), (K if tB else N)
    assert cA % 4 == 0 and cB % 4 == 0, (form, M, N, K)
    return dict(lda=cA + 4, ldb=cB)


def _not4(x):
    return x if x % 4 else x + 1


def _hidden_cases():
    out, j = [], 0
    for C_in in (1, 2, 3):
        for ec in (0, 1 + C_in, 1 + C_in + 3):
            for vec in (1, 0):
                for M in (1, 129):
                    mode = j % 3
                    if vec:          # N and ldc multiples of 4: 16-byte stores
                        N, ldc, offC = (64, 132)[j % 2], r4((64, 132)[j % 2] + ec) + 4 * (j % 2), 0
                    else:            # scalar stores: N odd / ldc odd / C four bytes off
                        N, ldc, offC = [(65, 65 + ec + 3, 0), (64, _not4(64 + ec + 1), 0), (132, 132 + r4(ec), 1), (3, 4 + r4(ec), 0), (131, 131 + ec, 0)][j % 5]
                    K = (17, 32, 130, 5)[j % 4]
                    va, vb = _GENERAL_WIDTHS[j % 8]
                    out.append(_mk(f"hidden-m{mode}-C{C_in}-copy{ec}-{M}x{N}x{K}-{'vec' if vec else 'scalar'}", "hidden", "NT", M, N, K, mode, va, vb,
                                   variant=j, ldc=ldc, offC=offC, epi="hidden", C_in=C_in, ext_copy=ec, ext_ld=1 + C_in + (j % 3), ext_off=j % 2))
                    j += 1
    # more than one column tile (the ext columns are copied by the LAST one) and a grid that takes the re-deal
    out.append(_mk("hidden-m2-grid2x4", "hidden", "NT", 4 * 128 - 3, 131, 33, 2, variant=1, ldc=136, epi="hidden", C_in=2, ext_copy=5, ext_ld=3))
    out.append(_mk("hidden-m1-grid3x2", "hidden", "NT", 129, 257, 16, 1, variant=2, ldc=264, epi="hidden", C_in=3, ext_copy=7, ext_ld=8))
    return out


def _mask_cases():
    out, j = [], 0
    layouts = ((0, 0), (1, 0), (0, 1))   # (mask_ld odd, mask base 4 bytes off): aligned / scalar mask reads twice
    for N in (129, 130, 131):
        for odd, moff in layouts:
            for mode in range(3):
                M = (5, 129, 257)[(j + mode) % 3]
                K = (16, 33, 131, 4)[j % 4]
                va, vb = _GENERAL_WIDTHS[(j + 5) % 8]
                out.append(_mk(f"mask-m{mode}-{M}x{N}x{K}-ld{'odd' if odd else '4'}-off{moff}", "mask", "NN", M, N, K, mode, va, vb, variant=j,
                               ldc=132 + (4, 0, 1)[j % 3], offC=(j % 7 == 6) * 1, epi="mask", c_zero_to=132, mask_ld=136 + odd, mask_off=moff))
                j += 1
    for act, omega in ((ACT_COS, 0.0), (ACT_SIN, 30.0), (ACT_SIN, 0.5)):
        for mode in range(3):
            for odd, moff in ((0, 0), (1, 1)):
                M, N, K = (65, 129, 4)[j % 3], (131, 64, 129)[(j + mode) % 3], (17, 32, 5)[j % 3]
                va, vb = _GENERAL_WIDTHS[(j + 2) % 8]
                out.append(_mk(f"maskp-m{mode}-act{act}-w{omega}-{M}x{N}x{K}-ld{'odd' if odd else '4'}", "mask", "NN", M, N, K, mode, va, vb, variant=j,
                               ldc=r4(N) + 4, epi="maskp", mask_act=act, omega=omega, c_zero_to=r4(N), mask_ld=r4(N) + 4 + odd, mask_off=moff,
                               positive=True))
                j += 1
    return out


def _extsum_cases():
    out, j = [], 0
    for M in (1, 127, 129, 257):
        for mode in range(3):
            C_in, N, K = (1, 2, 3)[(j + mode) % 3], (5, 65, 131, 129)[j % 4], (17, 32, 3, 130)[(j + mode) % 4]
            va, vb = _GENERAL_WIDTHS[(j + 1) % 8]
            out.append(_mk(f"extsum-m{mode}-C{C_in}-{M}x{N}x{K}", "extsum", "NN", M, N, K, mode, va, vb, variant=j, ldc=r4(N) + 4 * (j % 2), epi="mask",
                           c_zero_to=r4(N), mask_ld=r4(N) + (j % 2), mask_off=0, C_in=C_in, ext_ld=1 + C_in + (j % 2), ext_off=j % 3 == 2, extsum=True))
            j += 1
    # what wide.h's layer 0 launches: the periodic mask with the column sums, in buffer mode
    out.append(_mk("extsum-m2-maskp-sin", "extsum", "NN", 257, 131, 33, 2, variant=1, ldc=136, epi="maskp", mask_act=ACT_SIN, omega=30.0, c_zero_to=132,
                   mask_ld=136, C_in=2, ext_ld=3, extsum=True, positive=True))
    return out


def _real_cases():
    out = []
    for fi, form in enumerate(FORMS):
        for mode in range(3):
            M, N, K = (131, 65, 129)[(fi + mode) % 3], (65, 129, 131)[(fi + mode) % 3], (131, 130, 33)[mode]
            va, vb = _GENERAL_WIDTHS[(2 * fi + mode) % 8]
            out.append(_mk(f"real-{form}-m{mode}-{M}x{N}x{K}", "real", form, M, N, K, mode, va, vb, variant=fi + mode, real=True))
    out.append(_mk("real-TN-m2-split", "real", "TN", 129, 131, 2064, 2, variant=1, kps=512, real=True))
    out.append(_mk("real-NT-m0-split", "real", "NT", 65, 63, 513, 0, 2, 1, variant=2, kps=128, real=True))
    out.append(_mk("real-splitk-TN", "real", "TN", 16, 16, 2064, 1, variant=0, padA=0, padB=0, ldc=16, splitk=True, real=True, lda=20, ldb=16))
    out.append(_mk("real-splitk-NN", "real", "NN", 15, 17, 513, 0, 1, 1, variant=0, padA=0, padB=0, ldc=17, splitk=True, real=True))
    return out


def _table():
    cases = _form_cases() + _split_cases() + _hidden_cases() + _mask_cases() + _extsum_cases() + _real_cases()
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _table()
GROUPS = ["NT", "NN", "TN", "TT", "split", "hidden", "mask", "extsum", "real"]


def group(name):
    return [c for c in CASES if c.group == name]


# rejected launches: (what, code, overrides of a valid NT / NN case)
REJECTIONS = [
    ("hidden on NN", INR_EINVAL, dict(form="NN", epi="hidden")),
    ("hidden on TN", INR_EINVAL, dict(form="TN", epi="hidden")),
    ("hidden on TT", INR_EINVAL, dict(form="TT", epi="hidden")),
    ("mask on NT", INR_EINVAL, dict(form="NT", epi="mask")),
    ("mask on TN", INR_EINVAL, dict(form="TN", epi="mask")),
    ("mask on TT", INR_EINVAL, dict(form="TT", epi="mask")),
    ("M = 0", INR_EINVAL, dict(M=0)),
    ("N = 0", INR_EINVAL, dict(N=0)),
    ("K = 0", INR_EINVAL, dict(K=0)),
    ("M < 0", INR_EINVAL, dict(M=-1)),
    ("N < 0", INR_EINVAL, dict(N=-128)),
    ("K < 0", INR_EINVAL, dict(K=-16)),
    ("slices of 8", INR_EINVAL, dict(K=64, kps=8)),
    ("slices of 20", INR_EINVAL, dict(K=64, kps=20)),
    ("slices of 24, buffer mode", INR_EINVAL, dict(K=64, kps=24, buf=1, padA=1, padB=1)),
    ("slices of 132", INR_EINVAL, dict(K=513, kps=132)),
]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Buf:
    flat: torch.Tensor       # the whole allocation (float32)
    base: int                # index of the array's first element
    rows: int
    ld: int
    cols: int                # logical extent of a row

    def view(self, cols=None, rows=None, at=0):
        return self.flat.as_strided((self.rows if rows is None else rows, self.cols if cols is None else cols), (self.ld, 1), self.base + at)


def _nan_pattern(n):
    return torch.full((n,), PATTERN, dtype=torch.int32).view(torch.float32)


def _alloc(rows, ld, cols, off, fill, span=None):
    g = r4(2 * ld + 64)
    n = g + 4 + (rows * ld if span is None else span) + g
    flat = _nan_pattern(n) if fill is None else torch.full((n,), fill, dtype=torch.float32)
    return Buf(flat, g + off, rows, ld, cols)


def _ints(gen, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


_CACHE = {}


def materialise(case):
    """the case's arrays (CPU, built once and shared: callers must not change them): operands and epilogue inputs as Buf, outputs as Buf
    pre-filled with the NaN pattern"""
    if case.name in _CACHE:
        return _CACHE[case.name]
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    fill = SENTINEL if case.buf else float("nan")
    m = {}
    for key, (rows, cols), ld, off in (("A", case.shapeA, case.lda, case.offA), ("B", case.shapeB, case.ldb, case.offB)):
        b = _alloc(rows, ld, cols, off, fill)
        if case.real:
            b.view()[:] = torch.randn(rows, cols, generator=gen)
        else:
            b.view()[:] = _ints(gen, (rows, cols), 1 if case.positive else -3, 3)
        m[key] = b
    if case.buf and case.form in ("NT", "NN"):   # the weight operand's rows: zeros up to the next multiple of 16
        cols = case.shapeB[1]
        if r16(cols) > cols:
            m["B"].view(cols=r16(cols) - cols, at=cols)[:] = 0.0
    M, N, C = case.M, case.N, case.C_in
    if case.epi == "hidden":
        m["bias"] = _alloc(1, N, N, 1, float("nan"))
        m["bias"].view()[:] = _ints(gen, (1, N))
        m["skip"] = _alloc(N, C, C, 0, float("nan"))
        m["skip"].view()[:] = _ints(gen, (N, C))
    if case.epi == "hidden" or case.extsum:
        m["ext"] = _alloc(M, case.ext_ld, 1 + C, case.ext_off, float("nan"))
        m["ext"].view()[:] = _ints(gen, (M, 1 + C))
    if case.epi in ("mask", "maskp"):
        m["mask"] = _alloc(M, case.mask_ld, N, case.mask_off, float("nan"))
        if case.epi == "mask":
            z = _ints(gen, (M, N))
            z[(z == 0) & (torch.rand(M, N, generator=gen) < 0.5)] = -0.0
        else:   # quarter turns: omega z (cos: z) in {0, pi / 2, pi, 3 pi / 2}
            q = torch.randint(0, 4, (M, N), generator=gen)
            z = (q.double() * (math.pi / 2) / (case.omega if case.mask_act == ACT_SIN else 1.0)).float()
            m["quarter"] = q
        m["mask"].view()[:] = z
    span = case.splits * case.c_stride
    m["C"] = _alloc(M + 2, case.ldc, N, case.offC, None, span=span)
    if case.splitk:
        m["part"] = _alloc(1, 1, 1, 0, None, span=SPLITK_MAX * M * N)
    if case.extsum:
        m["extsum"] = _alloc(1, 1, 1, 0, None, span=case.tiles[1] * N * (1 + C))
    _CACHE[case.name] = m
    return m


# ---- references ------------------------------------------------------------------------------------------------------------------
def _logical(case, m, dtype):
    A = m["A"].view().to(dtype)
    B = m["B"].view().to(dtype)
    return (A.t() if case.tA else A), (B.t() if case.tB else B)     # [M][K], [K][N]


_REFS = {}


def reference(case):
    """dict(C=, C_def=, C_tol=, E=, max_intermediate=): `C` the expected allocation of C as float64 (NaN where the operation defines
    nothing: C_def False), C_tol None (exact) or the allowed |difference| per element; E the expected `extsum` (exact under the relu
    mask; under the periodic mask `check` holds the sums to the device's own C instead).  Integer cases: int64 arithmetic;
    max_intermediate is the largest sum of absolute values of the terms of any sum taken, which bounds every partial sum in any order."""
    if case.name in _REFS:
        return _REFS[case.name]
    m = materialise(case)
    M, N, K, C = case.M, case.N, case.K, case.C_in
    exact = not case.real
    dt = torch.int64 if exact else torch.float64
    A, B = _logical(case, m, dt)
    Cb = m["C"]
    ref = torch.full((Cb.flat.numel(),), float("nan"), dtype=torch.float64)
    tol = torch.zeros_like(ref)
    defd = torch.zeros(Cb.flat.numel(), dtype=torch.bool)
    absprod = A.abs() @ B.abs()
    out = dict(max_intermediate=float(absprod.max()), E=None)

    def put(at, rows, cols, ld, values, t=None, col0=0):
        idx = (Cb.base + at + col0 + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]).reshape(-1)
        ref[idx] = values.reshape(-1).double()
        defd[idx] = True
        if t is not None:
            tol[idx] = t.reshape(-1).double()

    if case.splitk:
        put(0, M, N, N, A @ B, None if exact else 2 * K * U * absprod)
    elif case.epi == "store":
        for z in range(case.splits):
            lo, hi = z * case.kslice, min(K, (z + 1) * case.kslice)
            put(z * case.c_stride, M, N, case.ldc, A[:, lo:hi] @ B[lo:hi], None if exact else 2 * (hi - lo) * U * (A[:, lo:hi].abs() @ B[lo:hi].abs()))
    else:
        P = A @ B
        if case.epi == "hidden":
            bias, skip, ext = m["bias"].view()[0].long(), m["skip"].view().long(), m["ext"].view().long()
            pre = P + bias[None, :] + ext[:, 1:] @ skip.t()
            out["max_intermediate"] = float((absprod + bias.abs()[None, :] + ext[:, 1:].abs() @ skip.abs().t()).max())
            put(0, M, N, case.ldc, pre.clamp(min=0))
            if case.ext_copy:
                tail = torch.zeros(M, case.ext_copy, dtype=torch.int64)
                tail[:, :1 + C] = ext
                put(0, M, case.ext_copy, case.ldc, tail, col0=N)
            res = None
        elif case.epi == "mask":
            res = P * (m["mask"].view() > 0).long()
            put(0, M, N, case.ldc, res)
        else:
            q = m["quarter"]
            if case.mask_act == ACT_COS:      # -sin(z)
                factor = torch.tensor([0.0, -1.0, 0.0, 1.0], dtype=torch.float64)[q]
            else:                             # omega cos(omega z)
                factor = case.omega * torch.tensor([1.0, 0.0, -1.0, 0.0], dtype=torch.float64)[q]
            assert bool((P != 0).all()), case
            res = P.double() * factor
            put(0, M, N, case.ldc, res, 1e-3 * max(1.0, case.omega) * P.abs().double())
        if case.c_zero_to > N:
            put(0, M, case.c_zero_to - N, case.ldc, torch.zeros(M, case.c_zero_to - N), col0=N)
        if case.extsum:
            x1 = torch.cat([torch.ones(M, 1, dtype=torch.int64), m["ext"].view().long()[:, 1:]], dim=1)    # (1, x_m)
            ty = case.tiles[1]
            E = torch.zeros(ty, N, 1 + C, dtype=torch.float64)
            Eabs = torch.zeros_like(E)
            for t in range(ty):
                rows = slice(t * BM, min(M, (t + 1) * BM))
                E[t] = res[rows].double().t() @ x1[rows].double()
                Eabs[t] = res[rows].double().abs().t() @ x1[rows].double().abs()
            out["E"] = E.reshape(-1)
            if case.epi == "mask":
                out["max_intermediate"] = max(out["max_intermediate"], float(Eabs.max()))
    out.update(C=ref, C_def=defd, C_tol=None if (exact and case.epi != "maskp") else tol)
    _REFS[case.name] = out
    return out


# ---- launch arguments and the device-side rules the coverage is counted by ------------------------------------------------------
def fill_args(case, addr):
    """ShimArgs of the case; addr[key] = address of the first byte of the allocation materialise(case)[key].flat"""
    m = materialise(case)

    def p(key):
        return addr[key] + 4 * m[key].base if key in m else None

    a = ShimArgs()
    a.A, a.B, a.C = p("A"), p("B"), p("C")
    a.bias, a.skip, a.ext, a.mask = p("bias"), p("skip"), p("ext"), p("mask")
    a.extsum = p("extsum") if case.extsum else None
    a.c_split_stride = case.c_stride
    a.tA, a.tB = case.tA, case.tB
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc = case.M, case.N, case.K, case.lda, case.ldb, case.ldc
    a.k_per_split = case.kps
    a.epi = EPI[case.epi]
    a.ext_ld, a.C_in, a.ext_copy = case.ext_ld, case.C_in, case.ext_copy
    a.mask_ld, a.mask_act, a.omega = case.mask_ld, case.mask_act, case.omega
    a.buf, a.c_zero_to, a.padA, a.padB = case.buf, case.c_zero_to, case.padA, case.padB
    return a


def fake_addresses(case):
    """addresses aligned like an allocator's (256 bytes), for the host-side questions (mode, flavours): nothing is ever read there"""
    return {key: 0x10000000 * (i + 1) for i, key in enumerate(materialise(case)) if key != "quarter"}


def pick_mode(lib, case, addr=None):
    """(MODE, vecA, vecB, buf) as gemm_launch decides them.  gemm_launch has set k_per_split by then: so does this."""
    a = fill_args(case, addr or fake_addresses(case))
    a.k_per_split = case.kslice
    va, vb, bf = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    mode = lib.gemm_shim_pick_mode(ctypes.byref(a), ctypes.byref(va), ctypes.byref(vb), ctypes.byref(bf))
    return mode, va.value, vb.value, bf.value


def _flavour(vec, pad, c0, length, cmax):      # gemm_flavour
    if vec == 1:
        return 1
    straddle = cmax % vec != 0 and c0 < cmax < c0 + length
    return 1 if (straddle and not pad) else vec


def load_flavours(case, vecA, vecB):
    """the sets of load flavours the general kernel takes for A and for B over all its tiles and k-steps"""
    def free(vec, pad, extent):
        return {_flavour(vec, pad, t0, BM, extent) for t0 in range(0, extent, BM)}

    def along_k(vec, pad):
        got = set()
        for z in range(case.splits):
            lo, hi = z * case.kslice, min(case.K, (z + 1) * case.kslice)
            for kb in range(lo, hi, BK):
                got.add(_flavour(vec, pad, kb, BK, hi) if kb + BK > hi else vec)
        return got
    fa = free(vecA, case.padA, case.M) if case.tA else along_k(vecA, case.padA)
    fb = along_k(vecB, case.padB) if case.tB else free(vecB, case.padB, case.N)
    return fa, fb


def store_paths(case):
    """(values of vec_c, values of vec_mask) over the lanes of the launch whose first column lies inside C"""
    def lanes(ok):
        return {bool(ok and n + 3 < case.N) for n in range(0, case.N, 4)}
    vc = set()
    for z in range(case.splits):
        vc |= lanes(case.ldc % 4 == 0 and (4 * (case.offC + z * case.c_stride)) % 16 == 0)
    vm = lanes(case.mask_ld % 4 == 0 and case.mask_off % 4 == 0) if case.epi in ("mask", "maskp") else set()
    return vc, vm


def redealt(case):
    gx, gy, gz = case.tiles
    return (gx * gy * gz) % 8 == 0 and gx * gy > 1


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def check(case, got_C, got_E=None, got_part=None):
    """problems of a launch's outputs (the whole allocations, float32 on the CPU) as a list of strings: empty when all is well"""
    ref, m, bad = reference(case), materialise(case), []

    def first(mask):
        return [int(i) for i in torch.nonzero(mask).flatten()[:4]]

    defd = ref["C_def"]
    untouched = got_C.view(torch.int32)[~defd] == PATTERN
    if not bool(untouched.all()):
        idx = torch.nonzero(~defd).flatten()[~untouched]
        bad.append(f"{int((~untouched).sum())} elements outside the result were written, first at offsets {[int(i) - m['C'].base for i in idx[:4]]} from C")
    want, have = ref["C"][defd], got_C[defd].double()
    if ref["C_tol"] is None:
        wrong = ~(have == want)
    else:
        wrong = ~((have - want).abs() <= ref["C_tol"][defd])
    if bool(wrong.any()):
        idx = torch.nonzero(defd).flatten()[wrong]
        bad.append(f"{int(wrong.sum())} of {int(defd.sum())} elements of C differ, first at offsets {[int(i) - m['C'].base for i in idx[:4]]} from C: "
                   f"got {have[wrong][:4].tolist()} expected {want[wrong][:4].tolist()}")
    if case.extsum:
        Eb = m["extsum"]
        n = ref["E"].numel()
        have = got_E[Eb.base:Eb.base + n].double()
        guard = torch.ones(got_E.numel(), dtype=torch.bool)
        guard[Eb.base:Eb.base + n] = False
        if not bool((got_E.view(torch.int32)[guard] == PATTERN).all()):
            bad.append("extsum: elements outside [row tiles][N][1 + C_in] were written")
        want = ref["E"]
        if case.epi == "mask":
            wrong = ~(have == want)
        else:   # periodic mask: C (held to its own bar above) is not exact, so the sums are held to the float64 sums of what the device
            # stored in C: 128 float32 terms per sum in a fixed but unspecified order, |difference| <= 2 128 2^-24 sum |terms|
            x1 = torch.cat([torch.ones(case.M, 1, dtype=torch.float64), m["ext"].view().double()[:, 1:]], dim=1)
            dev = got_C.as_strided((case.M, case.N), (case.ldc, 1), m["C"].base).double()
            tiles = [slice(t * BM, (t + 1) * BM) for t in range(case.tiles[1])]
            want = torch.stack([dev[t].t() @ x1[t] for t in tiles]).reshape(-1)
            wrong = ~((have - want).abs() <= 2 * BM * U * torch.stack([dev[t].abs().t() @ x1[t].abs() for t in tiles]).reshape(-1))
        if bool(wrong.any()):
            bad.append(f"extsum: {int(wrong.sum())} of {n} sums differ, first at {first(wrong)}: got {have[wrong][:4].tolist()} expected {want[wrong][:4].tolist()}")
    if case.splitk:   # the partial products lie inside [GEMM_SPLITK_MAX][M][N]
        Pb = m["part"]
        guard = torch.ones(got_part.numel(), dtype=torch.bool)
        guard[Pb.base:Pb.base + SPLITK_MAX * case.M * case.N] = False
        if not bool((got_part.view(torch.int32)[guard] == PATTERN).all()):
            bad.append("part: elements outside [GEMM_SPLITK_MAX][M][N] were written")
    return bad
