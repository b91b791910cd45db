"""awesome_amd/csrc/gemm.h launched directly (tests/gemm_shim) on the cases of tests/gemm_cases.py: all 21 kernels - four operand
forms, three load modes, four epilogues - at the extents, strides, alignments and slice lengths where their index arithmetic has an
edge.  Integer cases must reproduce the int64 reference exactly, real-valued ones stay inside the float32 dot-product bound and give
equal bits twice; every output element the operation does not define must keep the NaN pattern it was filled with.  The operands lie
well inside their allocations (guards of two rows and 64 floats that poison a wrong read: NaN, or 1e30 in buffer mode); only the
guards around the OUTPUTS are checked.  One process, the default stream, one synchronisation per group."""
import ctypes

import pytest
import torch

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu


def _launch(lib, c, dev):
    """uploads the case, launches it (real-valued cases twice, from fresh outputs) and returns what to check after the group's
    synchronisation: (case, device tensors per run)"""
    m = G.materialise(c)
    t = {k: b.flat.to(dev) for k, b in m.items() if isinstance(b, G.Buf)}
    runs = []
    for run in range(c.launches):
        if run:
            for k in ("C", "part", "extsum"):
                if k in t:
                    t[k] = m[k].flat.to(dev)
        addr = {k: v.data_ptr() for k, v in t.items()}
        assert all(a % 256 == 0 for a in addr.values()), c.row()        # the offsets of the table decide the alignment
        assert G.pick_mode(lib, c, addr)[0] == c.mode, c.row()
        a = G.fill_args(c, addr)
        if c.splitk:
            rc = lib.gemm_shim_splitk(c.tA, c.tB, c.M, c.N, c.K, a.A, c.lda, a.B, c.ldb, a.C, addr["part"] + 4 * m["part"].base)
        else:
            rc = lib.gemm_shim_launch(ctypes.byref(a))
        assert rc == G.INR_OK, (rc, c.row())
        runs.append({k: t[k] for k in ("C", "part", "extsum") if k in t})
    return c, t, runs


@pytest.mark.parametrize("group", G.GROUPS)
def test_gemm_cases(group):
    lib = G.load_shim()
    dev = torch.device("cuda:0")
    cases = G.group(group)
    assert cases
    for c in cases:
        G.reference(c)                       # (the CPU side first: a broken case fails before anything is launched)
    launched = [_launch(lib, c, dev) for c in cases]
    torch.cuda.synchronize()
    failures = []
    for c, _, runs in launched:
        outs = [{k: v.cpu() for k, v in r.items()} for r in runs]
        bad = G.check(c, outs[0]["C"], outs[0].get("extsum"), outs[0].get("part"))
        if c.real and not torch.equal(outs[0]["C"].view(torch.int32), outs[1]["C"].view(torch.int32)):
            bad.append("two runs gave different bits")
        if bad:
            failures.append(f"[{c.row()}] " + "; ".join(bad))
    assert not failures, f"{len(failures)} of {len(cases)} cases:\n" + "\n".join(failures)
