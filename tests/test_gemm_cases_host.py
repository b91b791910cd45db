"""The CPU side of the direct GEMM tests (tests/test_gpu_gemm.py): the shim over awesome_amd/csrc/gemm.h compiles for gfx950, the case
table of tests/gemm_cases.py reaches every kernel, load flavour and store path it claims to, its references are exact and agree with a
plain float64 evaluation, and gemm_launch rejects what it must before any launch.  No GPU: nothing here launches a kernel."""
import collections
import ctypes
import dataclasses

import pytest
import torch

from tests import gemm_cases as G


@pytest.fixture(scope="module")
def lib():
    return G.load_shim()


@pytest.fixture(scope="module")
def picked(lib):
    return {c.name: G.pick_mode(lib, c) for c in G.CASES}


def test_shim_compiles_and_matches_gemm_h(lib):
    assert not G.shim_needs_build()
    assert [lib.gemm_shim_const(i) for i in range(4)] == [G.BK, G.BM, G.BN, G.SPLITK_MAX]
    for K in (1, 129, 513, 2048, 2064, 4096):
        assert lib.gemm_shim_splitk_len(K) == dataclasses.replace(G.CASES[0], K=K, splitk=True).kslice, K


def test_table_size_and_validity():
    assert sum(c.launches for c in G.CASES) <= G.MAX_LAUNCHES
    assert {c.group for c in G.CASES} == set(G.GROUPS)
    for c in G.CASES:
        c.validate()
        assert not c.real or c.epi == "store"
        m = G.materialise(c)
        assert max(b.flat.numel() for b in m.values() if isinstance(b, G.Buf)) * 4 < 8 << 20, c.row()


def test_every_case_runs_the_mode_it_names(picked):
    """pick_mode works on sizes and pointer VALUES: the addresses are made up, nothing is allocated or launched"""
    for c in G.CASES:
        mode, va, vb, buf = picked[c.name]
        assert mode == c.mode and buf == c.buf, (c.row(), mode, va, vb, buf)
        assert (mode == 0) or (va == 4 and vb == 4), c.row()


def test_every_kernel_and_every_extent_is_reached(picked):
    kernels = collections.Counter((c.kernel, picked[c.name][0]) for c in G.CASES)
    want = {(k, m) for k in ("NT", "NN", "TN", "TT", "HIDDEN", "MASK", "MASKP") for m in range(3)}   # the 21 instantiations
    assert set(kernels) == want, want - set(kernels)
    for form in G.FORMS:
        for mode in range(3):
            mine = [c for c in G.CASES if c.form == form and picked[c.name][0] == mode and not c.real]
            assert {c.M for c in mine} >= set(G.MS) and {c.N for c in mine} >= set(G.NS) and {c.K for c in mine} >= set(G.KS), (form, mode)
    # wide.h's buffer-mode launches (TN split, HIDDEN, MASK and MASKP with the column sums) and plain TT
    assert any(c.mode == 2 and c.form == "TN" and c.splits > 1 for c in G.CASES)
    assert any(c.mode == 2 and c.epi == "mask" and c.extsum for c in G.CASES) and any(c.mode == 2 and c.epi == "maskp" and c.extsum for c in G.CASES)
    assert any(c.mode == 2 and c.form == "TT" for c in G.CASES)
    assert {(c.mode, c.extsum) for c in G.CASES if c.epi == "mask"} == {(m, e) for m in range(3) for e in (False, True)}
    assert {(c.mode, c.M) for c in G.CASES if c.extsum and c.epi == "mask"} >= {(m, M) for m in range(3) for M in (1, 127, 129, 257)}


def test_every_load_flavour_and_store_path_is_reached(picked):
    fa, fb, straddle = set(), set(), set()
    for c in G.CASES:
        mode, va, vb, _ = picked[c.name]
        if mode == 0:
            a, b = G.load_flavours(c, va, vb)
            fa |= {(c.form, f) for f in a}
            fb |= {(c.form, f) for f in b}
            for op, vec, got in (("A", va, a), ("B", vb, b)):
                if vec > 1 and got == {1, vec}:
                    straddle.add((c.form, op, vec))     # scalar loads on the straddling tile, vectors elsewhere
    every = {(f, v) for f in G.FORMS for v in (4, 2, 1)}
    assert fa == every and fb == every, (every - fa, every - fb)
    assert straddle >= {(f, op, v) for f in G.FORMS for op in "AB" for v in (4, 2)}, straddle
    for kernel in ("NT", "NN", "TN", "TT", "HIDDEN", "MASK", "MASKP"):
        vc = set().union(*(G.store_paths(c)[0] for c in G.CASES if c.kernel == kernel))
        assert vc == {True, False}, kernel
    for kernel in ("MASK", "MASKP"):
        vm = set().union(*(G.store_paths(c)[1] for c in G.CASES if c.kernel == kernel))
        assert vm == {True, False}, kernel
    # the XCD re-deal: taken and not taken, each with more than one tile
    multi = [c for c in G.CASES if c.tiles[0] * c.tiles[1] > 1]
    assert {G.redealt(c) for c in multi} == {True, False}
    assert {c.tiles for c in G.CASES if c.group == "split"} >= {(2, 2, 2), (3, 2, 4), (3, 1, 3)}
    # split contraction: the lengths, a last slice shorter than one k-step, the slice-sum kernel around its block
    split = [c for c in G.CASES if c.group == "split" and not c.splitk]
    assert {(c.K, c.kps) for c in split} >= {(K, k) for K in (129, 513, 2064) for k in (16, 128, 512)}
    assert any(0 < c.K - (c.splits - 1) * c.kslice < G.BK for c in split)
    assert {c.M * c.N for c in G.CASES if c.splitk} >= {1, 255, 256, 257}
    # HIDDEN: every C_in with every ext_copy, both store paths, both M
    hid = [c for c in G.CASES if c.epi == "hidden"]
    assert {(c.C_in, c.ext_copy) for c in hid} >= {(C, e) for C in (1, 2, 3) for e in (0, 1 + C, 1 + C + 3)}
    assert {c.M for c in hid} >= {1, 129}
    assert {(c.N % 4 == 0 and c.ldc % 4 == 0 and c.offC == 0, c.mode) for c in hid} == {(v, m) for v in (True, False) for m in range(3)}
    # MASK: the padding columns at every N, aligned and scalar mask reads
    msk = [c for c in G.CASES if c.epi == "mask" and not c.extsum]
    assert {(c.N, c.c_zero_to) for c in msk} == {(N, 132) for N in (129, 130, 131)}
    assert {(c.mask_ld % 4 != 0, c.mask_off) for c in msk} == {(False, 0), (True, 0), (False, 1)}


def test_buffer_mode_falls_back_at_2_gib(lib):
    """32-bit byte offsets: an operand of 2 GiB or more leaves buffer mode for plain V4 (sizes only; nothing is allocated)"""
    base = next(c for c in G.CASES if c.mode == 2 and c.form == "NT" and c.epi == "store" and c.splits == 1)
    for over, want in ((dict(M=(1 << 19) - 1, lda=1024), (2, 1)), (dict(M=1 << 19, lda=1024), (1, 0)), (dict(N=1 << 19, ldb=1024), (1, 0)),
                       (dict(N=(1 << 19) - 1, ldb=1024), (2, 1))):
        c = dataclasses.replace(base, K=16, **over)
        a = G.fill_args(base, G.fake_addresses(base))
        a.M, a.N, a.K, a.lda, a.ldb, a.k_per_split = c.M, c.N, c.K, c.lda, c.ldb, 16
        buf = ctypes.c_int(-1)
        mode = lib.gemm_shim_pick_mode(ctypes.byref(a), None, None, ctypes.byref(buf))
        assert (mode, buf.value) == want, over


def test_integer_references_are_exact_in_float32():
    """the condition under which equality is the right comparison: no sum of absolute values of the terms of any sum the kernel takes
    reaches 2^24 (so no partial sum in any order does), and every input is an integer in [-3, 3]"""
    for c in G.CASES:
        m = G.materialise(c)
        if c.real:
            continue
        for key in ("A", "B", "bias", "skip", "ext") + (("mask",) if c.epi == "mask" else ()):
            if key in m:
                v = m[key].view()
                assert bool((v == v.round()).all()) and float(v.abs().max()) <= 3, (c.row(), key)
        assert G.reference(c)["max_intermediate"] < 2 ** 24, c.row()


def _plain(c):
    """the operation in float64, operands taken out of the allocations by their strides"""
    m = G.materialise(c)

    def mat(key, rows, cols, ld):
        return m[key].flat.as_strided((rows, cols), (ld, 1), m[key].base).double()
    A = mat("A", c.K, c.M, c.lda).t() if c.tA else mat("A", c.M, c.K, c.lda)
    B = mat("B", c.N, c.K, c.ldb).t() if c.tB else mat("B", c.K, c.N, c.ldb)
    if c.splitk or c.epi == "store":
        ks = [(0, c.K)] if c.splitk else [(z * c.kslice, min(c.K, (z + 1) * c.kslice)) for z in range(c.splits)]
        return [torch.matmul(A[:, lo:hi], B[lo:hi]) for lo, hi in ks], A, B
    P = torch.matmul(A, B)
    if c.epi == "hidden":
        x = mat("ext", c.M, 1 + c.C_in, c.ext_ld)
        P = torch.relu(P + mat("bias", 1, c.N, c.N) + x[:, 1:] @ mat("skip", c.N, c.C_in, c.C_in).t())
        P = torch.cat([P, x, torch.zeros(c.M, 3)], dim=1)[:, :c.N + c.ext_copy]
    elif c.epi == "mask":
        P = torch.where(mat("mask", c.M, c.N, c.mask_ld) > 0, P, torch.zeros(()).double())
    else:
        z = mat("mask", c.M, c.N, c.mask_ld)
        P = P * (-torch.sin(z) if c.mask_act == G.ACT_COS else c.omega * torch.cos(c.omega * z))
    return [P], A, B


def test_references_agree_with_plain_float64():
    for c in G.CASES:
        ref, m = G.reference(c), G.materialise(c)
        slices, A, B = _plain(c)
        C = m["C"]
        seen = torch.zeros_like(ref["C_def"])
        for z, P in enumerate(slices):
            idx = C.base + z * c.c_stride + torch.arange(c.M)[:, None] * c.ldc + torch.arange(P.shape[1])[None, :]
            got = ref["C"][idx]
            seen[idx.reshape(-1)] = True
            if c.real:
                assert torch.allclose(got, P, rtol=0, atol=1e-12 * float(P.abs().max())), c.row()
            elif c.epi == "maskp":   # the factors are 0 or +-1 (x omega) up to the float32 rounding of the quarter turns
                assert bool(((got - P).abs() <= 1e-5 * max(1.0, c.omega) * torch.matmul(A, B).abs()).all()), c.row()
            else:
                assert torch.equal(got, P), c.row()
        if c.c_zero_to > c.N:
            idx = C.base + torch.arange(c.M)[:, None] * c.ldc + torch.arange(c.N, c.c_zero_to)[None, :]
            assert bool((ref["C"][idx] == 0).all()), c.row()
            seen[idx.reshape(-1)] = True
        assert torch.equal(seen, ref["C_def"]), c.row()                   # nothing else is defined
        assert bool(torch.isnan(ref["C"][~ref["C_def"]]).all()), c.row()
        if c.real:   # the bar: 2 k 2^-24 (|A| . |B|) over the slice
            lo, hi = 0, (c.K if c.splitk else min(c.K, c.kslice))
            idx = C.base + torch.arange(c.M)[:, None] * c.ldc + torch.arange(c.N)[None, :]
            assert torch.allclose(ref["C_tol"][idx], 2 * (hi - lo) * 2.0 ** -24 * (A[:, lo:hi].abs() @ B[lo:hi].abs()), rtol=1e-12), c.row()
        if c.extsum and c.epi == "mask":
            x1 = m["ext"].view().double().clone()
            x1[:, 0] = 1.0
            E = torch.stack([slices[0][t * G.BM:(t + 1) * G.BM].t() @ x1[t * G.BM:(t + 1) * G.BM] for t in range(c.tiles[1])])
            assert torch.equal(ref["E"], E.reshape(-1)), c.row()


def test_check_notices_a_wrong_element_and_a_touched_guard():
    """the comparison itself: the expected allocation passes; one element off by one, one guard element written, fail"""
    for c in (G.group("NT")[5], G.group("hidden")[7], G.group("mask")[2]):
        ref, m = G.reference(c), G.materialise(c)
        good = m["C"].flat.clone()
        good[ref["C_def"]] = ref["C"][ref["C_def"]].float()
        assert G.check(c, good) == []
        off = good.clone()
        off[int(torch.nonzero(ref["C_def"])[-1])] += 1.0
        assert len(G.check(c, off)) == 1
        touched = good.clone()
        touched[int(torch.nonzero(~ref["C_def"])[0])] = 0.0
        assert len(G.check(c, touched)) == 1
        assert bool((m["C"].flat.view(torch.int32) == G.PATTERN).all())   # the shared case itself is unchanged


@pytest.mark.parametrize("what,code,over", G.REJECTIONS, ids=[r[0] for r in G.REJECTIONS])
def test_rejections(lib, what, code, over):
    """refused on the host before any launch: the pointers are made up"""
    base = next(c for c in G.CASES if c.form == over.get("form", "NT") and c.epi == "store" and c.mode == 1 and c.splits == 1)
    c = dataclasses.replace(base, name="rejected: " + what, mask_ld=base.N, ext_ld=4, C_in=2, **over)
    a = G.fill_args(base, G.fake_addresses(base))
    for f in ("tA", "tB", "M", "N", "K", "buf", "padA", "padB"):
        setattr(a, f, getattr(c, f))
    a.k_per_split, a.epi, a.mask_ld, a.ext_ld, a.C_in = c.kps, G.EPI[c.epi], c.mask_ld, c.ext_ld, c.C_in
    assert lib.gemm_shim_launch(ctypes.byref(a)) == code


def test_gemm_rm_splitk_rejects_without_a_launch(lib):
    assert lib.gemm_shim_splitk(1, 0, 0, 16, 64, 0x1000, 16, 0x2000, 16, 0x3000, 0x4000) == G.INR_EINVAL
    assert lib.gemm_shim_splitk(0, 0, 16, 16, -1, 0x1000, 16, 0x2000, 16, 0x3000, 0x4000) == G.INR_EINVAL
