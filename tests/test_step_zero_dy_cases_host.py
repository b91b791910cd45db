"""The cases of tests/step_zero_dy_cases.py on the CPU, with no kernel of this project involved: the patterns put their zeros where
their names say, the saturation cases are conditioned and saturate exactly the intended points in float32 torch (logits >= 40 there,
|logit| <= 5 elsewhere), a correct float32 evaluation meets every bar of tests/test_gpu_step_zero_dy.py against the float64 reference,
the trajectory crosses the float32 threshold - and the gradient bar sees what the skip's two likely faults would do."""
import numpy as np
import pytest
import torch

from tests import step2_cases as S
from tests import step_l0_cases as Z
from tests import step_zero_dy_cases as Y


def test_patterns_mark_what_they_say():
    n = Z.LAUNCHES["three_each"][1]
    whole = {"first": [0], "middle": [2], "last": [4], "two_consecutive": [0, 2], "two_consecutive_late": [3, 5], "alternating": [0, 3, 4],
             "ragged": [5]}
    for pat, chunks in whole.items():
        c = Y.pattern_case(130, 2, "three_each", pat)
        assert Y.dead_chunks(c["dlog"]) == chunks, pat
        assert int((c["dlog"] == 0).sum()) == int(c["zero"].sum()) == sum(min(64, n - 64 * k) for k in chunks)
    for w in range(4):
        c = Y.pattern_case(130, 2, "three_each", f"one_live_w{w}")
        z = (c["dlog"] == 0).reshape(-1)[128:192].reshape(4, 16)
        assert Y.dead_chunks(c["dlog"]) == [] and [int(v) for v in z.sum(1)] == [16 - (k == w) for k in range(4)]
        c = Y.pattern_case(130, 2, "three_each", f"tile_w{w}")
        z = (c["dlog"] == 0).reshape(-1)[128:192].reshape(4, 16)
        assert [int(v) for v in z.sum(1)] == [16 * (k == w) for k in range(4)] and int((c["dlog"] == 0).sum()) == 16
    c = Y.pattern_case(130, 2, "three_each", "neg_zero")
    assert bool(torch.signbit(c["dlog"][c["zero"]]).all()) and Y.dead_chunks(c["dlog"]) == [0, 3]
    assert Y.dead_chunks(Y.pattern_case(130, 2, "three_each", "all")["dlog"]) == [0, 1, 2, 3, 4, 5]
    for pat, chunks in {"first": [0, 1, 2], "second": [8, 9], "ragged": [10]}.items():
        assert Y.dead_chunks(Y.pattern_case(130, 2, "two_and_one", pat)["dlog"]) == chunks
    # the case it is derived from is left as it was
    assert int((Z.case(130, 2, "three_each")["dlog"] == 0).sum()) == 0


@pytest.mark.filterwarnings("ignore:invalid value encountered in divide")   # (the printed share of a bar whose reference is all zero)
@pytest.mark.parametrize("name,pattern", Y.PATTERNS)
@pytest.mark.parametrize("h,C", Y.SHAPES)
def test_float32_torch_meets_the_pattern_bars(h, C, name, pattern):
    c = Y.pattern_case(h, C, name, pattern)
    (gref, xref), (g32, x32) = S.ref(c, S.vjp), S.vjp(c, torch.float32)
    tag = f"h {h} C {C} {name} {pattern} float32 torch"
    S.assert_tensors(g32, gref, S.GRAD_BAR, tag)
    S.assert_tensors({"dcoords": x32}, {"dcoords": xref}, S.DCOORDS_BAR, tag)
    assert int((xref[:, c["zero"]] != 0).sum()) == 0
    if pattern == "all":
        assert all(int((v != 0).sum()) == 0 for v in gref.values())


@pytest.mark.parametrize("name", Y.SAT_LAUNCHES)
@pytest.mark.parametrize("h,C", Y.SHAPES)
def test_saturation_cases(h, C, name):
    c = Y.sat_case(h, C, name)
    S.assert_conditioned(c)
    assert all(bool((v != 0).all()) for v in c["p"].values())
    assert Y.dead_chunks(c["sat"].logical_not().float()) == ([0, 3, 5] if name == "three_each" else [1, 8, 10])
    for kind in ("se", "bce"):
        for dtype in (torch.float32, torch.float64):
            dy, y = Y.dl_dlogit(c, kind, dtype)
            assert float(y[c["sat"]].min()) >= Y.SAT_MIN and float(y[~c["sat"]].abs().max()) <= Y.LIVE_MAX
            assert torch.equal(dy == 0, c["sat"]), (kind, dtype)      # zero on exactly the intended points
        lo, go = S.ref(c, Y.sat_loss_and_grads, kind)
        l32, g32 = Y.sat_loss_and_grads(c, kind, torch.float32)
        S.assert_tensors(g32, go, S.GRAD_BAR, f"h {h} C {C} {name} {kind} float32 torch")
        assert l32 == pytest.approx(lo, rel=1e-5)


def test_sine_pattern_case():
    c = Y.sine_pattern_case()
    S.assert_conditioned(c)
    assert Y.dead_chunks(c["dlog"]) == [8, 9] and int((c["dlog"] == 0).sum()) == 128 + 16
    S.assert_tensors(Y.encode_vjp(c, torch.float32), S.ref(c, Y.encode_vjp), S.ENCODE_BAR, "sine float32 torch")


def test_nan_case():
    c = Y.nan_case()
    dy, y = Y.dl_dlogit(c, "se")
    assert int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(dy[37]))
    rest = torch.ones(64, dtype=torch.bool)
    rest[37] = False
    assert int((dy[:64][rest] != 0).sum()) == 0


def test_trajectory_crosses_the_threshold():
    """float32 torch: no zero dL/dlogit at the start, no chunk without a gradient after two steps, chunks 0, 3 and 5 without one after
    twelve; and float32 meets the trajectory's bars against float64"""
    c = Y.traj_case()
    S.assert_conditioned(c)
    dy0, y0 = Y.dl_dlogit(c, "se")
    assert Y.dead_chunks(dy0) == [] and int((dy0 == 0).sum()) == 0
    assert float(y0[c["near"]].max()) < Y.THRESHOLD - 1.0 and float(y0[~c["near"]].abs().max()) <= Y.LIVE_MAX
    for steps, dead in ((2, []), (12, [0, 3, 5])):
        pk = Y.trajectory(c, steps, torch.float32)[0]
        assert Y.dead_chunks(Y.dl_dlogit(dict(c, p=pk), "se")[0]) == dead, steps
    (pf, losses, _), (p32, l32, _) = S.ref(c, Y.trajectory), Y.trajectory(c, Y.TRAJ_STEPS, torch.float32)
    np.testing.assert_allclose(np.asarray(l32), np.asarray(losses), rtol=2e-5)
    for k, want in pf.items():
        np.testing.assert_allclose(p32[k].numpy(), want.numpy(), rtol=2e-4, atol=5e-6, err_msg=k)


def test_the_gradient_bar_sees_stale_rows_and_a_skipped_live_chunk():
    """What the two likely faults would do, in float64.  (a) A skipped wave that stages nothing: the live waves of its chunk multiply the
    dz1 rows it staged one chunk earlier - here chunk 2's tile `w` summed with chunk 0's dL/dlogit.  (b) Flag words read from the wrong
    chunk: a live chunk's backward pass is dropped.  Either misses some tensor's bar by more than 100 x."""
    c = Y.pattern_case(130, 2, "three_each", "tile_w1")
    gref, _ = S.ref(c, S.vjp)
    stale = c["dlog"].clone()
    stale[128 + 16:128 + 32] = c["dlog"][16:32]
    dropped = c["dlog"].clone()
    dropped[256:320] = 0.0
    for what, dlog in (("stale rows", stale), ("a dropped chunk", dropped)):
        g, _ = S.vjp(dict(c, dlog=dlog))
        use = {k: S.bar_use(g[k], gref[k], **S.GRAD_BAR) for k in gref}
        print(f"{what}: {max(use.values()):.0f} x the bar ({max(use, key=use.get)})")
        assert max(use.values()) > 100.0
