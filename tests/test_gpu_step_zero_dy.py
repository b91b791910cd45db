"""GPU parity of the L = 1 step kernel where it skips work whose every term is an exact zero (icnn_step.h, icnn_step_bwd.h, DESIGN.md
4.1): a wave whose 16 dL/dlogit are all +-0 stages zeros and skips its backward block, and a chunk in which no wave has a non-zero
dL/dlogit skips the dW phase and the chunk-end barrier.  What can go wrong there: a skipped wave that leaves the previous chunk's dz1
rows in the stage for the three live waves to multiply; the four flag words of one chunk overwritten by a wave that has run ahead into
the next (no chunk-end barrier holds it back); a live wave or a NaN taken for zero; dcoords left unwritten; a stage overwritten under a
slower wave's reads once the barrier is gone.  The method is that of tests/test_gpu_step_l0_under_dw.py: tiny launches, the slab base
set by hand (inrfit_debug_set_slab_base), the float64 CPU oracle as checker, and every launch a second time on NaN-filled workspaces
and outputs with equal bits.  Cases and patterns: tests/step_zero_dy_cases.py; that float32 torch meets every bar on them and that the
zeros are where they are meant to be: tests/test_step_zero_dy_cases_host.py.

Bars: those of tests/step2_cases.py, unchanged - loss rel 1e-5, gradients rel 2e-4 + 2e-6 max|g|, coordinate gradients rel 2e-4 +
2e-6 max|g|, the encode net's gradients 3e-3; the trajectory's as in test_gpu_step2_chunks.py (losses rel 2e-5, parameters rel 2e-4 +
5e-6).  On top: where the float64 gradient is exactly zero the device's is exactly zero."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import step2_cases as S  # noqa: E402  (references, bars, figures)
from tests import step_zero_dy_cases as Y  # noqa: E402
from tests.test_gpu_step_l0_under_dw import _dev_inputs, _two_runs, amd, launch  # noqa: E402,F401  (the same launches and runs)


def assert_exact_zeros(got, want, tag):
    """wherever the float64 reference is exactly zero, so is the device's value"""
    for k, r in want.items():
        z = np.asarray(r) == 0
        bad = int((np.asarray(got[k])[z] != 0).sum())
        print(f"   {tag} {k}: {int(z.sum())} exact zeros in the reference, {bad} of them non-zero on the device")
        assert bad == 0, (tag, k)


@pytest.mark.parametrize("name,pattern", Y.PATTERNS)
@pytest.mark.parametrize("h,C", Y.SHAPES)
def test_exact_zero_patterns(amd, h, C, name, pattern):
    """the vector-Jacobian product with zeros written into dL/dlogit"""
    A = amd
    c = Y.pattern_case(h, C, name, pattern)
    dev, flat, grid = _dev_inputs(A, c)
    gref, _ = S.ref(c, S.vjp)
    with launch(A, name):
        (g,) = _two_runs(A, lambda: (A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev)),))
    got = A.unpack_params(c["spec"], g[0].cpu())
    tag = f"h {h} C {C} {name} {pattern}"
    if pattern == "all":
        assert int((g != 0).sum()) == 0
    S.assert_tensors(got, gref, S.GRAD_BAR, tag)
    assert_exact_zeros(got, gref, tag)


@pytest.mark.parametrize("kind", ["se", "bce"])
@pytest.mark.parametrize("name", Y.SAT_LAUNCHES)
@pytest.mark.parametrize("h,C", Y.SHAPES)
def test_natural_saturation(amd, h, C, name, kind):
    """zeros that the float32 sigmoid makes: whole chunks, a ragged chunk and one wave tile at logits >= 40"""
    A = amd
    c = Y.sat_case(h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    lo, go = S.ref(c, Y.sat_loss_and_grads, kind)
    tgt = (c["un_bce"] if kind == "bce" else c["un"])[None].to(dev)
    with launch(A, name):
        loss, g = _two_runs(A, lambda: A.loss_grad(c["spec"], flat, grid, tgt, loss=kind))
    got = A.unpack_params(c["spec"], g[0].cpu())
    tag = f"h {h} C {C} {name} {kind}"
    print(f"{tag}: loss rel err {abs(float(loss[0]) - lo) / abs(lo):.2e}")
    S.assert_tensors(got, go, S.GRAD_BAR, tag)
    assert_exact_zeros(got, go, tag)
    assert float(loss[0]) == pytest.approx(lo, rel=1e-5)


def test_a_nan_logit_in_a_zero_chunk_still_poisons_the_gradients(amd):
    """63 saturated points and one NaN logit in a chunk: NaN is not zero, the chunk runs, loss and gradients are non-finite"""
    A = amd
    c = Y.nan_case()
    dev, flat, grid = _dev_inputs(A, c)
    runs = []
    try:
        with launch(A, "three_each"):
            for poison in (False, True):
                A._lib.POISON = poison
                runs.append(A.loss_grad(c["spec"], flat, grid, c["un"][None].to(dev), loss="se"))
    finally:
        A._lib.POISON = False
    (loss, g), (loss2, g2) = runs
    assert torch.equal(g.view(torch.int32), g2.view(torch.int32)) and torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
    got = A.unpack_params(c["spec"], g[0].cpu())
    print({k: int((~torch.isfinite(v)).sum()) for k, v in got.items()})
    assert not bool(torch.isfinite(loss).all())
    # (the output layer's sums take dy itself; below it the point's own relu masks, NaN > 0 being false, may stop the NaN)
    for k in ("out.ln.bias", "out.ln.weight", "out.skp.weight"):
        assert not bool(torch.isfinite(got[k]).any()), k


def test_two_images_in_one_launch(amd):
    """two images, two workgroups of three chunks each: image 0 with `two_consecutive`, image 1 with `alternating` - each image's
    flag words are its own workgroups', each judged against its own float64 reference"""
    A = amd
    dev = torch.device("cuda:0")
    cs = [Y.pattern_case(130, 2, "two_images", pat, im) for im, pat in enumerate(("two_consecutive", "alternating"))]
    spec = cs[0]["spec"]
    flat = torch.stack([A.pack_state_dict(spec, c["p"], dev) for c in cs]).contiguous()
    grid = A.Grid.explicit(torch.stack([c["coords"] for c in cs]).to(dev))
    dlog = torch.stack([c["dlog"] for c in cs]).to(dev)
    with launch(A, "two_images", 2):
        (g,) = _two_runs(A, lambda: (A.icnn.backward(spec, flat, grid, dlog),))
    for im, c in enumerate(cs):
        gref, _ = S.ref(c, S.vjp)
        got = A.unpack_params(spec, g[im].cpu())
        S.assert_tensors(got, gref, S.GRAD_BAR, f"two images, image {im}")
        assert_exact_zeros(got, gref, f"two images, image {im}")


@pytest.mark.filterwarnings("ignore:invalid value encountered in divide")   # (the printed share of a bar whose reference is all zero)
@pytest.mark.parametrize("h,C,name,pattern", [(130, 2, "three_each", "alternating"), (130, 2, "three_each", "all"),
                                              (64, 2, "two_and_one", "second"), (100, 2, "three_each", "one_live_w2"),
                                              (130, 3, "three_each", "two_consecutive_late")])
def test_coordinate_gradient_kernel(amd, h, C, name, pattern):
    """the DX instantiations keep their backward block dense and skip only the dW phase: dcoords is written for every valid point (the
    NaN-filled second run has none left), and is exactly zero where dL/dlogit is"""
    A = amd
    c = Y.pattern_case(h, C, name, pattern)
    dev, flat, grid = _dev_inputs(A, c)
    gref, xref = S.ref(c, S.vjp)
    with launch(A, name):
        g, dco = _two_runs(A, lambda: A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev), want_dcoords=True))
    tag = f"h {h} C {C} {name} {pattern} dx"
    got = A.unpack_params(c["spec"], g[0].cpu())
    S.assert_tensors(got, gref, S.GRAD_BAR, tag)
    S.assert_tensors({"dcoords": dco[0].cpu()}, {"dcoords": xref}, S.DCOORDS_BAR, tag)
    assert_exact_zeros(got, gref, tag)
    assert_exact_zeros({"dcoords": dco[0].cpu()}, {"dcoords": xref}, tag)
    assert int((dco[0].cpu()[:, c["zero"]] != 0).sum()) == 0


def test_sine_encode_net(amd):
    """a sin layer 0 (its own instantiation), two_and_one: the second chunks of workgroups 0 and 1 and one wave tile zero"""
    A = amd
    dev = torch.device("cuda:0")
    c = Y.sine_pattern_case()
    go = S.ref(c, Y.encode_vjp)
    flat, grid = c["flat"][None].to(dev).contiguous(), A.Grid.explicit(c["coords"].to(dev))
    with launch(A, "two_and_one"):
        (g,) = _two_runs(A, lambda: (A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev)),))
    got = {k: v for k, v in A.unpack_params(c["spec"], g[0].cpu()).items() if k in go}
    S.assert_tensors(got, go, S.ENCODE_BAR, "sine")


def test_adam_clamp_trajectory_across_the_threshold(amd):
    """25 Adam + clamp steps during which three chunks saturate: one 25-step fit = 25 one-step fits bit for bit, plain and NaN-filled
    workspaces alike, and losses and parameters against the oracle's float64 trajectory"""
    A = amd
    c = Y.traj_case()
    dev, flat, grid = _dev_inputs(A, c)
    un = c["hard"][None].to(dev)
    pf, losses, _ = S.ref(c, Y.trajectory)
    with launch(A, "three_each"):
        params_w, loss_w = _two_runs(A, lambda: (lambda f: (f.params, f.loss_hist))(
            A.fit(c["spec"], flat.clone(), grid, un, Y.TRAJ_STEPS, lr=2e-3, want_logits=False)))
        params, opt, hist = flat.clone(), A.icnn.new_opt_state(c["spec"], 1, dev), []
        for k in range(Y.TRAJ_STEPS):
            one = A.fit(c["spec"], params, grid, un, 1, lr=2e-3, opt_state=opt, step0=k, want_logits=False)
            params, opt = one.params, one.opt_state
            hist.append(one.loss_hist[:, 0].clone())
        last = A.loss_grad(c["spec"], params, grid, un, loss="se")[1]
    assert torch.equal(params_w, params)
    assert torch.equal(loss_w, torch.stack(hist, dim=1))
    got_l = loss_w[0].cpu().numpy().astype(np.float64)
    got = A.unpack_params(c["spec"], params_w[0].cpu())
    print(f"loss curve max rel err {float(np.abs(got_l / np.asarray(losses) - 1).max()):.2e}")
    for k, want in pf.items():
        print(f"   {k}: max |err| {float(np.abs(got[k].double().numpy() - want.numpy()).max()):.2e}")
    np.testing.assert_allclose(got_l, np.asarray(losses), rtol=2e-5)
    for k, want in pf.items():
        np.testing.assert_allclose(got[k].numpy(), want.numpy(), rtol=2e-4, atol=5e-6, err_msg=k)
    assert bool(torch.isfinite(last).all())
