"""The cases of tests/step2_cases.py on the CPU, with no kernel of this project involved: their inputs are conditioned (no ReLU
pre-activation within 4 x the float32 forward error bound of zero), they are deterministic, and a correct float32 evaluation (plain
CPU torch, the oracle's own functions on the float32 parameters) meets EVERY bar of tests/test_gpu_step2_chunks.py against the float64
reference - so the bars are reachable before any GPU is involved; and the gradient bar sees ONE lost point."""
import numpy as np
import pytest
import torch

from tests import step2_cases as S

ALL = [(h, C, name) for h, C in S.SHAPES for name in S.LAUNCHES]


@pytest.mark.parametrize("h,C,name", ALL)
def test_case_is_conditioned_and_deterministic(h, C, name):
    c = S.case(h, C, name)
    ratio, bmax, pmin = S.assert_conditioned(c)
    n = c["coords"].shape[1]
    print(f"h {h} C {C} {name}: {c['redrawn']} of {n} points redrawn in {c['rounds']} rounds; min |pre| / b {ratio:.2f}, max b {bmax:.1e}, "
          f"min |pre| {pmin:.1e}")
    assert tuple(c["coords"].shape) == (C, S.LAUNCHES[name][1]) and c["spec"].n_layers == 2
    again = S.build_case(h, C, name)
    for k in ("coords", "un", "hard", "dlog"):
        assert torch.equal(c[k], again[k]), k
    for k, v in c["p"].items():
        assert torch.equal(v, again["p"][k]) and bool((v != 0).all()), k
    # what the redraw is for: float32 torch takes every unit of every point on the float64 side
    z64 = [pre > 0 for pre, _ in S.preact_bounds(S.f64(c["p"]), c["coords"].double().t())]
    z32 = [pre > 0 for pre, _ in S.preact_bounds(c["p"], c["coords"].t())]
    assert sum(int((a != b).sum()) for a, b in zip(z64, z32)) == 0


def test_two_image_cases_are_conditioned():
    for h, C in [(130, 2), (64, 2)]:
        for im in (0, 1):
            S.assert_conditioned(S.case(h, C, "two_images", im))
        assert not torch.equal(S.case(h, C, "two_images", 0)["coords"], S.case(h, C, "two_images", 1)["coords"])


@pytest.mark.parametrize("h,C,name", ALL)
def test_float32_torch_meets_the_loss_and_gradient_bars(h, C, name):
    c = S.case(h, C, name)
    lo, go = S.ref(c, S.loss_and_grads, "se", "none")
    l32, g32 = S.loss_and_grads(c, "se", "none", torch.float32)
    print(f"h {h} C {C} {name}: loss rel err {abs(l32 - lo) / abs(lo):.2e}")
    S.assert_tensors(g32, go, S.GRAD_BAR, f"h {h} C {C} {name} float32 torch")
    assert l32 == pytest.approx(lo, rel=1e-5)
    y64, y32 = S.ref(c, S.logits), S.logits(c, torch.float32)
    np.testing.assert_allclose(y32.numpy(), y64.numpy(), atol=5e-6, rtol=1e-5)


@pytest.mark.parametrize("name", list(S.LAUNCHES))
@pytest.mark.parametrize("h,C", [(130, 2), (64, 3)])
def test_float32_torch_meets_the_bce_bars(h, C, name):
    c = S.case(h, C, name)
    lo, go = S.ref(c, S.loss_and_grads, "bce", "sssdms")
    l32, g32 = S.loss_and_grads(c, "bce", "sssdms", torch.float32)
    S.assert_tensors(g32, go, S.GRAD_BAR, f"h {h} C {C} {name} bce float32 torch")
    assert l32 == pytest.approx(lo, rel=1e-5)


@pytest.mark.parametrize("name", list(S.LAUNCHES))
@pytest.mark.parametrize("h,C", S.COMPILED)
def test_float32_torch_meets_the_coordinate_gradient_bars(h, C, name):
    c = S.case(h, C, name)
    (gref, xref), (g32, x32) = S.ref(c, S.vjp), S.vjp(c, torch.float32)
    S.assert_tensors(g32, gref, S.GRAD_BAR, f"h {h} C {C} {name} vjp float32 torch")
    S.assert_tensors({"dcoords": x32}, {"dcoords": xref}, S.DCOORDS_BAR, f"h {h} C {C} {name} float32 torch")


@pytest.mark.parametrize("h,C,name", [(130, 2, "two_and_one"), (64, 2, "three_each")])
def test_float32_torch_meets_the_trajectory_bars(h, C, name):
    c = S.case(h, C, name)
    (pf, losses), (p32, l32) = S.ref(c, S.trajectory), S.trajectory(c, 10, torch.float32)
    print(f"loss curve max rel err {float(np.abs(np.asarray(l32) / np.asarray(losses) - 1).max()):.2e}")
    for k, want in pf.items():
        print(f"   {k}: max |err| {float((p32[k].double() - want).abs().max()):.2e}")
    np.testing.assert_allclose(np.asarray(l32), np.asarray(losses), rtol=2e-5)
    for k, want in pf.items():
        np.testing.assert_allclose(p32[k].numpy(), want.numpy(), rtol=2e-4, atol=5e-6, err_msg=k)


@pytest.mark.parametrize("kind", ["fourier", "sine"])
def test_encode_cases(kind):
    c = S.encode_case(kind)
    S.assert_conditioned(c)
    assert c["spec"].n_layers == 2 and c["spec"].act0 == ("cos" if kind == "fourier" else "sin")
    (lo, go), (l32, g32) = S.ref(c, S.encode_loss_and_grads), S.encode_loss_and_grads(c, torch.float32)
    S.assert_tensors(g32, go, S.ENCODE_BAR, f"{kind} float32 torch")
    assert l32 == pytest.approx(lo, rel=1e-4)


@pytest.mark.parametrize("kind", ["cdn", "pcn"])
def test_composite_cases(kind):
    """The conditioning holds behind the float64 deformation with the flow kernels' own bar as the error of the ICNN's inputs, and
    float32 torch meets the composite's bars."""
    c = S.composite_case(kind)
    S.assert_conditioned(c)
    (lo, go, xd, y), (l32, g32, xd32, y32) = S.ref(c, S.composite_loss_and_grads), S.composite_loss_and_grads(c, torch.float32)
    bar, xbar = (S.CDN_BAR, S.CDN_XD) if kind == "cdn" else (S.PCN_BAR, S.PCN_XD)
    S.assert_tensors(g32, go, bar, f"{kind} float32 torch")
    assert l32 == pytest.approx(lo, rel=2e-5 if kind == "cdn" else 3e-5)
    np.testing.assert_allclose(xd32.numpy(), xd.numpy(), **xbar)
    assert all(float(g.abs().max()) > 0 for k, g in go.items() if k.startswith(("convex_net.", "linear.")))


def test_the_gradient_bar_sees_one_lost_point():
    """three_each's last chunk holds ONE point.  A kernel that lost it (the float64 gradient without that point's term) misses some
    tensor's bar by more than 100 x, at every shape."""
    for h, C in S.SHAPES:
        c = S.case(h, C, "three_each")
        _, go = S.ref(c, S.loss_and_grads, "se", "none")
        lost = S.grads_without_last_point(c)
        use = {k: S.bar_use(lost[k], go[k], **S.GRAD_BAR) for k in go}
        print(f"h {h} C {C}: one lost point uses {max(use.values()):.0f} x the bar ({max(use, key=use.get)})")
        assert max(use.values()) > 100.0
