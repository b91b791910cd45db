"""The cases of tests/step_l0_cases.py on the CPU, with no kernel of this project involved: their inputs are conditioned (no ReLU
pre-activation within 4 x the float32 forward error bound of zero), they are deterministic, and a correct float32 evaluation (plain
CPU torch, the oracle's own functions on the float32 parameters) meets EVERY bar of tests/test_gpu_step_l0_under_dw.py against the
float64 reference - so the bars are reachable before any GPU is involved; and the gradient bar sees ONE lost point."""
import numpy as np
import pytest
import torch

from tests import step2_cases as S
from tests import step_l0_cases as Z

ALL = [(h, C, name) for h, C in Z.SHAPES for name in Z.LAUNCHES]


@pytest.mark.parametrize("h,C,name", ALL)
def test_case_is_conditioned_and_deterministic(h, C, name):
    c = Z.case(h, C, name)
    ratio, bmax, pmin = S.assert_conditioned(c)
    n = c["coords"].shape[1]
    print(f"h {h} C {C} {name}: {c['redrawn']} of {n} points redrawn in {c['rounds']} rounds; min |pre| / b {ratio:.2f}, max b {bmax:.1e}, "
          f"min |pre| {pmin:.1e}")
    assert tuple(c["coords"].shape) == (C, Z.LAUNCHES[name][1]) and c["spec"].n_layers == 1
    again = Z.build_case(h, C, name)
    for k in ("coords", "un", "hard", "dlog"):
        assert torch.equal(c[k], again[k]), k
    for k, v in c["p"].items():
        assert torch.equal(v, again["p"][k]) and bool((v != 0).all()), k
    # what the redraw is for: float32 torch takes every unit of every point on the float64 side
    z64 = [pre > 0 for pre, _ in S.preact_bounds(S.f64(c["p"]), c["coords"].double().t())]
    z32 = [pre > 0 for pre, _ in S.preact_bounds(c["p"], c["coords"].t())]
    assert sum(int((a != b).sum()) for a, b in zip(z64, z32)) == 0
    # both sides of the layer-0 mask occur (a mask stuck at one value would not go unnoticed)
    on = float(z64[0].double().mean())
    assert 0.02 < on < 0.98, on


def test_two_image_cases_are_conditioned():
    for im in (0, 1):
        S.assert_conditioned(Z.case(130, 2, "two_images", im))
    assert not torch.equal(Z.case(130, 2, "two_images", 0)["coords"], Z.case(130, 2, "two_images", 1)["coords"])


@pytest.mark.parametrize("h,C,name", ALL)
def test_float32_torch_meets_the_loss_and_gradient_bars(h, C, name):
    c = Z.case(h, C, name)
    lo, go = S.ref(c, S.loss_and_grads, "se", "none")
    l32, g32 = S.loss_and_grads(c, "se", "none", torch.float32)
    print(f"h {h} C {C} {name}: loss rel err {abs(l32 - lo) / abs(lo):.2e}")
    S.assert_tensors(g32, go, S.GRAD_BAR, f"h {h} C {C} {name} float32 torch")
    assert l32 == pytest.approx(lo, rel=1e-5)


def test_float32_torch_meets_the_two_image_bars():
    for im in (0, 1):
        c = Z.case(130, 2, "two_images", im)
        lo, go = S.ref(c, S.loss_and_grads, "bce", "sssdms")
        l32, g32 = S.loss_and_grads(c, "bce", "sssdms", torch.float32)
        S.assert_tensors(g32, go, S.GRAD_BAR, f"two images, image {im} float32 torch")
        assert l32 == pytest.approx(lo, rel=1e-5)


@pytest.mark.parametrize("name", list(Z.LAUNCHES))
@pytest.mark.parametrize("h,C", [(130, 2), (64, 2), (100, 2)])
def test_float32_torch_meets_the_coordinate_gradient_bars(h, C, name):
    c = Z.case(h, C, name)
    (gref, xref), (g32, x32) = S.ref(c, S.vjp), S.vjp(c, torch.float32)
    S.assert_tensors(g32, gref, S.GRAD_BAR, f"h {h} C {C} {name} vjp float32 torch")
    S.assert_tensors({"dcoords": x32}, {"dcoords": xref}, S.DCOORDS_BAR, f"h {h} C {C} {name} float32 torch")


def test_sine_case():
    c = Z.sine_case()
    S.assert_conditioned(c)
    assert c["spec"].n_layers == 1 and c["spec"].act0 == "sin"
    (lo, go), (l32, g32) = S.ref(c, S.encode_loss_and_grads), S.encode_loss_and_grads(c, torch.float32)
    S.assert_tensors(g32, go, S.ENCODE_BAR, "sine float32 torch")
    assert l32 == pytest.approx(lo, rel=1e-4)


def test_the_gradient_bar_sees_one_lost_point():
    """three_each's last chunk holds ONE point.  A kernel that lost it (the float64 gradient without that point's term) misses some
    tensor's bar by more than 100 x, at every shape that runs on the fused kernel."""
    for h, C in [s for s in Z.SHAPES if s[0] <= 130]:
        c = Z.case(h, C, "three_each")
        _, go = S.ref(c, S.loss_and_grads, "se", "none")
        lost = S.grads_without_last_point(c)
        use = {k: S.bar_use(lost[k], go[k], **S.GRAD_BAR) for k in go}
        print(f"h {h} C {C}: one lost point uses {max(use.values()):.0f} x the bar ({max(use, key=use.get)})")
        assert max(use.values()) > 100.0


def test_the_input_gradient_bar_sees_a_stale_point():
    """What a layer-0 slice that ran behind the chunk-end barrier would do: it reads the coordinates of the NEXT chunk's points from the
    stage.  The float64 input-weight gradient with one chunk's coordinates replaced by the next one's (the masked dz0 unchanged)
    misses its bar by more than 100 x at the multi-chunk launches."""
    for name in Z.MULTI_CHUNK:
        c = Z.case(130, 2, name)
        p = {k: v.detach().double().requires_grad_(True) for k, v in c["p"].items()}
        x = c["coords"].double().t()
        pre = torch.nn.functional.linear(x, p["input.weight"], p["input.bias"])
        pre.retain_grad()
        out = torch.sigmoid(O_forward_from_pre(p, pre, x))
        ((c["un"].double() - out) ** 2).mean().backward()
        dz0 = pre.grad                                   # (N, h): what the backward product and the mask hand to the layer-0 sums
        want = dz0.t() @ x
        np.testing.assert_allclose(want.numpy(), p["input.weight"].grad.numpy(), rtol=1e-12, atol=1e-18)
        stale = x.clone()
        wgs = Z.LAUNCHES[name][2]
        stale[0:64] = x[64 * wgs:64 * wgs + 64]          # workgroup 0's first chunk summed with its second chunk's coordinates
        use = S.bar_use((dz0.t() @ stale).numpy(), want.numpy(), **S.GRAD_BAR)
        print(f"{name}: one chunk's stale coordinates use {use:.0f} x the bar of input.weight")
        assert use > 100.0


def O_forward_from_pre(p, pre, x):
    """the L = 1 ICNN's logits (N,) from its layer-0 pre-activation"""
    F = torch.nn.functional
    z0 = F.relu(pre)
    z1 = F.relu(F.linear(z0, p["skip.0.ln.weight"], p["skip.0.ln.bias"]) + F.linear(x, p["skip.0.skp.weight"]))
    return (F.linear(z1, p["out.ln.weight"], p["out.ln.bias"]) + F.linear(x, p["out.skp.weight"]))[:, 0]
