"""GPU parity of the L = 1 step kernel where its layer-0 mask is read back from the staged z0 and its layer-0 gradient runs as slices
between the k-steps of the dW product (icnn_step.h, icnn_step_l0.h).  What can go wrong there: a mask value taken from
another point's row or another unit's column of the stage; a slice that reads coordinates the next chunk has already overwritten (one
that is not complete in front of the chunk-end barrier); a tile quad's padding, or the leftover units, mixed into the transpose; a
point of a ragged chunk counted.  The method is that of tests/test_gpu_step_dw_first.py: tiny launches, the slab base set by hand
(inrfit_debug_set_slab_base) to choose the chunks per workgroup, the float64 CPU oracle as checker, and every launch a second time on
a NaN-filled workspace with equal bits.  Cases, launches and shapes: tests/step_l0_cases.py; that float32 torch meets every bar on
them: tests/test_step_l0_cases_host.py.  A slice behind the barrier would fail the multi-chunk launches and pass `one_each`.

Bars: the suite's own, as in test_gpu_step_dw_first.py - loss rel 1e-5, gradients rel 2e-4 + 2e-6 max|g|, coordinate gradients
rel 2e-4 + 2e-6 max|g|, the encode net loss rel 1e-4, gradients 3e-3."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import step2_cases as S  # noqa: E402  (references, bars, figures)
from tests import step_l0_cases as Z  # noqa: E402


@pytest.fixture(scope="module")
def amd():
    import awesome_amd as A
    A._lib.load()
    assert torch.cuda.is_available()
    return A


@contextlib.contextmanager
def launch(A, name, n_images=1):
    """the slab base of the launch `name`; the library's own (0) again afterwards"""
    base, n, wgs = Z.TWO_IMAGES if name == "two_images" else Z.LAUNCHES[name]
    lib = A._lib.load()
    assert lib.inrfit_debug_set_slab_base(base) == 0
    try:
        assert lib.inrfit_slabs_per_image(n, n_images) == wgs
        yield
    finally:
        lib.inrfit_debug_set_slab_base(0)


def _dev_inputs(A, c):
    dev = torch.device("cuda:0")
    assert c["spec"].supported()
    assert c["spec"].fused() == (c["spec"].n_hidden <= 130)
    return dev, A.pack_state_dict(c["spec"], c["p"], dev)[None].contiguous(), A.Grid.explicit(c["coords"].to(dev))


def _two_runs(A, fn):
    """fn() on plain workspaces and outputs, then on NaN-filled ones: the same bits, nothing non-finite"""
    runs = []
    try:
        for poison in (False, True):
            A._lib.POISON = poison
            runs.append(fn())
    finally:
        A._lib.POISON = False
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    for a in runs[0]:
        assert torch.isfinite(a).all()
    return runs[0]


@pytest.mark.parametrize("name", list(Z.LAUNCHES))
@pytest.mark.parametrize("h,C", Z.SHAPES)
def test_loss_and_every_gradient(amd, h, C, name):
    A = amd
    c = Z.case(h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    lo, go = S.ref(c, S.loss_and_grads, "se", "none")
    with launch(A, name):
        loss, g = _two_runs(A, lambda: A.loss_grad(c["spec"], flat, grid, c["un"][None].to(dev), loss="se"))
    print(f"h {h} C {C} {name}: loss rel err {abs(float(loss[0]) - lo) / abs(lo):.2e}")
    S.assert_tensors(A.unpack_params(c["spec"], g[0].cpu()), go, S.GRAD_BAR, f"h {h} C {C} {name}")   # (prints every figure first)
    assert float(loss[0]) == pytest.approx(lo, rel=1e-5)


def test_two_images_in_one_launch(amd):
    """base 4, two images: two workgroups of three chunks per image, each image with its own parameters, coordinates and targets,
    judged against its own float64 reference (BCE with the sssdms weights)"""
    A = amd
    dev = torch.device("cuda:0")
    cs = [Z.case(130, 2, "two_images", im) for im in (0, 1)]
    spec = cs[0]["spec"]
    flat = torch.stack([A.pack_state_dict(spec, c["p"], dev) for c in cs]).contiguous()
    grid = A.Grid.explicit(torch.stack([c["coords"] for c in cs]).to(dev))
    hard = torch.stack([c["hard"] for c in cs]).to(dev)
    with launch(A, "two_images", 2):
        loss, g = _two_runs(A, lambda: A.loss_grad(spec, flat, grid, hard, loss="bce", weight_mode="sssdms"))
    for im, c in enumerate(cs):
        lo, go = S.ref(c, S.loss_and_grads, "bce", "sssdms")
        print(f"image {im}: loss rel err {abs(float(loss[im]) - lo) / abs(lo):.2e}")
        S.assert_tensors(A.unpack_params(spec, g[im].cpu()), go, S.GRAD_BAR, f"two images, image {im}")
        assert float(loss[im]) == pytest.approx(lo, rel=1e-5)


@pytest.mark.parametrize("h,C,name", [(130, 2, "three_each"), (64, 2, "two_and_one"), (100, 2, "one_each")])
def test_coordinate_gradient_kernel(amd, h, C, name):
    """the DX instantiations: the masked dz0 feeds dcoords in front of the barrier and the layer-0 slices behind it"""
    A = amd
    c = Z.case(h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    gref, xref = S.ref(c, S.vjp)
    with launch(A, name):
        g, dco = _two_runs(A, lambda: A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev), want_dcoords=True))
    S.assert_tensors(A.unpack_params(c["spec"], g[0].cpu()), gref, S.GRAD_BAR, f"h {h} C {C} {name}")
    S.assert_tensors({"dcoords": dco[0].cpu()}, {"dcoords": xref}, S.DCOORDS_BAR, f"h {h} C {C} {name}")


def test_sine_encode_net(amd):
    """a sin layer 0 (its own instantiation: the pre-activation is still recomputed on the matrix pipe, the slices are shared), two
    chunks on three of eight workgroups, at the bars of test_gpu_encode"""
    A = amd
    dev = torch.device("cuda:0")
    c = Z.sine_case()
    lo, go = S.ref(c, S.encode_loss_and_grads)
    flat, grid = c["flat"][None].to(dev).contiguous(), A.Grid.explicit(c["coords"].to(dev))
    with launch(A, "two_and_one"):
        loss, g = _two_runs(A, lambda: A.loss_grad(c["spec"], flat, grid, c["hard"][None].to(dev)))
    print(f"sine: loss rel err {abs(float(loss[0]) - lo) / lo:.2e}")
    got = {k: v for k, v in A.unpack_params(c["spec"], g[0].cpu()).items() if k in go}
    S.assert_tensors(got, go, S.ENCODE_BAR, "sine")
    assert float(loss[0]) == pytest.approx(lo, rel=1e-4)
