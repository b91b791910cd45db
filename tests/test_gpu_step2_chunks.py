"""GPU parity of the L = 2 step kernel (icnn2_step_kernel, csrc/icnn_step2.h) in workgroups that take MORE THAN ONE chunk.
At h = 130 the two weight images fill the LDS and the dW stage aliases the W2 image (Cfg2::ALIAS): behind each chunk's backward pass the
waves overwrite W2 with (dz2 | z1ext), then with (dz1 | z0ext), and a workgroup with another chunk to come fetches W2 again by LDS-DMA,
awaited at barrier (A) of that chunk behind its layer-1 product.  A stale or half-arrived W2 image, a piece that never comes back, a stage
write in front of barrier (B), the dWa / dWb / dL0 / accW accumulators carried across chunks, a ragged last chunk in a second or
third trip, the dcoords stores of the DX instantiations inside the loop: all of it runs only where a workgroup takes two or more
chunks, which no other test with a gradient bar does for L = 2.  So the launches are tiny and the slab base is set by hand
(inrfit_debug_set_slab_base), as tests/test_gpu_step_dw_first.py does for the L = 1 kernel:

    two_and_one    base 8, N = 64 * 10 + 17   workgroups 0-2 take two chunks (one re-fetch; chunk 10 has 17 points), 3-7 take one
    one_each       base 8, N = 64 * 3         three workgroups, one chunk each: no re-fetch (the control)
    three_each     base 2, N = 64 * 5 + 1     two workgroups, three chunks each (two re-fetches); the last chunk holds one point
    seven_on_one   base 1, N = 64 * 6 + 5     one workgroup, seven chunks (a.wgs == 1, six re-fetches)

Shapes (h, C): the four compiled ones (130 | 64) x (2 | 3) - at 64 the stage has LDS of its own and nothing is re-fetched, so both
branches run - and the zero-padded widths (100, 2) on the 130 kernel, (48, 2) on the 64 kernel.

Checker: the CPU oracle in float64 on inputs that are CONDITIONED (tests/step2_cases.py: no ReLU pre-activation within 4 x the float32
forward error bound of zero, so no correct float32 evaluation can take a unit on the other side of its kink; the CPU side of it,
float32 torch meeting every bar below, is tests/test_step2_cases_host.py), and bit-equality of runs of the same build with and
without NaN-filled workspaces and outputs.

Bars: assertions this suite already makes on this kernel at one chunk per workgroup - loss rel 1e-5; every parameter gradient tensor
rtol 2e-4, atol 2e-6 max|ref| + 1e-9 (test_every_column_reaches_its_parameter); dcoords rtol 2e-4, atol 2e-6 max|ref|
(test_coordinate_gradient); logits atol 5e-6, rtol 1e-5 (test_any_hidden_width...); 10-step loss curve rel 2e-5, parameters after 10 Adam
steps rtol 2e-4, atol 5e-6 (the L = 1 file); encode nets loss rel 1e-4, gradients 3e-3 (|ref| + max|ref|) (test_gpu_encode); composites:
those of test_hip_flow_forward_and_cdn_gradients and of test_gpu_rnvp.py::test_forward_and_gradients.

Every test prints e_hip / e_torch32 - the max-norm error relative to max|ref| of HIP and of float32 CPU torch, both against float64 -
before it asserts (recorded in profiles/NOTES.md, not asserted)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import inr_oracle as O  # noqa: E402,F401  (checker only)
from tests import step2_cases as S  # noqa: E402

NAMES = list(S.LAUNCHES)
MULTI = ["two_and_one", "three_each", "seven_on_one"]


@pytest.fixture(scope="module")
def amd():
    import awesome_amd as A
    A._lib.load()
    assert torch.cuda.is_available()
    return A


@contextlib.contextmanager
def launch(A, name, n_images=1):
    """the slab base of the launch `name`; the library's own (0) again afterwards"""
    base, n, wgs = S.TWO_IMAGES if name == "two_images" else S.LAUNCHES[name]
    lib = A._lib.load()
    assert lib.inrfit_debug_set_slab_base(base) == 0
    try:
        assert lib.inrfit_slabs_per_image(n, n_images) == wgs
        yield
    finally:
        lib.inrfit_debug_set_slab_base(0)


def _dev_inputs(A, c):
    dev = torch.device("cuda:0")
    assert c["spec"].supported() and c["spec"].fused()
    return dev, A.pack_state_dict(c["spec"], c["p"], dev)[None].contiguous(), A.Grid.explicit(c["coords"].to(dev))


def _three_runs(A, fn):
    """fn() twice on NaN-filled workspaces and outputs and once on plain ones: the same bits, nothing non-finite"""
    runs = []
    try:
        for poison in (True, True, False):
            A._lib.POISON = poison
            runs.append(fn())
    finally:
        A._lib.POISON = False
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    for a in runs[0]:
        assert torch.isfinite(a).all()
    return runs[0]


def _ratio(tag, got, ref, t32):
    """prints e_hip / e_torch32 over the tensors of `ref`"""
    e_hip, e_t32 = S.worst_max_norm(got, ref), S.worst_max_norm(t32, ref)
    print(f"[e_hip/e_torch32] {tag}: e_hip {e_hip:.2e} e_torch32 {e_t32:.2e} ratio {e_hip / max(e_t32, 1e-300):.2f}")


def _grads(A, spec, flat):
    return {k: v.double().numpy() for k, v in A.unpack_params(spec, flat.cpu()).items()}


# ---- a. loss and every gradient ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("h,C", S.SHAPES)
def test_loss_and_every_gradient(amd, h, C, name):
    A = amd
    c = S.case(h, C, name)
    S.assert_conditioned(c)
    dev, flat, grid = _dev_inputs(A, c)
    lo, go = S.ref(c, S.loss_and_grads, "se", "none")
    with launch(A, name):
        loss, g = _three_runs(A, lambda: A.loss_grad(c["spec"], flat, grid, c["un"][None].to(dev), loss="se"))
    tag = f"se h {h} C {C} {name}"
    print(f"{tag}: loss rel err {abs(float(loss[0]) - lo) / abs(lo):.2e}")
    got = _grads(A, c["spec"], g[0])
    _ratio(tag, got, go, S.ref(c, S.loss_and_grads, "se", "none", torch.float32)[1])
    S.assert_tensors(got, go, S.GRAD_BAR, tag)   # (prints every figure before the first assertion)
    assert float(loss[0]) == pytest.approx(lo, rel=1e-5)


# ---- b. BCE with the sssdms weights -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("h,C", [(130, 2), (64, 3)])
def test_bce_with_sssdms_weights(amd, h, C, name):
    A = amd
    c = S.case(h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    lo, go = S.ref(c, S.loss_and_grads, "bce", "sssdms")
    with launch(A, name):
        loss, g = _three_runs(A, lambda: A.loss_grad(c["spec"], flat, grid, c["hard"][None].to(dev), loss="bce", weight_mode="sssdms"))
    tag = f"bce h {h} C {C} {name}"
    print(f"{tag}: loss rel err {abs(float(loss[0]) - lo) / abs(lo):.2e}")
    got = _grads(A, c["spec"], g[0])
    _ratio(tag, got, go, S.ref(c, S.loss_and_grads, "bce", "sssdms", torch.float32)[1])
    S.assert_tensors(got, go, S.GRAD_BAR, tag)
    assert float(loss[0]) == pytest.approx(lo, rel=1e-5)


# ---- c. external gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("h,C", [(130, 2), (64, 3)])
def test_external_gradient(amd, h, C, name):
    """the train kernel with dL/dlogits handed in (`backward`)"""
    A = amd
    c = S.case(h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    with launch(A, name):
        (g,) = _three_runs(A, lambda: (A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev)),))
    tag = f"vjp h {h} C {C} {name}"
    got = _grads(A, c["spec"], g[0])
    _ratio(tag, got, S.ref(c, S.vjp)[0], S.ref(c, S.vjp, torch.float32)[0])
    S.assert_tensors(got, S.ref(c, S.vjp)[0], S.GRAD_BAR, tag)


# ---- d. coordinate gradients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("h,C", S.COMPILED)
def test_coordinate_gradient_kernel(amd, h, C, name):
    """the DX instantiations (their own register allocation, and a second kind of global store inside the chunk loop)"""
    A = amd
    c = S.case(h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    gref, xref = S.ref(c, S.vjp)
    g32, x32 = S.ref(c, S.vjp, torch.float32)
    with launch(A, name):
        g, dco = _three_runs(A, lambda: A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev), want_dcoords=True))
    tag = f"dx h {h} C {C} {name}"
    got = _grads(A, c["spec"], g[0])
    got_x = {"dcoords": dco[0].cpu().double().numpy()}
    _ratio(tag, got, gref, g32)
    _ratio(tag + " dcoords", got_x, {"dcoords": xref}, {"dcoords": x32})
    for k, r in gref.items():
        print(f"   {tag} {k}: max |err| / max |ref| {S.max_norm_error(got[k], r):.2e}, of its bar {S.bar_use(got[k], r, **S.GRAD_BAR):.3f}")
    S.assert_tensors(got_x, {"dcoords": xref}, S.DCOORDS_BAR, tag)
    S.assert_tensors(got, gref, S.GRAD_BAR, tag)


# ---- e. the forward-only kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MULTI)
@pytest.mark.parametrize("h,C", [(130, 2), (64, 2), (100, 2)])
def test_forward_only_kernel(amd, h, C, name):
    A = amd
    c = S.case(h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    ref = S.ref(c, S.logits).numpy()
    with launch(A, name):
        (logits,) = _three_runs(A, lambda: (A.forward(c["spec"], flat, grid),))
    got = logits[0].cpu().double().numpy()
    print(f"[e_hip/e_torch32] forward h {h} C {C} {name}: logits max |err| {float(np.abs(got - ref).max()):.2e}, float32 torch "
          f"{float(np.abs(S.ref(c, S.logits, torch.float32).double().numpy() - ref).max()):.2e}")
    np.testing.assert_allclose(got, ref, atol=5e-6, rtol=1e-5)


# ---- f. two images in one launch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,C", [(130, 2), (64, 2)])
def test_two_images_in_one_launch(amd, h, C):
    """base 4, two images: img = blockIdx.x / a.wgs, two workgroups of three chunks per image, each image with its own parameters,
    coordinates and targets, judged against its own float64 reference"""
    A = amd
    dev = torch.device("cuda:0")
    cs = [S.case(h, C, "two_images", im) for im in (0, 1)]
    for c in cs:
        S.assert_conditioned(c)
    spec = cs[0]["spec"]
    flat = torch.stack([A.pack_state_dict(spec, c["p"], dev) for c in cs]).contiguous()
    grid = A.Grid.explicit(torch.stack([c["coords"] for c in cs]).to(dev))
    un = torch.stack([c["un"] for c in cs]).to(dev)
    with launch(A, "two_images", 2):
        loss, g = _three_runs(A, lambda: A.loss_grad(spec, flat, grid, un, loss="se"))
    out = []
    for im, c in enumerate(cs):
        lo, go = S.ref(c, S.loss_and_grads, "se", "none")
        tag = f"two images h {h} C {C} image {im}"
        print(f"{tag}: loss rel err {abs(float(loss[im]) - lo) / abs(lo):.2e}")
        got = _grads(A, spec, g[im])
        _ratio(tag, got, go, S.ref(c, S.loss_and_grads, "se", "none", torch.float32)[1])
        out.append((got, go, tag, float(loss[im]), lo))
    for got, go, tag, l, lo in out:
        S.assert_tensors(got, go, S.GRAD_BAR, tag)
        assert l == pytest.approx(lo, rel=1e-5)


# ---- g. encode nets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fourier", "sine"])
def test_encode_nets(amd, kind):
    """one cos (h = 130) and one sin (h = 64) layer 0 in front of two hidden layers, two chunks on three of eight workgroups, at the bars
    of test_gpu_encode; the skip weights are constants of this model family and left out"""
    A = amd
    dev = torch.device("cuda:0")
    c = S.encode_case(kind)
    S.assert_conditioned(c)
    assert c["spec"].supported() and c["spec"].fused()
    lo, go = S.ref(c, S.encode_loss_and_grads)
    flat, grid = c["flat"][None].to(dev).contiguous(), A.Grid.explicit(c["coords"].to(dev))
    with launch(A, "two_and_one"):
        loss, g = _three_runs(A, lambda: A.loss_grad(c["spec"], flat, grid, c["hard"][None].to(dev)))
    print(f"{kind}: loss rel err {abs(float(loss[0]) - lo) / lo:.2e}")
    got = {k: v for k, v in _grads(A, c["spec"], g[0]).items() if k in go}
    _ratio(f"encode {kind}", got, go, S.ref(c, S.encode_loss_and_grads, torch.float32)[1])
    S.assert_tensors(got, go, S.ENCODE_BAR, kind)
    assert float(loss[0]) == pytest.approx(lo, rel=1e-4)


# ---- h. trajectory ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,C,name", [(130, 2, "two_and_one"), (64, 2, "three_each")])
def test_adam_clamp_trajectory(amd, h, C, name):
    """25 Adam + clamp steps: one 25-step fit = 25 one-step fits, bit for bit (every step's slabs are complete when its update reads
    them, and the W2 image the next step's first chunk multiplies by is the updated one); 10 steps against the oracle's in float64."""
    A = amd
    c = S.case(h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    un = c["hard"][None].to(dev)
    pf, losses = S.ref(c, S.trajectory)
    p32, l32 = S.ref(c, S.trajectory, 10, torch.float32)
    with launch(A, name):
        whole = A.fit(c["spec"], flat.clone(), grid, un, 25, lr=2e-3, want_logits=False)
        ten = A.fit(c["spec"], flat.clone(), grid, un, 10, lr=2e-3, want_logits=False)
        params, opt, hist = flat.clone(), A.icnn.new_opt_state(c["spec"], 1, dev), []
        for k in range(25):
            one = A.fit(c["spec"], params, grid, un, 1, lr=2e-3, opt_state=opt, step0=k, want_logits=False)
            params, opt = one.params, one.opt_state
            hist.append(one.loss_hist[:, 0].clone())
    P = c["spec"].n_params
    got_l = ten.loss_hist[0].cpu().numpy().astype(np.float64)
    got = A.unpack_params(c["spec"], ten.params[0].cpu())
    print(f"h {h} {name}: loss curve max rel err {float(np.abs(got_l / np.asarray(losses) - 1).max()):.2e}, float32 torch "
          f"{float(np.abs(np.asarray(l32) / np.asarray(losses) - 1).max()):.2e}")
    for k, want in pf.items():
        print(f"   {k}: max |err| {float(np.abs(got[k].double().numpy() - want.numpy()).max()):.2e}, float32 torch "
              f"{float((p32[k].double() - want).abs().max()):.2e}")
    assert int(whole.status[0]) == 0 and int(ten.status[0]) == 0
    assert torch.equal(whole.params, params)
    assert torch.equal(whole.opt_state[:, :2 * P], opt[:, :2 * P])
    assert torch.equal(whole.loss_hist, torch.stack(hist, dim=1))
    np.testing.assert_allclose(got_l, np.asarray(losses), rtol=2e-5)
    for k, want in pf.items():
        np.testing.assert_allclose(got[k].numpy(), want.numpy(), rtol=2e-4, atol=5e-6, err_msg=k)
    for k in c["spec"].clamp_keys():
        assert float(got[k].min()) >= 0.0


# ---- i. composites ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cdn", "pcn"])
def test_composites(amd, kind):
    """ICNN(130, 2, 2) behind the coupling flow (cdn) and behind the RealNVP (pcn) at two_and_one: the DX kernel's coordinate gradient
    drives the deformation's.  The conditioning holds for the ICNN's inputs as the flow kernels give them: the deformed coordinates are
    asserted to lie within the bar that the conditioning allowed for them."""
    A = amd
    from awesome_amd import flow as FL
    from awesome_amd import rnvp as R
    dev = torch.device("cuda:0")
    c = S.composite_case(kind)
    S.assert_conditioned(c)
    ispec = A.IcnnSpec(130, 2, 2)
    lo, go, xd_ref, y_ref = S.ref(c, S.composite_loss_and_grads)
    _, g32, _, _ = S.ref(c, S.composite_loss_and_grads, torch.float32)
    grid, un = A.Grid.explicit(c["coords"].to(dev)), c["un"][None].to(dev)
    if kind == "cdn":
        fspec = FL.FlowSpec(S.CDN_WIDTH, S.CDN_K)
        ip, fp = FL.split_cdn_state_dict(ispec, fspec, c["sd"], dev)
        ip, fp = ip[None].contiguous(), fp[None].contiguous()
        bar, xbar, lrel = S.CDN_BAR, S.CDN_XD, 2e-5
        with launch(A, "two_and_one"):
            xd = FL.flow_forward(fspec, fp, grid)
            loss, gi, gf = _three_runs(A, lambda: FL.cdn_loss_grad(ispec, fspec, ip, fp, grid, un, loss="bce"))
        got = FL.merge_cdn_state_dict(ispec, fspec, gi[0].cpu(), gf[0].cpu())
    else:
        rspec = c["rspec"]
        ip = A.pack_state_dict(ispec, {k[len("convex_net."):]: v for k, v in c["sd"].items() if k.startswith("convex_net.")}, dev)[None].contiguous()
        fp = R.pack_rnvp_state_dict(rspec, c["sd"], dev)[None].contiguous()
        bar, xbar, lrel = S.PCN_BAR, S.PCN_XD, 3e-5
        with launch(A, "two_and_one"):
            xd = R.rnvp_forward(rspec, fp, grid)
            loss, gi, gf = _three_runs(A, lambda: R.pcn_loss_grad(ispec, rspec, ip, fp, grid, un, loss="se", weight_mode="sssdms"))
        got = {"convex_net." + k: v for k, v in A.unpack_params(ispec, gi[0].cpu()).items()}
        got.update(R.unpack_rnvp_params(rspec, gf[0].cpu()))
    got = {k: v.double().numpy() for k, v in got.items()}
    print(f"{kind}: loss rel err {abs(float(loss[0]) - lo) / abs(lo):.2e}; deformed coordinates max |err| "
          f"{float((xd[0].cpu().double() - xd_ref).abs().max()):.2e}")
    _ratio(f"composite {kind}", got, go, g32)
    np.testing.assert_allclose(xd[0].cpu().numpy(), xd_ref.numpy(), **xbar)
    S.assert_tensors(got, go, bar, kind)
    assert float(loss[0]) == pytest.approx(lo, rel=lrel)
