"""GPU parity of the L = 1 step kernel around the point where its dW tiles leave for the gradient slab (icnn_step.h).
Written for the order "dW product first, the tiles of a workgroup's LAST chunk leave from inside the chunk loop" (measured slower
and not shipped, profiles/NOTES.md); what ships moves the same stores the other way, in between the cross-lane sums behind the loop
(icnn_step_tiles.h).  Either way the same few things can go wrong: which chunk a workgroup takes for its last one, a tile stored
before its last chunk was added, stored twice or never, a slab column of the sums clobbered by a tile.  (The L = 2 kernel's counterpart, with its W2 re-fetch: tests/test_gpu_step2_chunks.py.)
So the launches here are tiny and the
slab base is set by hand (inrfit_debug_set_slab_base) to choose the chunks per workgroup:

    base 8, N = 64 * 10 + 17   11 chunks on 8 workgroups: 0-2 take two, 3-7 take one, the last chunk is ragged
    base 8, N = 64 * 3         the library launches one workgroup per chunk when there are fewer chunks than slabs: three workgroups
                               with one chunk each (no launch of the library has a workgroup without a chunk)
    base 2, N = 64 * 5 + 1     6 chunks on 2 workgroups: three each (0, 2, 4 and 1, 3, 5), the last chunk holds one point

Checker: the CPU oracle in float64 (its own error is far below every bar), and bit-equality of runs of the same build with and without a
NaN-filled workspace (a slab column that is never written, or written early and overwritten, would show there).
Bars: the suite's own - loss rel 1e-5, gradients rel 2e-4 + 2e-6 max|g| (test_loss_and_grads_match_reference); coordinate
gradients rel 2e-4 + 2e-6 max|g| (test_coordinate_gradient_kernels); encode nets loss rel 1e-4, gradients 3e-3 (test_gpu_encode);
logits 5e-6 (test_forward_matches_reference); parameters after 10 Adam steps rel 2e-4 + 5e-6 (test_adam_clamp_trajectory)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import inr_oracle as O  # noqa: E402  (checker only)

LAUNCHES = {"two_and_one": (8, 64 * 10 + 17, 8), "one_each": (8, 64 * 3, 3), "three_each": (2, 64 * 5 + 1, 2)}   # slab base, N, workgroups
SHAPES = [(130, 2), (64, 2), (32, 2), (130, 3)]


@pytest.fixture(scope="module")
def amd():
    import awesome_amd as A
    A._lib.load()
    assert torch.cuda.is_available()
    return A


@contextlib.contextmanager
def launch(A, name):
    """the slab base of LAUNCHES[name]; the library's own (0) again afterwards"""
    base, n, wgs = LAUNCHES[name]
    lib = A._lib.load()
    assert lib.inrfit_debug_set_slab_base(base) == 0
    try:
        assert lib.inrfit_slabs_per_image(n, 1) == wgs
        yield
    finally:
        lib.inrfit_debug_set_slab_base(0)


_CASES = {}


def _case(A, h, C, name):
    """One problem per (shape, launch), built once and left unchanged: parameters (non-zero everywhere), explicit coordinates,
    soft and hard targets."""
    key = (h, C, name)
    if key not in _CASES:
        n = LAUNCHES[name][1]
        g = torch.Generator().manual_seed(1000 * h + 10 * C + n)
        spec = A.IcnnSpec(n_hidden=h, in_features=C, n_layers=1)
        assert spec.supported()
        p = {k: (torch.rand(shp, generator=g) - 0.45) * 0.3 for k, shp in spec.keys_shapes()}
        coords = torch.rand(C, n, generator=g)
        un = torch.rand(n, generator=g)
        _CASES[key] = dict(spec=spec, p=p, coords=coords, un=un, hard=(un > 0.6).float(), dlog=torch.randn(n, generator=g), refs={})
    return _CASES[key]


def _f64(p):
    return {k: v.double() for k, v in p.items()}


def _image(c):
    """the oracle's (1, C, 1, N) view of the coordinates"""
    C, n = c["coords"].shape
    return c["coords"].double().reshape(1, C, 1, n)


def _ref_loss(c, kind, mode):
    """float64 loss and gradients, computed once per case"""
    if (kind, mode) not in c["refs"]:
        tgt = (c["hard"] if mode == "sssdms" else c["un"]).double().reshape(1, 1, 1, -1)
        c["refs"][(kind, mode)] = O.loss_and_grads(_f64(c["p"]), _image(c), tgt, kind, mode)
    return c["refs"][(kind, mode)]


def _ref_vjp(c):
    """float64 d (dlog . logits) / d parameters and / d coordinates, computed once per case"""
    if "vjp" not in c["refs"]:
        pr = {k: v.double().requires_grad_(True) for k, v in c["p"].items()}
        xr = c["coords"].double().t().clone().requires_grad_(True)
        (O.icnn_forward(pr, xr)[:, 0] * c["dlog"].double()).sum().backward()
        c["refs"]["vjp"] = ({k: v.grad for k, v in pr.items()}, xr.grad.t())
    return c["refs"]["vjp"]


def _dev_inputs(A, c):
    dev = torch.device("cuda:0")
    return dev, A.pack_state_dict(c["spec"], c["p"], dev)[None].contiguous(), A.Grid.explicit(c["coords"].to(dev))


def _assert_grads(A, spec, got_flat, ref, tag, rtol=2e-4, arel=2e-6):
    got = A.unpack_params(spec, got_flat.cpu())
    assert set(got) == set(ref)
    for k, r in ref.items():
        r = r.numpy()
        print(f"   {tag} {k}: max |err| / max |ref| {float(np.abs(got[k].double().numpy() - r).max()) / (float(np.abs(r).max()) + 1e-30):.2e}")
    for k, r in ref.items():
        r = r.numpy()
        np.testing.assert_allclose(got[k].numpy(), r, rtol=rtol, atol=arel * float(np.abs(r).max()) + 1e-9, err_msg=f"{tag} {k}")


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


# ---- 1., 2. chunks per workgroup x shapes: loss and every gradient ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAUNCHES))
@pytest.mark.parametrize("h,C", SHAPES)
def test_loss_and_every_gradient(amd, h, C, name):
    A = amd
    c = _case(A, h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    lo, go = _ref_loss(c, "se", "none")
    with launch(A, name):
        loss, g = _three_runs(A, lambda: A.loss_grad(c["spec"], flat, grid, c["un"][None].to(dev), loss="se"))
    print(f"h {h} C {C} {name}: loss rel err {abs(float(loss[0]) - lo) / abs(lo):.2e}")
    _assert_grads(A, c["spec"], g[0], go, f"h {h} C {C} {name}")   # (prints every figure before the first assertion)
    assert float(loss[0]) == pytest.approx(lo, rel=1e-5)


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_bce_with_sssdms_weights(amd, name):
    A = amd
    c = _case(A, 130, 2, name)
    dev, flat, grid = _dev_inputs(A, c)
    lo, go = _ref_loss(c, "bce", "sssdms")
    with launch(A, name):
        loss, g = _three_runs(A, lambda: A.loss_grad(c["spec"], flat, grid, c["hard"][None].to(dev), loss="bce", weight_mode="sssdms"))
    print(f"{name}: loss rel err {abs(float(loss[0]) - lo) / abs(lo):.2e}")
    _assert_grads(A, c["spec"], g[0], go, name)
    assert float(loss[0]) == pytest.approx(lo, rel=1e-5)


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_external_gradient(amd, name):
    """the train kernel with dL/dlogits handed in (`backward`)"""
    A = amd
    c = _case(A, 130, 2, name)
    dev, flat, grid = _dev_inputs(A, c)
    with launch(A, name):
        (g,) = _three_runs(A, lambda: (A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev)),))
    _assert_grads(A, c["spec"], g[0], _ref_vjp(c)[0], name)


@pytest.mark.parametrize("name", list(LAUNCHES))
@pytest.mark.parametrize("h,C", SHAPES)
def test_coordinate_gradient_kernel(amd, h, C, name):
    """the DX instantiations (their own register allocation, and a second kind of global store inside the chunk loop)"""
    A = amd
    c = _case(A, h, C, name)
    dev, flat, grid = _dev_inputs(A, c)
    gref, xref = _ref_vjp(c)
    with launch(A, name):
        g, dco = _three_runs(A, lambda: A.icnn.backward(c["spec"], flat, grid, c["dlog"][None].to(dev), want_dcoords=True))
    xref = xref.numpy()
    print(f"h {h} C {C} {name}: dcoords max |err| / max |ref| {float(np.abs(dco[0].cpu().double().numpy() - xref).max()) / float(np.abs(xref).max()):.2e}")
    _assert_grads(A, c["spec"], g[0], gref, f"h {h} C {C} {name}")
    np.testing.assert_allclose(dco[0].cpu().numpy(), xref, rtol=2e-4, atol=2e-6 * float(np.abs(xref).max()))


@pytest.mark.parametrize("kind", ["fourier", "sine"])
def test_encode_nets(amd, kind):
    """one cos and one sin layer 0 (their own instantiations), two chunks on three of eight workgroups, at the bars of test_gpu_encode"""
    A = amd
    from awesome_amd.model import FourierFeatureNet, SineLayerNet
    dev = torch.device("cuda:0")
    torch.manual_seed(62)
    m = FourierFeatureNet(d_in=2, n_hidden=130, n_hidden_layers=1, factor=30.0) if kind == "fourier" else \
        SineLayerNet(in_features=2, n_hidden=130, n_hidden_layers=1)
    c = _case(A, 130, 2, "two_and_one")
    coords = c["coords"] - (0.5 if kind == "sine" else 0.0)      # the sine notebook centres its coordinates
    p = {k: v.double().requires_grad_(True) for k, v in A.unpack_params(m.spec, m.flat_parameters().cpu()).items()}
    n = coords.shape[1]
    yo = O.icnn_forward_image(p, coords.double().reshape(1, 2, 1, n), m.spec.act0, m.spec.omega)
    lo = O.weighted_loss(torch.sigmoid(yo), c["hard"].double().reshape(1, 1, 1, n), "se")
    lo.backward()
    flat, grid = m.flat_parameters()[None].to(dev).contiguous(), A.Grid.explicit(coords.to(dev))
    with launch(A, "two_and_one"):
        loss, g = _three_runs(A, lambda: A.loss_grad(m.spec, flat, grid, c["hard"][None].to(dev)))
    print(f"{kind}: loss rel err {abs(float(loss[0]) - float(lo)) / float(lo):.2e}")
    ref = {k: v.grad for k, v in p.items() if not k.endswith("skp.weight")}   # the skip weights are constants of this model family
    got = {k: v for k, v in A.unpack_params(m.spec, g[0].cpu()).items() if k in ref}
    for k, r in ref.items():
        r = r.numpy()
        print(f"   {kind} {k}: max |err| / max |ref| {float(np.abs(got[k].double().numpy() - r).max()) / (float(np.abs(r).max()) + 1e-30):.2e}")
    assert float(loss[0]) == pytest.approx(float(lo), rel=1e-4)
    for k, r in ref.items():
        r = r.numpy()
        np.testing.assert_allclose(got[k].numpy(), r, rtol=3e-3, atol=3e-3 * float(np.abs(r).max()) + 1e-9, err_msg=k)


# ---- 3. trajectory ----------------------------------------------------------------------------------------------------------------
def test_adam_clamp_trajectory(amd):
    """25 Adam + clamp steps where three workgroups take two chunks: one 25-step fit = 25 one-step fits, bit for bit (every step's
    slabs are complete when its update reads them, whichever launch follows); 10 steps against the oracle's."""
    A = amd
    c = _case(A, 130, 2, "two_and_one")
    dev, flat, grid = _dev_inputs(A, c)
    un = c["hard"][None].to(dev)
    pf, losses, _ = O.fit_icnn(_f64(c["p"]), _image(c), c["hard"].double().reshape(1, 1, 1, -1), 10, lr=2e-3)
    with launch(A, "two_and_one"):
        whole = A.fit(c["spec"], flat.clone(), grid, un, 25, lr=2e-3, want_logits=False)
        ten = A.fit(c["spec"], flat.clone(), grid, un, 10, lr=2e-3, want_logits=False)
        params, opt, hist = flat.clone(), A.icnn.new_opt_state(c["spec"], 1, dev), []
        for k in range(25):
            one = A.fit(c["spec"], params, grid, un, 1, lr=2e-3, opt_state=opt, step0=k, want_logits=False)
            params, opt = one.params, one.opt_state
            hist.append(one.loss_hist[:, 0].clone())
    P = c["spec"].n_params
    assert int(whole.status[0]) == 0 and int(ten.status[0]) == 0
    assert torch.equal(whole.params, params)
    assert torch.equal(whole.opt_state[:, :2 * P], opt[:, :2 * P])
    assert torch.equal(whole.loss_hist, torch.stack(hist, dim=1))
    got_l = ten.loss_hist[0].cpu().numpy().astype(np.float64)
    print(f"loss curve max rel err {float(np.abs(got_l / np.asarray(losses) - 1).max()):.2e}")
    got = A.unpack_params(c["spec"], ten.params[0].cpu())
    for k, want in pf.items():
        print(f"   {k}: max |err| {float(np.abs(got[k].double().numpy() - want.numpy()).max()):.2e}")
    np.testing.assert_allclose(got_l, np.asarray(losses), rtol=2e-5)
    for k, want in pf.items():
        np.testing.assert_allclose(got[k].numpy(), want.numpy(), rtol=2e-4, atol=5e-6, err_msg=k)
    for k in c["spec"].clamp_keys():
        assert float(got[k].min()) >= 0.0


# ---- 4. the forward-only kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_and_one", "three_each"])
def test_forward_only_kernel_on_a_ragged_launch(amd, name):
    A = amd
    c = _case(A, 130, 2, name)
    dev, flat, grid = _dev_inputs(A, c)
    with torch.no_grad():
        ref = O.icnn_forward_image(_f64(c["p"]), _image(c)).reshape(-1).numpy()
    with launch(A, name):
        (logits,) = _three_runs(A, lambda: (A.forward(c["spec"], flat, grid),))
    print(f"{name}: logits max |err| {float(np.abs(logits[0].cpu().double().numpy() - ref).max()):.2e}")
    np.testing.assert_allclose(logits[0].cpu().numpy(), ref, rtol=0, atol=5e-6)
