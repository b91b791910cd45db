"""The launch edges of the step and update kernels.

Step kernel: the parameter image reaches LDS by LDS-DMA in 1 KB pieces plus a register-copied tail (no compiled image is a multiple
of 1 KB), and the first chunk's point is loaded before the image has arrived - also by the workgroups that have no chunk, which
load a clamped address and must still deliver zero slabs.  Update kernel: the slab loads are a block's first memory instructions and
also cover the padding columns of a slab row, which must never reach a result.

Checker: the CPU oracle, or bit-equality of two runs of the same build."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import inr_oracle as O  # noqa: E402  (checker only)

COMPILED_L1 = [(130, 2), (130, 3), (64, 2), (64, 3), (32, 2), (32, 3)]   # every (n_hidden, in_features) with an L = 1 step kernel
PADDED = [(100, 2), (129, 2)]                                           # run zero-padded on the 130 kernel


@pytest.fixture(scope="module")
def amd():
    import awesome_amd as A
    A._lib.load()
    assert torch.cuda.is_available()
    return A


def _params(spec, seed):
    """non-zero everywhere: a lost or misplaced piece of the image changes some result"""
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(shp, generator=g) - 0.45) * 0.3 for k, shp in spec.keys_shapes()}


def _assert_grads(A, spec, got_flat, ref, tag):
    """the bars of test_loss_and_every_parameter_gradient"""
    got = A.unpack_params(spec, got_flat.cpu())
    assert set(got) == set(ref)
    for k, r in ref.items():
        r = r.numpy()
        print(f"   {tag} {k}: max |err| / max |ref| {float(np.abs(got[k].numpy() - r).max()) / (float(np.abs(r).max()) + 1e-30):.2e}")
    for k, r in ref.items():
        r = r.numpy()
        np.testing.assert_allclose(got[k].numpy(), r, rtol=2e-4, atol=2e-4 * float(np.abs(r).max()) + 1e-10, err_msg=f"{tag} {k}")


# ---- 1. the image copy ----------------------------------------------------------------------------------------------------------
_IMAGE_CASES = {}


def _image_case(A, h, C):
    if (h, C) not in _IMAGE_CASES:
        H_, W_ = 19, 23
        spec = A.IcnnSpec(n_hidden=h, in_features=C, n_layers=1)
        assert spec.supported()
        p = _params(spec, 1000 * h + C)
        grid_t = O.positional_grid(W_, H_) if C == 2 else O.positional_grid(W_, H_, 0.4, 1.0)
        un = torch.from_numpy(np.random.RandomState(h + C).rand(1, 1, H_, W_).astype(np.float32))
        with torch.no_grad():
            logits = O.icnn_forward_image(p, grid_t[None]).reshape(-1)
        lo, go = O.loss_and_grads(p, grid_t[None], un, "se")
        _IMAGE_CASES[(h, C)] = dict(spec=spec, p=p, grid_t=grid_t, un=un, logits=logits, loss=float(lo), grads=go)
    return _IMAGE_CASES[(h, C)]


@pytest.mark.parametrize("h,C", COMPILED_L1 + PADDED)
def test_image_copy_every_l1_shape(amd, h, C):
    A, dev = amd, torch.device("cuda:0")
    c = _image_case(A, h, C)
    flat = A.pack_state_dict(c["spec"], c["p"], dev)[None].contiguous()
    grid = A.Grid.from_image_grid(c["grid_t"].to(dev))
    logits = A.forward(c["spec"], flat, grid)
    loss, g = A.loss_grad(c["spec"], flat, grid, c["un"].reshape(1, -1).to(dev), loss="se")
    ref = c["logits"].numpy()
    print(f"h {h} C {C}: logits max |err| {float(np.abs(logits[0].cpu().numpy() - ref).max()):.2e}, "
          f"loss rel err {abs(float(loss[0]) - c['loss']) / abs(c['loss']):.2e}")
    np.testing.assert_allclose(logits[0].cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    assert float(loss[0]) == pytest.approx(c["loss"], rel=2e-5)
    _assert_grads(A, c["spec"], g[0], c["grads"], f"h {h} C {C}")


# ---- 2. the early point loads ---------------------------------------------------------------------------------------------------
_POINT_CASES = {}


def _point_case(A, h, C, hw):
    """two images on a grid of one partial chunk: own parameters and targets, and for C = 3 an own t per image"""
    key = (h, C, hw)
    if key not in _POINT_CASES:
        H_, W_ = hw
        spec = A.IcnnSpec(n_hidden=h, in_features=C, n_layers=1)
        ts = [0.4, 0.9]
        ps, grids, uns, refs = [], [], [], []
        for i in range(2):
            p = _params(spec, 77 * h + 10 * C + H_ + i)
            gt = O.positional_grid(W_, H_) if C == 2 else O.positional_grid(W_, H_, ts[i], 1.0)
            un = torch.from_numpy(np.random.RandomState(h + C + H_ + i).rand(1, 1, H_, W_).astype(np.float32))
            refs.append(O.loss_and_grads(p, gt[None], un, "se"))
            ps.append(p), grids.append(gt), uns.append(un.reshape(-1))
        _POINT_CASES[key] = dict(spec=spec, ps=ps, grids=grids, uns=torch.stack(uns), refs=refs, ts=torch.tensor(ts))
    return _POINT_CASES[key]


@pytest.mark.parametrize("mode", ["separable", "explicit"])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7)])
@pytest.mark.parametrize("h,C", [(130, 2), (32, 3)])
def test_first_point_of_a_partial_chunk_and_of_no_chunk(amd, h, C, hw, mode):
    """1 x 1 and 5 x 7: one partial chunk per image; every other workgroup of the launch has no chunk and delivers a zero slab"""
    A, dev = amd, torch.device("cuda:0")
    c = _point_case(A, h, C, hw)
    H_, W_ = hw
    spec = c["spec"]
    flat = torch.stack([A.pack_state_dict(spec, p, dev) for p in c["ps"]]).contiguous()
    if mode == "separable":
        grid = A.Grid.separable(torch.linspace(0, 1, W_).to(dev), torch.linspace(0, 1, H_).to(dev), c["ts"].to(dev) if C == 3 else None)
    else:
        grid = A.Grid.from_image_grid(torch.stack(c["grids"]).to(dev))
    assert grid.n_points == H_ * W_ < 64
    loss, g = A.loss_grad(spec, flat, grid, c["uns"].to(dev), loss="se")
    for i in range(2):
        lo, go = c["refs"][i]
        print(f"h {h} C {C} grid {hw} {mode} image {i}: loss rel err {abs(float(loss[i]) - lo) / abs(lo):.2e}")
        assert float(loss[i]) == pytest.approx(lo, rel=2e-5)
        _assert_grads(A, spec, g[i], go, f"image {i}")


def test_joint_prior_step_with_fewer_targets_than_points(amd):
    """data_count < N: the early load's target index is clamped to the last target, and the points behind carry no data term.  The
    data term against the closed form on the oracle's logits; the gradient, read out of Adam's first moment after step 1
    (m = (1 - beta1) g from zero state), against the oracle's autograd."""
    from awesome_amd import joint as J
    A, dev = amd, torch.device("cuda:0")
    H_, W_, nd, cd = 5, 7, 20, 0.35
    spec = A.IcnnSpec(n_hidden=130, in_features=2, n_layers=1)
    p = _params(spec, 5)
    gt = O.positional_grid(W_, H_)
    n = H_ * W_
    gen = torch.Generator().manual_seed(9)
    tgt = torch.rand(nd, generator=gen)
    seg = torch.rand(n, generator=gen) * 0.9 + 0.05
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    prob = torch.sigmoid(O.icnn_forward_image(pr, gt[None]).reshape(-1))
    data = cd * torch.mean((tgt - prob[:nd]) ** 2)
    data.backward()
    data = data.detach()
    row = A.pack_state_dict(spec, p, dev).clone()
    opt = torch.zeros(2 * spec.n_params + 8, device=dev)
    res = J.joint_prior_step(spec, row, opt, A.Grid.linspace(W_, H_, dev), seg.to(dev), tgt.to(dev),
                             J.joint_prior_desc("se", data_count=nd, c_data=cd), step=1, lr=1e-3)
    assert int(res.status[0]) == 0 and float(res.loss[3]) == 1.0
    print(f"data term rel err {abs(float(res.loss[1]) - float(data)) / float(data):.2e}")
    assert float(res.loss[1]) == pytest.approx(float(data), rel=2e-5)
    assert float(res.loss[0]) == pytest.approx(float(data), rel=2e-5)
    g = opt[:spec.n_params] / np.float32(1.0 - 0.9)
    _assert_grads(A, spec, g, {k: v.grad.detach() for k, v in pr.items()}, "joint prior step")


# ---- 3. the update kernel's early slab loads ------------------------------------------------------------------------------------
_FIT_CASES = {}


def _fit_case(A, h, C, hw):
    """one problem and the oracle's (float64) 3 Adam steps with the convexity clamp, computed once"""
    key = (h, C, hw)
    if key not in _FIT_CASES:
        H_, W_ = hw
        spec = A.IcnnSpec(n_hidden=h, in_features=C, n_layers=1)
        assert spec.supported()
        p = _params(spec, 3 * h + C + W_)
        gt = O.positional_grid(W_, H_) if C == 2 else O.positional_grid(W_, H_, 0.4, 1.0)
        un = torch.from_numpy(np.random.RandomState(h + W_).rand(1, 1, H_, W_).astype(np.float32))
        pd = {k: v.double() for k, v in p.items()}
        pf, losses, _ = O.fit_icnn(pd, gt[None].double(), un.double(), 3, lr=2e-3)
        lo, go = O.loss_and_grads(pd, gt[None].double(), un.double(), "se")
        _FIT_CASES[key] = dict(spec=spec, p=p, gt=gt, un=un, pf=pf, losses=losses, loss=lo, grads=go)
    return _FIT_CASES[key]


# (131 x 127: 520 lines -> wide and narrow blocks, 260 chunks on 256 slabs;  (32, 3) on 19 x 23: fewer lines than CUs;  h = 256: the
# one-slab identity view of the layer-by-layer path)
@pytest.mark.parametrize("h,C,hw", [(130, 2, (131, 127)), (32, 3, (19, 23)), (256, 2, (19, 23))])
def test_three_adam_steps_poisoned_and_not(amd, h, C, hw):
    A, dev = amd, torch.device("cuda:0")
    c = _fit_case(A, h, C, hw)
    spec = c["spec"]
    flat = A.pack_state_dict(spec, c["p"], dev)[None].contiguous()
    grid = A.Grid.from_image_grid(c["gt"].to(dev))
    un = c["un"].reshape(1, -1).to(dev)
    runs = []
    try:
        for poison in (True, False):
            A._lib.POISON = poison
            runs.append(A.fit(spec, flat.clone(), grid, un, 3, lr=2e-3, clamp=True, record_loss=True, want_logits=False))
    finally:
        A._lib.POISON = False
    a, b = runs
    P = spec.n_params
    assert int(a.status.sum()) == 0 and int(b.status.sum()) == 0
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.opt_state[:, :P], b.opt_state[:, :P]) and torch.equal(a.opt_state[:, P:2 * P], b.opt_state[:, P:2 * P])
    assert torch.equal(a.loss_hist, b.loss_hist)
    assert torch.isfinite(a.params).all() and torch.isfinite(a.opt_state[:, :2 * P]).all() and torch.isfinite(a.loss_hist).all()
    # the oracle's 3 steps, at the bars of tests/test_gpu_update_layout.py
    got_l, want_l = a.loss_hist[0].cpu().numpy().astype(np.float64), np.asarray(c["losses"])
    print(f"h {h} C {C} grid {hw}: loss curve max rel err {float(np.abs(got_l / want_l - 1).max()):.2e}")
    np.testing.assert_allclose(got_l, want_l, rtol=2e-5)
    got = A.unpack_params(spec, a.params[0].cpu())
    for k, want in c["pf"].items():
        print(f"   {k}: max |err| {float(np.abs(got[k].double().numpy() - want.numpy()).max()):.2e}")
    for k, want in c["pf"].items():
        np.testing.assert_allclose(got[k].numpy(), want.numpy(), rtol=1e-4, atol=2e-5, err_msg=k)


def test_reduce_mode_poisoned_and_not(amd):
    A, dev = amd, torch.device("cuda:0")
    c = _fit_case(A, 130, 2, (131, 127))
    spec = c["spec"]
    flat = A.pack_state_dict(spec, c["p"], dev)[None].contiguous()
    grid = A.Grid.from_image_grid(c["gt"].to(dev))
    un = c["un"].reshape(1, -1).to(dev)
    runs = []
    try:
        for poison in (True, False):
            A._lib.POISON = poison
            runs.append(A.loss_grad(spec, flat, grid, un, loss="se"))
    finally:
        A._lib.POISON = False
    (la, ga), (lb, gb) = runs
    assert torch.equal(la, lb) and torch.equal(ga, gb) and torch.isfinite(ga).all()
    assert float(la[0]) == pytest.approx(c["loss"], rel=2e-5)
    got = A.unpack_params(spec, ga[0].cpu())
    for k, r in c["grads"].items():
        r = r.numpy()
        scale = max(1e-8, float(np.abs(r).max()))
        print(f"   {k}: max |err| {float(np.abs(got[k].double().numpy() - r).max()):.3e} (scale {scale:.3e})")
        np.testing.assert_allclose(got[k].numpy(), r, rtol=2e-4, atol=2e-6 * scale + 1e-9, err_msg=k)


# ---- 4. a frozen image ----------------------------------------------------------------------------------------------------------
def test_nan_target_at_step_2_of_4_freezes_the_image(amd):
    """Steps 2 to 4 see a NaN target: parameters and both moments stay what step 1 left, bit for bit."""
    A, dev = amd, torch.device("cuda:0")
    c = _fit_case(A, 32, 3, (19, 23))
    spec = c["spec"]
    P = spec.n_params
    flat = A.pack_state_dict(spec, c["p"], dev)[None].contiguous()
    grid = A.Grid.from_image_grid(c["gt"].to(dev))
    un = c["un"].reshape(1, -1).to(dev)
    bad = un.clone()
    bad[0, 200] = float("nan")
    one = A.fit(spec, flat.clone(), grid, un, 1, lr=2e-3, want_logits=False)
    assert int(one.status[0]) == 0 and not torch.equal(one.params, flat)
    p1, s1 = one.params.clone(), one.opt_state.clone()
    rest = A.fit(spec, one.params, grid, bad, 3, lr=2e-3, opt_state=one.opt_state, step0=1, want_logits=False)
    assert int(rest.status[0]) == 1   # INR_STATUS_NONFINITE (include/inrfit.h)
    assert torch.equal(rest.params, p1)
    assert torch.equal(rest.opt_state[:, :2 * P], s1[:, :2 * P])
