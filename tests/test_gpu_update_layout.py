"""The update kernel's two layout decisions: every block owns whole 128-byte lines of the slab columns, and the
"frozen by a non-finite loss" decision reads the step kernel's dense loss partials (one float per workgroup at the tail of the slab
buffer) instead of the slabs' loss column.  Neither changes a sum, so what is pinned here is that every column still reaches its
parameter at slab counts that take every path of the group sum - 2 slabs (fewer than the 16 groups), 17 (the tail loop) and 256 (the
unrolled trip) - for a width with leftover units (130), a zero-padded one (64), one and two hidden layers; and that a NaN seen by the
LAST workgroup alone freezes the image in every kernel that takes the decision."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import inr_oracle as O  # (checker only)

pytestmark = pytest.mark.gpu

GRIDS = {2: (10, 10), 17: (34, 32), 256: (128, 128)}   # slab count -> (W, H): 100 points = 2 chunks of 64, 64 * 17 points, 256 chunks


@pytest.fixture(scope="module")
def amd():
    import awesome_amd
    awesome_amd._lib.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return awesome_amd


@contextlib.contextmanager
def slab_base(amd, base):
    lib = amd._lib.load()
    assert lib.inrfit_debug_set_slab_base(base) == 0
    try:
        yield
    finally:
        lib.inrfit_debug_set_slab_base(0)


def _base_for(slabs, n_images):
    """slab base at which n_images images of GRIDS[slabs] get `slabs` slabs each (0 = the library's own 256)"""
    return slabs * n_images if slabs * n_images > 256 else 0


_PROBLEMS = {}


def _problem(amd, slabs, h, L):
    """two images (state dicts, packed parameters, targets) on GRIDS[slabs] and their float64 losses / gradients, computed once"""
    key = (slabs, h, L)
    if key not in _PROBLEMS:
        from awesome_amd.model import ConvexNextNet
        W, H = GRIDS[slabs]
        grid = O.positional_grid(W, H)
        spec = amd.IcnnSpec(h, 2, L)
        sds, uns, ref = [], [], []
        for i in range(2):
            torch.manual_seed(31 * slabs + 7 * h + L + i)
            m = ConvexNextNet(n_hidden=h, n_hidden_layers=L, in_features=2)
            sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
            un = torch.from_numpy(np.random.RandomState(slabs + h + L + i).rand(1, 1, H, W).astype(np.float32))
            ref.append(O.loss_and_grads({k: v.double() for k, v in sd.items()}, grid[None].double(), un.double(), "se"))
            sds.append(sd)
            uns.append(un.reshape(-1))
        params = torch.stack([amd.pack_state_dict(spec, sd, "cuda:0") for sd in sds]).contiguous()
        _PROBLEMS[key] = (spec, params, amd.Grid.from_image_grid(grid.to("cuda:0")), torch.stack(uns).to("cuda:0"), ref)
    return _PROBLEMS[key]


def _clamped(k):
    return k.endswith("ln.weight") and (k.startswith("skip") or k.startswith("out"))


@pytest.mark.parametrize("h,L", [(130, 1), (64, 1), (130, 2), (64, 2)])
@pytest.mark.parametrize("slabs", [2, 17, 256])
def test_every_column_reaches_its_parameter(amd, slabs, h, L):
    spec, params, grid, un, ref = _problem(amd, slabs, h, L)
    lib = amd._lib.load()
    with slab_base(amd, _base_for(slabs, 2)):
        assert lib.inrfit_slabs_per_image(grid.n_points, 2) == slabs
        loss, g = amd.loss_grad(spec, params, grid, un, loss="se")
        one = amd.fit(spec, params.clone(), grid, un, 1, lr=1e-2, loss="se", optimizer="adam", want_logits=False)
    assert int(one.status.sum()) == 0
    # the reduce mode's loss (the slab column) and the fit's (the same column, frozen decision from the dense partials): same bits
    assert torch.equal(loss.view(torch.int32), one.loss_hist[:, 0].contiguous().view(torch.int32))
    for i in range(2):
        lo, go = ref[i]
        assert float(loss[i]) == pytest.approx(float(lo), rel=2e-5)
        got = amd.unpack_params(spec, g[i].cpu())
        assert set(got) == set(go)
        for k, r in go.items():
            r = r.numpy()
            scale = max(1e-8, float(np.abs(r).max()))
            err = float(np.abs(got[k].double().numpy() - r).max())
            print(f"slabs {slabs} h {h} L {L} image {i} {k}: max |err| {err:.3e} (scale {scale:.3e})")
            np.testing.assert_allclose(got[k].numpy(), r, rtol=2e-4, atol=2e-6 * scale + 1e-9, err_msg=f"image {i} {k}")
        # one Adam step on the reduced gradient; the clamped ranges are projected afterwards and are left out
        p = params[i].cpu().clone().requires_grad_(True)
        p.grad = g[i].cpu().clone()
        torch.optim.Adam([p], lr=1e-2).step()
        want, new = amd.unpack_params(spec, p.detach()), amd.unpack_params(spec, one.params[i].cpu())
        for k in want:
            if not _clamped(k):
                np.testing.assert_allclose(new[k].numpy(), want[k].numpy(), rtol=1e-4, atol=2e-5, err_msg=f"image {i} {k}")


def _last_slab_point(slabs):
    return 64 * (slabs - 1) + 3   # chunk c goes to workgroup c % slabs: a point of chunk slabs - 1


@pytest.mark.parametrize("h,L", [(130, 1), (64, 2)])
@pytest.mark.parametrize("slabs", [2, 17, 256])
def test_nan_in_the_last_slab_freezes_the_icnn_fit(amd, slabs, h, L):
    spec, params, grid, un, _ = _problem(amd, slabs, h, L)
    P = spec.n_params
    bad = un.clone()
    bad[0, _last_slab_point(slabs)] = float("nan")
    opt0 = amd.icnn.new_opt_state(spec, 2, params.device)
    opt0[:, :2 * P] = torch.rand(2, 2 * P, device=params.device) * 1e-3   # moments that a step would change
    with slab_base(amd, _base_for(slabs, 2)):
        both = amd.fit(spec, params.clone(), grid, bad, 3, lr=2e-3, opt_state=opt0.clone(), want_logits=False)
    with slab_base(amd, _base_for(slabs, 1)):
        assert amd._lib.load().inrfit_slabs_per_image(grid.n_points, 1) == slabs
        alone = amd.fit(spec, params[1:].clone(), grid, un[1:], 3, lr=2e-3, opt_state=opt0[1:].clone(), want_logits=False)
    assert both.status.cpu().tolist() == [1, 0] and int(alone.status[0]) == 0
    assert torch.equal(both.params[0], params[0])
    assert torch.equal(both.opt_state[0, :2 * P], opt0[0, :2 * P])
    assert torch.equal(both.params[1], alone.params[0]) and not torch.equal(both.params[1], params[1])
    assert torch.equal(both.opt_state[1, :2 * P], alone.opt_state[0, :2 * P])
    assert torch.equal(both.loss_hist[1], alone.loss_hist[0])


@pytest.mark.parametrize("h", [64, 130])
@pytest.mark.parametrize("base", [2, 17, 0])
def test_nan_in_the_last_slab_freezes_both_parameter_sets_of_the_deformed_fits(amd, base, h):
    """cdn_fit / pcn_fit at 64x64 (64 chunks): 2, 17 and 64 slabs.  n_hidden 130 runs both updates in one launch, the deformation's blocks
    taking the decision from the dense partials themselves (frozen_in_launch); 64 runs the two launches."""
    from awesome_amd import flow as FL, rnvp as R
    from awesome_amd.dataset import convex_blob_unaries
    from awesome_amd.model import ConvexDiffeomorphismNet, real_nvp_path_connected_net
    dev = torch.device("cuda:0")
    slabs = base or 64
    g64 = amd.Grid.linspace(64, 64, dev)
    u64 = convex_blob_unaries(256, 0).reshape(256, 256)[::4, ::4].reshape(1, -1).contiguous().to(dev)
    u64[0, _last_slab_point(slabs)] = float("nan")
    torch.manual_seed(4)
    cdn = ConvexDiffeomorphismNet(n_hidden=h, n_hidden_layers=1, nf_layers=4, nf_hidden=24, diffeo_args=dict(backbone="normal_block"))
    pcn = real_nvp_path_connected_net(channels=2, hidden_units=16, flow_n_flows=4, flow_output_fn="tanh", convex_net_hidden_units=h)
    with slab_base(amd, base):
        assert amd._lib.load().inrfit_slabs_per_image(64 * 64, 1) == slabs
        ispec, fspec = cdn._specs()
        flat = cdn._engine_pack(cdn.state_dict()).to(dev)[None]
        ip, fp = flat[:, :ispec.n_params].contiguous(), flat[:, ispec.n_params:].contiguous()
        r = FL.cdn_fit(ispec, fspec, ip.clone(), fp.clone(), g64, u64, 3)
        assert int(r.status[0]) == 1 and torch.equal(r.icnn_params, ip) and torch.equal(r.flow_params, fp)
        assert not r.icnn_opt_state[:, :2 * ispec.n_params].any() and not r.flow_opt_state[:, :2 * fp.shape[1]].any()
        ispec, rspec = pcn._specs()
        flat = pcn._engine_pack(pcn.state_dict()).to(dev)[None]
        ip, fp = flat[:, :ispec.n_params].contiguous(), flat[:, ispec.n_params:].contiguous()
        R.actnorm_init(rspec, fp, g64)
        r = R.pcn_fit(ispec, rspec, ip.clone(), fp.clone(), g64, u64, 3)
        assert int(r.status[0]) == 1 and torch.equal(r.icnn_params, ip) and torch.equal(r.flow_params, fp)
        assert not r.icnn_opt_state[:, :2 * ispec.n_params].any() and not r.flow_opt_state[:, :2 * fp.shape[1]].any()


@pytest.mark.parametrize("h,L", [(130, 1), (64, 2)])
def test_poisoned_workspace_at_17_slabs(amd, h, L):
    """every byte a fit reads has been written by it: the dense loss partials are part of the (NaN-filled) workspace"""
    spec, params, grid, un, _ = _problem(amd, 17, h, L)
    runs = []
    try:
        for poison in (True, False):
            amd._lib.POISON = poison
            runs.append(amd.fit(spec, params.clone(), grid, un, 20, lr=2e-3, record_loss=True, want_logits=True))
    finally:
        amd._lib.POISON = False
    a, b = runs
    assert int(a.status.sum()) == 0
    assert torch.isfinite(a.params).all() and torch.isfinite(a.loss_hist).all() and torch.isfinite(a.logits).all()
    assert torch.equal(a.params, b.params) and torch.equal(a.opt_state, b.opt_state)
    assert torch.equal(a.loss_hist, b.loss_hist) and torch.equal(a.logits, b.logits)
