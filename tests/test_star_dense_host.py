"""The star-shape prior's dense fits on the host (no GPU): the binding, the argument checks of the new entry points (answered before
the first HIP call), the module's PriorFitMixin pieces, the joint routing and the `star` kind of the synthetic data."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_abi import _declared_functions

_FAKE = 0x1000   # a device pointer that is never dereferenced: every case below is answered on the host
_EINVAL, _EUNSUPPORTED, _EWORKSPACE = -1, -2, -3
_NEW = ("inrfit_star_dense_tile_points", "inrfit_star_opt_state_floats", "inrfit_star_dense_workspace_bytes", "inrfit_star_fit_dense",
        "inrfit_star_loss_grad_dense")


def test_exports_equal_the_header_and_the_version_script_and_the_abi_stays_8():
    import os
    from awesome_amd import _lib
    names = _declared_functions()
    assert set(_lib.EXPORTS) == set(names)
    for must in _NEW:
        assert must in names
    # the version script exports the header's prefix and nothing else
    script = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "inrfit.map")).read()
    assert "global: inrfit_*;" in script and "local: *;" in script
    lib = _lib.load()
    for must in _NEW:
        assert hasattr(lib, must)
    ver = ctypes.c_int()
    assert lib.inrfit_query(ctypes.byref(ver), None, None) == 0 and ver.value == 8 == _lib.INRFIT_ABI_VERSION   # additions only
    assert ctypes.sizeof(_lib.InrStarDesc) == 4


def test_size_queries():
    from awesome_amd import _lib as L
    from awesome_amd import star as S
    lib = L.load()
    T = lib.inrfit_star_dense_tile_points()
    assert T == S.dense_tile_points() and T > 0 and T % 64 == 0
    for h in (1, 33, 130, 1024):
        d = L.InrStarDesc(h)
        P = h * h + 8 * h + 4
        assert lib.inrfit_star_opt_state_floats(d) == 2 * P + L.INR_OPT_HEADER_FLOATS == S.opt_state_floats(S.StarSpec(h))
        small, one, many = (lib.inrfit_star_dense_workspace_bytes(d, n, 1) for n in (100, T, 50 * T))
        assert 0 < small < one == many        # the workspace is bounded by the tile, whatever the image's size
        assert lib.inrfit_star_dense_workspace_bytes(d, T, 3) >= one
    assert lib.inrfit_star_opt_state_floats(L.InrStarDesc(0)) == _EUNSUPPORTED
    assert lib.inrfit_star_opt_state_floats(None) == _EUNSUPPORTED
    assert lib.inrfit_star_dense_workspace_bytes(L.InrStarDesc(2000), 10, 1) == _EUNSUPPORTED
    assert lib.inrfit_star_dense_workspace_bytes(L.InrStarDesc(8), 0, 1) == _EINVAL
    assert lib.inrfit_star_dense_workspace_bytes(L.InrStarDesc(8), 10, 0) == _EINVAL


# ---- single-fault table: a valid call with ONE argument spoiled, answered before the first HIP call -----------------------------------
def _args(**over):
    from awesome_amd import _lib as L
    a = dict(star=130, params=_FAKE, opt_state=_FAKE, coords=_FAKE, stride=0, targets=_FAKE, loss=(L.INR_LOSS_SE, L.INR_WEIGHT_NONE),
             opt=dict(), n_pixels=1000, n=2, steps=3, step0=0, first=0, status=_FAKE, loss_out=_FAKE, grads=_FAKE, ws=_FAKE,
             wsb=1 << 40)
    a.update(over)
    a["star"] = None if a["star"] is None else L.InrStarDesc(a["star"])
    a["loss"] = None if a["loss"] is None else L.InrLossDesc(*a["loss"], 1.0, 0.0, 0.0)
    if a["opt"] is not None:
        o = dict(kind=L.INR_OPT_ADAM, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, clamp=0, plateau=0, plateau_patience=2,
                 plateau_factor=0.5, plateau_threshold=1e-4, plateau_min_lr=0.0, plateau_eps=1e-8, freeze_skips=0, freeze_input=0,
                 logits_at_last_forward=0)
        o.update(a["opt"])
        a["opt"] = L.InrOptDesc(**o)
    return a


_ENTRY = {
    "fit": lambda lib, a: lib.inrfit_star_fit_dense(a["star"], a["params"], a["opt_state"], a["coords"], a["stride"], a["targets"],
                                                    a["loss"], a["opt"], a["n_pixels"], a["n"], a["steps"], a["step0"], a["first"], None,
                                                    None, a["status"], a["ws"], a["wsb"], None),
    "loss_grad": lambda lib, a: lib.inrfit_star_loss_grad_dense(a["star"], a["params"], a["coords"], a["stride"], a["targets"], a["loss"],
                                                                a["n_pixels"], a["n"], a["loss_out"], a["grads"], a["ws"], a["wsb"], None),
}
_BOTH = [
    (dict(star=None), _EUNSUPPORTED),
    (dict(star=0), _EUNSUPPORTED),
    (dict(star=1025), _EUNSUPPORTED),
    (dict(star=1025, wsb=16), _EUNSUPPORTED),     # the shape is answered in front of the workspace
    (dict(params=None), _EINVAL),
    (dict(coords=None), _EINVAL),
    (dict(targets=None), _EINVAL),
    (dict(loss=None), _EINVAL),
    (dict(loss=(2, 0)), _EINVAL),                 # INR_LOSS_EXTERNAL
    (dict(loss=(0, 9)), _EINVAL),
    (dict(loss=(0, -1)), _EINVAL),
    (dict(n_pixels=0), _EINVAL),
    (dict(n=0), _EINVAL),
    (dict(stride=-2000), _EINVAL),
    (dict(stride=1999), _EINVAL),                 # images would overlap: a stride is 0 or at least 2 n_pixels
    (dict(ws=None), _EINVAL),
    (dict(wsb=16), _EWORKSPACE),                  # a short workspace
    (dict(n_pixels=1 << 22, wsb=1 << 20), _EWORKSPACE),
]
_FIT = [
    (dict(opt=None), _EINVAL),
    (dict(opt=dict(kind=7)), _EINVAL),            # an unknown optimizer
    (dict(opt=dict(weight_decay=1e-5)), _EINVAL),
    (dict(opt=dict(clamp=1)), _EINVAL),
    (dict(opt=dict(freeze_skips=1)), _EINVAL),
    (dict(opt=dict(freeze_input=1)), _EINVAL),
    (dict(opt_state=None), _EINVAL),
    (dict(status=None), _EINVAL),
    (dict(steps=-1), _EINVAL),
    (dict(step0=-1), _EINVAL),
]
_LG = [(dict(loss_out=None), _EINVAL), (dict(grads=None), _EINVAL)]
_TABLE = [("fit", o, rc) for o, rc in _BOTH + _FIT] + [("loss_grad", o, rc) for o, rc in _BOTH + _LG]


@pytest.mark.parametrize("entry,over,want", _TABLE, ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in o.items())}" for e, o, _ in _TABLE])
def test_one_spoiled_argument_is_rejected_on_the_host(entry, over, want):
    from awesome_amd import _lib as L
    assert _ENTRY[entry](L.load(), _args(**over)) == want


def test_binding_refuses_bad_tensors_before_the_library():
    from awesome_amd import _lib as L
    from awesome_amd import star as S
    spec = S.StarSpec(8)
    p, x, t = torch.zeros(2, spec.n_params), torch.zeros(10, 2), torch.zeros(2, 10)
    with pytest.raises(ValueError):
        S.star_fit_dense(spec, p[0], x, t, 1)                      # params must be [n, P]
    with pytest.raises(ValueError):
        S.star_fit_dense(spec, p, x, t[:, :9], 1)                  # one target per pixel
    with pytest.raises(ValueError):
        S.star_fit_dense(spec, p, torch.zeros(3, 10, 2), t, 1)     # per-image coords: one grid per image
    with pytest.raises(ValueError):
        S.star_fit_dense(spec, p, x, t, 1, opt_state=torch.zeros(2, 5))
    with pytest.raises(L.InrfitError):
        S.star_fit_dense(spec, p, x, t, 1)                         # CPU tensors: no CPU path
    with pytest.raises(L.InrfitError):
        S.star_loss_grad_dense(spec, p, x, t)


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def test_module_reset_pack_unpack_and_parameter_order():
    from awesome_amd import star as S
    from awesome_amd.model import StarShapedNet
    from awesome_amd.model.pretrainable_module import PriorFitMixin
    torch.manual_seed(3)
    m = StarShapedNet(9)
    assert isinstance(m, PriorFitMixin)
    assert tuple(k for k, _ in m.named_parameters()) == S.PARAM_ORDER == tuple(m.state_dict().keys())
    first = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        m.offset.copy_(torch.tensor([[0.3, -0.2]]))
        for p in m.parameters():
            p.add_(1.0)
    torch.manual_seed(3)
    assert m.reset_parameters() is True
    for k, v in m.state_dict().items():                            # a seeded reset redraws what the seeded construction drew
        assert torch.equal(v, first[k]), k
    assert torch.equal(m.offset, torch.zeros(1, 2))
    flat = m._engine_pack(m.state_dict())
    assert flat.shape == (m.star_spec.n_params,) and flat.dtype == torch.float32
    assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for p in m.parameters()]))    # PriorBank's row = the flat vector
    back = m._engine_unpack(flat)
    assert list(back) == list(S.PARAM_ORDER)
    for k, v in m.state_dict().items():
        assert back[k].shape == v.shape and torch.equal(back[k], v), k
    d = m._pretrain_defaults()
    assert d["num_epochs"] == 2000 and d["lr"] == 1e-2 and d["optimizer"] == "adam" and d["use_plateau"] is False
    assert d["init_center"] == "center_of_mass" and d["proper_prior_fit_threshold"] == 0.5 and d["proper_prior_fit_retrys"] == 1
    assert d["reuse_state"] is True and d["reuse_state_epochs"] == 200


def test_centre_initialisation_and_warm_start_shift():
    from awesome_amd.model import StarShapedNet
    from awesome_amd.model.pretrainable_module import _Image
    from awesome_amd.model.star_net import foreground_mean
    H, W = 5, 7
    xs, ys = torch.linspace(0, 1, W), torch.linspace(0, 1, H)
    grid = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W)], 0)[None].contiguous()    # (1, 2, H, W)

    def frame(r0, r1, c0, c1):
        un = torch.ones(1, 1, H, W)
        un[0, 0, r0:r1, c0:c1] = 0.2
        return _Image(0, 0, None, un, grid, False)

    a, b = frame(1, 3, 2, 5), frame(2, 5, 3, 7)
    ma = foreground_mean(a.grid, a.unaries)
    np.testing.assert_allclose(ma.numpy(), [xs[2:5].mean(), ys[1:3].mean()], rtol=1e-6)
    np.testing.assert_allclose(foreground_mean(grid[0].reshape(2, -1), a.unaries.reshape(-1)).numpy(), ma.numpy(), rtol=1e-6)
    np.testing.assert_allclose(foreground_mean(grid, torch.ones(H, W)).numpy(), [0.5, 0.5], rtol=1e-6)   # no foreground: all pixels
    m = StarShapedNet(4)
    flat = m._engine_pack(m.state_dict())
    flat[0:2] = torch.tensor([-0.4, -0.3])
    keep = flat.clone()
    out, ctx = m._engine_warm_start(flat.clone(), None, b, {})      # no previous frame: nothing moves
    assert ctx is None and torch.equal(out, keep)
    ctx = m._engine_chain_context(None, a)
    assert torch.equal(ctx, ma)
    out, ctx2 = m._engine_warm_start(flat.clone(), ctx, b, {})
    mb = foreground_mean(b.grid, b.unaries)
    np.testing.assert_allclose(out[0:2].numpy(), (keep[0:2] - (mb - ma)).numpy(), rtol=1e-6)
    assert torch.equal(out[2:], keep[2:]) and torch.equal(ctx2, ma)


def test_joint_routing_refuses_the_star_prior():
    """StarShapedNet.spec is the ICNN shape of its autograd bridge, not the layout of its parameter vector: no fused joint step."""
    from awesome_amd.agent import _fused_prior_family
    from awesome_amd.model import ConvexNextNet, StarShapedNet
    for kind in ("adam", "adamax"):
        for lbl in (False, True):
            assert _fused_prior_family(StarShapedNet(130), kind, lbl) is None
            assert _fused_prior_family(StarShapedNet(150), kind, lbl) is None
    fam = _fused_prior_family(ConvexNextNet(n_hidden=130, n_hidden_layers=1, in_features=2), "adam", False)
    assert fam is not None and fam[0] == "icnn" and fam[2] is None and fam[3] is False       # the ICNN route is as it was


# ---- data ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [33, 64])
def test_star_kind_is_seeded_star_shaped_and_not_convex(size):
    from awesome_amd.dataset import SyntheticUnariesDataset, star_mask, star_shape
    ds = SyntheticUnariesDataset(n_images=4, size=size, kind="star", seed0=5)
    again = SyntheticUnariesDataset(n_images=4, size=size, kind="star", seed0=5)
    lin = np.linspace(0.0, 1.0, size)
    seen = []
    for i in range(4):
        un = ds.unaries(i)
        assert un.shape == (size, size) and un.dtype == torch.float32 and torch.equal(un, again.unaries(i))
        assert set(np.unique(un.numpy())) == {0.0, 1.0}             # the unaries convention: fg = 0
        mask = un.numpy() < 0.5
        assert np.array_equal(mask, star_mask(size, 5 + i)) and 0.05 < mask.mean() < 0.5
        seen.append(mask)
        cx, cy, r0, a, k, phase = star_shape(5 + i)
        assert a * (k * k + 1) > r0                                 # the curve is not convex
        # star-shaped about the centre: every point of the segment from the centre to a foreground pixel's own position lies in the
        # region (judged by the region's inequality - a pixel raster has no segments of its own)
        rows, cols = np.nonzero(mask)
        for t in (0.25, 0.5, 0.75, 0.999):
            x, y = cx + t * (lin[cols] - cx), cy + t * (lin[rows] - cy)
            assert np.all(np.hypot(x - cx, y - cy) <= r0 + a * np.cos(k * (np.arctan2(y - cy, x - cx) - phase)) + 1e-12)
        # not convex on the raster either: two foreground pixels whose midpoint pixel is background
        found = False
        for (r1, c1) in zip(rows[::7], cols[::7]):
            mr, mc = (rows + r1), (cols + c1)
            even = (mr % 2 == 0) & (mc % 2 == 0)
            if np.any(~mask[mr[even] // 2, mc[even] // 2]):
                found = True
                break
        assert found
    assert not np.array_equal(seen[0], seen[1])
