"""The rotation-symmetric prior's device fits on the host (no GPU): the binding, the argument checks of every new entry point, the
size queries, the conditions the GPU parity cases lean on, and the pose's chain rule against autograd."""
import ctypes

import pytest
import torch

from oracle import inr_oracle as O  # (checker only)
from tests import sym_cases as SC
from tests.test_abi import _declared_functions

_FAKE = 0x1000   # a device pointer that is never dereferenced: every case below is answered on the host
_EINVAL, _EUNSUPPORTED, _EWORKSPACE = -1, -2, -3
_NEW = ("inrfit_sym_workspace_bytes", "inrfit_sym_minibatch_workspace_bytes", "inrfit_sym_forward", "inrfit_sym_loss_grad",
        "inrfit_sym_fit", "inrfit_sym_fit_minibatch")


def test_exports_equal_the_header_and_hold_the_new_names():
    from awesome_amd import _lib
    names = _declared_functions()
    assert set(_lib.EXPORTS) == set(names)
    for must in _NEW:
        assert must in names
    lib = _lib.load()
    ver = ctypes.c_int()
    assert lib.inrfit_query(ctypes.byref(ver), None, None) == 0 and ver.value == 8   # additions only
    assert ctypes.sizeof(_lib.InrSymDesc) == 8


# ---- single-fault tables: a valid call with ONE argument spoiled, answered before the first HIP call ----------------------------------
def _args(**over):
    from awesome_amd import _lib as L
    a = dict(model=(130, 3, 1, 0, 0, 0), sym=(3, 0.001), loss=(L.INR_LOSS_SE, L.INR_WEIGHT_NONE), opt=L.INR_OPT_ADAM, params=_FAKE,
             pose=_FAKE, opt_state=_FAKE, pose_opt=_FAKE, coords=_FAKE, targets=_FAKE, n_points=1000, logits=_FAKE, loss_out=_FAKE,
             grads=_FAKE, pose_grads=_FAKE, n_pool=1000, index=_FAKE, counts=None, batch=200, n=1, steps=3, step0=0, ws=_FAKE, wsb=1 << 40)
    a.update(over)
    h, c, layers, act0, nf, no = a["model"]
    a["model"] = L.InrModelDesc(L.INR_MODEL_ICNN, h, c, layers, act0, 1.0, nf, no)
    a["sym"] = None if a["sym"] is None else L.InrSymDesc(*a["sym"])
    a["loss"] = None if a["loss"] is None else L.InrLossDesc(*a["loss"], 1.0, 0.0, 0.0)
    a["opt"] = None if a["opt"] is None else L.InrOptDesc(a["opt"], 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 1, 0, 0)
    a["grid"] = L.InrGridDesc(L.INR_GRID_EXPLICIT, 0, 0, a["n_points"], None, None, None, a["coords"], 0)
    if a["counts"] is not None:
        a["counts"] = (ctypes.c_int32 * len(a["counts"]))(*a["counts"])
    return a


_ENTRY = {
    "forward": lambda lib, a: lib.inrfit_sym_forward(a["model"], a["sym"], a["params"], a["pose"], a["grid"], a["n"], 1, a["logits"],
                                                     a["ws"], a["wsb"], None),
    "loss_grad": lambda lib, a: lib.inrfit_sym_loss_grad(a["model"], a["sym"], a["params"], a["pose"], a["grid"], a["targets"], a["loss"],
                                                         a["n"], 1, a["loss_out"], a["grads"], a["pose_grads"], a["ws"], a["wsb"], None),
    "fit": lambda lib, a: lib.inrfit_sym_fit(a["model"], a["sym"], a["params"], a["pose"], a["opt_state"], a["pose_opt"], a["grid"],
                                             a["targets"], a["loss"], a["opt"], a["n"], a["steps"], a["step0"], None, None, a["ws"],
                                             a["wsb"], None),
    "mb": lambda lib, a: lib.inrfit_sym_fit_minibatch(a["model"], a["sym"], a["params"], a["pose"], a["opt_state"], a["pose_opt"],
                                                      a["coords"], a["targets"], a["n_pool"], a["index"], a["counts"], a["batch"],
                                                      a["loss"], a["opt"], a["n"], a["steps"], a["step0"], None, None, a["ws"], a["wsb"],
                                                      None),
}
_WIDE, _TWO_CH, _FIVE_CH, _HUGE, _FOURIER = (150, 3, 1, 0, 0, 0), (130, 2, 1, 0, 0, 0), (130, 5, 1, 0, 0, 0), (1777, 3, 1, 0, 0, 0), (48, 3, 3, 1, 20, 3)
_ALL = [                                                   # every entry point
    (dict(params=None), _EINVAL),
    (dict(pose=None), _EINVAL),
    (dict(sym=None), _EINVAL),
    (dict(sym=(3, 0.0)), _EINVAL),                          # r_eps
    (dict(n=0), _EINVAL),
    (dict(ws=None), _EINVAL),
    (dict(model=_TWO_CH), _EUNSUPPORTED),                   # in_features != 3
    (dict(model=_FIVE_CH), _EUNSUPPORTED),
    (dict(model=_HUGE), _EUNSUPPORTED),                     # neither a fused kernel nor a layer-by-layer form
    (dict(model=_FOURIER), _EUNSUPPORTED),                  # (a periodic layer 0 is no ICNN form)
    (dict(model=_HUGE, wsb=16), _EUNSUPPORTED),             # the shape is answered in front of the workspace
    (dict(wsb=16), _EWORKSPACE),
    (dict(model=_WIDE, wsb=16), _EWORKSPACE),
    (dict(model=_WIDE, ws=None), _EINVAL),
]
_GRID = [(dict(coords=None), _EINVAL), (dict(n_points=0), _EINVAL)]                               # forward, loss_grad, fit
_LOSS = [(dict(targets=None), _EINVAL), (dict(loss=None), _EINVAL), (dict(loss=(2, 0)), _EINVAL),  # INR_LOSS_EXTERNAL
         (dict(loss=(0, 9)), _EINVAL)]                                                            # loss_grad, fit, mb
_FIT = [(dict(opt_state=None), _EINVAL), (dict(pose_opt=None), _EINVAL), (dict(opt=None), _EINVAL), (dict(opt=1), _EINVAL),   # Adamax
        (dict(opt=7), _EINVAL), (dict(steps=-1), _EINVAL), (dict(step0=-1), _EINVAL),
        (dict(model=_HUGE, steps=-1), _EINVAL)]                                                   # ... behind the plain arguments
_FAULTS = ([(e, f, c) for e in _ENTRY for f, c in _ALL] + [(e, f, c) for e in ("forward", "loss_grad", "fit") for f, c in _GRID] +
           [(e, f, c) for e in ("loss_grad", "fit", "mb") for f, c in _LOSS] + [(e, f, c) for e in ("fit", "mb") for f, c in _FIT] + [
    ("forward", dict(logits=None), _EINVAL),
    ("loss_grad", dict(loss_out=None), _EINVAL),
    ("loss_grad", dict(grads=None), _EINVAL),
    ("loss_grad", dict(pose_grads=None), _EINVAL),
    ("mb", dict(coords=None), _EINVAL),
    ("mb", dict(index=None), _EINVAL),
    ("mb", dict(n_pool=0), _EINVAL),
    ("mb", dict(batch=0), _EINVAL),
    ("mb", dict(counts=[200, 0, 5]), _EINVAL),
    ("mb", dict(counts=[200, 201, 5]), _EINVAL),
    ("mb", dict(model=_HUGE, n_pool=0), _EINVAL),
    ("mb", dict(wsb=200 * 4 * 3 + 1024), _EWORKSPACE),     # the staging buffers fit, the step's workspace does not
    ("mb", dict(counts=[200, 3, 64], wsb=16), _EWORKSPACE),
])


@pytest.mark.parametrize("entry,fault,code", _FAULTS, ids=[f"{e}-{'-'.join(f)}-{i}" for i, (e, f, _) in enumerate(_FAULTS)])
def test_single_fault_codes(entry, fault, code):
    from awesome_amd import _lib
    assert _ENTRY[entry](_lib.load(), _args(**fault)) == code


def test_size_queries():
    from awesome_amd import _lib as L
    lib = L.load()
    for model in ((130, 3, 1, 0, 0, 0), (32, 3, 1, 0, 0, 0), _WIDE):
        a = _args(model=model)
        one = lib.inrfit_sym_workspace_bytes(a["model"], a["grid"], 1)
        assert one > 3 * 1000 * 4 * 2
        assert lib.inrfit_sym_workspace_bytes(a["model"], a["grid"], 2) > one                         # grows with n_images
        assert lib.inrfit_sym_workspace_bytes(a["model"], _args(n_points=2000)["grid"], 1) > one      # ... and with the points
        mb = lib.inrfit_sym_minibatch_workspace_bytes(a["model"], 200, 1)
        assert lib.inrfit_sym_minibatch_workspace_bytes(a["model"], 300, 1) > mb                      # grows with batch
        assert lib.inrfit_sym_minibatch_workspace_bytes(a["model"], 200, 2) > mb                      # ... and with n_images
        # at least the staging planes (2 coordinates, the targets) plus the step's own workspace for every count
        worst = max(lib.inrfit_sym_workspace_bytes(a["model"], _args(n_points=c)["grid"], 1) for c in range(1, 201))
        assert 3 * 200 * 4 + worst <= mb < 3 * 200 * 4 + worst + 4096
        assert lib.inrfit_sym_workspace_bytes(a["model"], a["grid"], 0) == _EINVAL
        assert lib.inrfit_sym_workspace_bytes(a["model"], None, 1) == _EINVAL
        assert lib.inrfit_sym_minibatch_workspace_bytes(a["model"], 0, 1) == _EINVAL
        assert lib.inrfit_sym_minibatch_workspace_bytes(a["model"], 200, 0) == _EINVAL
    for bad in (_TWO_CH, _FIVE_CH, _HUGE, _FOURIER):
        a = _args(model=bad)
        assert lib.inrfit_sym_workspace_bytes(a["model"], a["grid"], 1) == _EUNSUPPORTED
        assert lib.inrfit_sym_minibatch_workspace_bytes(a["model"], 200, 1) == _EUNSUPPORTED
    assert lib.inrfit_sym_workspace_bytes(None, _args()["grid"], 1) == _EUNSUPPORTED


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def test_cases_have_the_shapes_they_claim():
    c = SC.case("sym130x2")
    assert tuple(c.index.shape) == (6, 200) and c.pool_coords.shape == (2, 1440) and c.n_images == 2
    assert not torch.equal(c.pool_targets[0], c.pool_targets[1])
    lik = c.pool_targets[0]
    assert 900 <= int((lik < 0.5).sum()) <= 1000 and 440 <= int((lik >= 0.5).sum()) <= 540 and float((lik - 0.5).abs().min()) >= 0.02
    assert tuple(SC.case("sym32").index.shape) == (6, 192) and SC.case("sym32").modules[0].spec.n_hidden == 32
    assert tuple(SC.case("sym150").index.shape) == (6, 200) and SC.case("sym150").modules[0].spec.n_hidden == 150
    assert SC.case("sym150_loader").counts == [64, 64, 3] * 2 and SC.case("sym150_loader").pool_coords.shape == (2, 131)
    assert SC.case("sym130_full").index is None and SC.case("sym130_full").steps == 6
    assert SC.case("sym32_wd").kw["weight_decay"] > 0 and torch.equal(SC.case("sym32_wd").index, SC.case("sym32").index)
    for name in SC.ALL_CASES:
        for m in SC.case(name).modules:
            assert m._pose().tolist() == [pytest.approx(0.013), pytest.approx(-0.021), pytest.approx(0.3)]
        assert SC.case(name).kw["symmetry_from_step"] == 3 and SC.case(name).steps == 6   # the switch falls inside the call


@pytest.mark.parametrize("name", SC.ALL_CASES)
def test_case_conditions(name):
    """The |v| kink and the 1 / r pole make float32 and float64 legitimately disagree at points that sit on them: on the float64
    trajectory every drawn point of every step keeps its distance.  And what the parity bars lean on: finite restatements, e32 > 0
    that is rounding and not a different loop, parameters and pose that move."""
    r = SC.references(name)
    assert r["min_v0"] >= SC.MIN_V0 and r["min_r"] >= SC.MIN_R, (r["min_v0"], r["min_r"])
    assert SC.finite(r["net"], r["pose"], r["hist"])
    for e, ref in ((r["e_net"], r["net"]), (r["e_pose"], r["pose"]), (r["e_hist"], r["hist"])):
        assert 0 < e < 1e-3 * float(ref.abs().max())
    c = SC.case(name)
    start = torch.stack([m._pose() for m in c.modules]).double()
    assert float((r["pose"] - start).abs().min()) > 1e-4       # every pose parameter of every image took its steps
    assert bool((r["hist"] > 0).all())


@pytest.mark.parametrize("h,n", [(130, 1440), (130, 193), (150, 1440), (150, 193)])
def test_gradient_reference_conditions(h, n):
    for sym in (False, True):
        g = SC.gradient_reference(h, n, sym)
        assert g["min_v0"] >= SC.MIN_V0 and g["min_r"] >= SC.MIN_R
        assert g["e_net"] > 0 and g["e_pose"] > 0 and float(g["pose"].abs().min()) > 1e-5


# ---- the kernel's arithmetic, checkable without a GPU ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [False, True], ids=["free", "mirror"])
def test_pose_gradient_formulas_match_autograd(sym):
    g0 = torch.Generator().manual_seed(31)
    x = torch.rand(257, 2, dtype=torch.float64, generator=g0) - 0.5
    g = torch.randn(257, 3, dtype=torch.float64, generator=g0)
    off = torch.tensor([SC.OFFSET], dtype=torch.float64, requires_grad=True)
    th = torch.tensor([SC.ORIENTATION], dtype=torch.float64, requires_grad=True)
    (O.rotation_symmetric_features(x, off, th, sym) * g).sum().backward()
    do, dth = SC.pose_gradient(x, off.detach(), th.detach(), g, sym)
    assert float((do - off.grad[0]).abs().max()) < 1e-11 * float(off.grad.abs().max())
    assert abs(float(dth - th.grad[0])) < 1e-11 * abs(float(th.grad[0]))


def test_pose_gradient_guards_the_centre():
    """A point at -offset has r == 0: autograd yields NaN there, the stated formulas leave it out."""
    x = torch.tensor([[-SC.OFFSET[0], -SC.OFFSET[1]], [0.2, 0.1], [-0.3, 0.25]], dtype=torch.float64)
    g = torch.ones(3, 3, dtype=torch.float64)
    off, th = torch.tensor([SC.OFFSET], dtype=torch.float64), torch.tensor([SC.ORIENTATION], dtype=torch.float64)
    do, dth = SC.pose_gradient(x, off, th, g, True)
    do2, dth2 = SC.pose_gradient(x[1:], off, th, g[1:], True)
    assert SC.finite(do, dth) and torch.equal(do, do2) and torch.equal(dth, dth2)
