"""The Python binding's shared call path (awesome_amd/_call.py), without a GPU: the optimizer descriptor every fit / step wrapper hands
the library, the argument checks in front of every entry point, the workspace query and the marshalling.

The expected descriptors are written out here from the wrappers' call sites as they stood before the binding was unified; the
plateau_* fields of a switched-off plateau are the one unified set (the library reads them only behind `plateau`)."""
import ctypes

import pytest
import torch

import awesome_amd as A
from awesome_amd import _call as X
from awesome_amd import _lib as L
from awesome_amd import flow as FL
from awesome_amd import icnn as K
from awesome_amd import joint as J
from awesome_amd import minibatch as MB
from awesome_amd import rnvp as R
from awesome_amd import star as ST
from awesome_amd import symmetric as SY

H, W_, H_, N, NI = 8, 4, 3, 12, 2          # h = 8, a 4 x 3 grid = 12 points, two images
ISPEC, SSPEC = A.IcnnSpec(H, 2, 1), A.IcnnSpec(H, 3, 1)
FSPEC, RSPEC, STAR = FL.FlowSpec(8, 2), R.RnvpSpec(2, 8, 2), ST.StarSpec(H)
P, SP, FP, RP = ISPEC.n_params, SSPEC.n_params, FSPEC.n_params, RSPEC.n_params
T, STEPS, BATCH = 3, 2, 5
ADAM, ADAMAX = 0, 1
OFF = (0, 200, 0.5, 1e-4, 0.0, 1e-8)       # plateau, patience, factor, threshold, min_lr, eps while it is off
PL = {"patience": 3, "factor": 0.25}
ON = (1, 3, 0.25, 1e-4, 0.0, 1e-8)


def z(*shape):
    return torch.zeros(*shape)


def grid():
    return K.Grid.linspace(W_, H_, "cpu")


def index():
    return torch.zeros(STEPS, BATCH, dtype=torch.int32)


def orders():
    return torch.arange(T)[None].repeat(2, 1)


def joint_args(n=1):
    return dict(grid=grid(), seg=z(N), target=z(N), desc=J.joint_desc(), step=1, lr=1e-3)


def prior_args():
    return dict(grid=grid(), seg=z(N), target=z(N), desc=J.joint_prior_desc(), step=1, lr=1e-3, seg_term=z(1))


def icnn_row():
    return dict(spec=ISPEC, params=z(P), opt_state=z(2 * P + 8))


def flow_rows(fspec_name, fspec, fp):
    return {"ispec": ISPEC, fspec_name: fspec, "icnn_params": z(1, P), "flow_params": z(1, fp), "icnn_opt_state": z(1, 2 * P + 8),
            "flow_opt_state": z(1, 2 * fp)}


# name -> (function, a valid set of arguments on the CPU, the tensor arguments to spoil one at a time)
WRAPPERS = {
    "forward": (K.forward, lambda: dict(spec=ISPEC, params=z(NI, P), grid=grid()), ["params"]),
    "loss_grad": (K.loss_grad, lambda: dict(spec=ISPEC, params=z(NI, P), grid=grid(), targets=z(NI, N)), ["params", "targets"]),
    "backward": (K.backward, lambda: dict(spec=ISPEC, params=z(NI, P), grid=grid(), dlogits=z(NI, N)), ["params", "dlogits"]),
    "step_only": (K.step_only, lambda: dict(spec=ISPEC, params=z(NI, P), grid=grid(), targets=z(NI, N), iters=1), ["params", "targets"]),
    "fit": (K.fit, lambda: dict(spec=ISPEC, params=z(NI, P), grid=grid(), targets=z(NI, N), steps=STEPS, opt_state=z(NI, 2 * P + 8)),
            ["params", "targets", "opt_state"]),
    "flow_forward": (FL.flow_forward, lambda: dict(fspec=FSPEC, flow_params=z(NI, FP), grid=grid()), ["flow_params"]),
    "flow_backward": (FL.flow_backward, lambda: dict(fspec=FSPEC, flow_params=z(NI, FP), grid=grid(), dout_coords=z(NI, 2, N)),
                      ["flow_params", "dout_coords"]),
    "cdn_forward": (FL.cdn_forward, lambda: dict(ispec=ISPEC, fspec=FSPEC, icnn_params=z(NI, P), flow_params=z(NI, FP), grid=grid()),
                    ["icnn_params", "flow_params"]),
    "cdn_loss_grad": (FL.cdn_loss_grad, lambda: dict(ispec=ISPEC, fspec=FSPEC, icnn_params=z(NI, P), flow_params=z(NI, FP), grid=grid(),
                                                     targets=z(NI, N)), ["icnn_params", "flow_params", "targets"]),
    "cdn_fit": (FL.cdn_fit, lambda: dict(ispec=ISPEC, fspec=FSPEC, icnn_params=z(NI, P), flow_params=z(NI, FP), grid=grid(), targets=z(NI, N),
                                         steps=STEPS, icnn_opt_state=z(NI, 2 * P + 8), flow_opt_state=z(NI, 2 * FP)),
                ["icnn_params", "flow_params", "targets", "icnn_opt_state", "flow_opt_state"]),
    "actnorm_init": (R.actnorm_init, lambda: dict(rspec=RSPEC, flow_params=z(NI, RP), grid=grid()), ["flow_params"]),
    "rnvp_forward": (R.rnvp_forward, lambda: dict(rspec=RSPEC, flow_params=z(NI, RP), grid=grid()), ["flow_params"]),
    "rnvp_backward": (R.rnvp_backward, lambda: dict(rspec=RSPEC, flow_params=z(NI, RP), grid=grid(), dout=z(NI, 2, N)), ["flow_params", "dout"]),
    "rnvp_inverse": (R.rnvp_inverse, lambda: dict(rspec=RSPEC, flow_params=z(NI, RP), coords=z(NI, 2, N)), ["flow_params", "coords"]),
    "rnvp_inverse_shared": (R.rnvp_inverse, lambda: dict(rspec=RSPEC, flow_params=z(NI, RP), coords=z(2, N)), ["flow_params", "coords"]),
    "fit_identity": (R.fit_identity, lambda: dict(rspec=RSPEC, flow_params=z(NI, RP), grid=grid(), steps=STEPS, flow_opt_state=z(NI, 2 * RP)),
                     ["flow_params", "flow_opt_state"]),
    "pcn_forward": (R.pcn_forward, lambda: dict(ispec=ISPEC, rspec=RSPEC, icnn_params=z(NI, P), flow_params=z(NI, RP), grid=grid()),
                    ["icnn_params", "flow_params"]),
    "pcn_loss_grad": (R.pcn_loss_grad, lambda: dict(ispec=ISPEC, rspec=RSPEC, icnn_params=z(NI, P), flow_params=z(NI, RP), grid=grid(),
                                                    targets=z(NI, N)), ["icnn_params", "flow_params", "targets"]),
    "pcn_fit": (R.pcn_fit, lambda: dict(ispec=ISPEC, rspec=RSPEC, icnn_params=z(NI, P), flow_params=z(NI, RP), grid=grid(), targets=z(NI, N),
                                        steps=STEPS, icnn_opt_state=z(NI, 2 * P + 8), flow_opt_state=z(NI, 2 * RP)),
                ["icnn_params", "flow_params", "targets", "icnn_opt_state", "flow_opt_state"]),
    "pcn_fit_sequence": (R.pcn_fit_sequence,
                         lambda: dict(ispec=ISPEC, rspec=RSPEC, icnn_params=z(1, P), flow_params=z(1, RP), frame_coords=z(T, 2, N),
                                      frame_targets=z(T, N), orders=orders(), batch_size=2, icnn_opt_state=z(1, 2 * P + 8),
                                      flow_opt_state=z(1, 2 * RP)),
                         ["icnn_params", "flow_params", "frame_coords", "frame_targets", "icnn_opt_state", "flow_opt_state"]),
    "fit_identity_sequence": (R.fit_identity_sequence,
                              lambda: dict(rspec=RSPEC, flow_params=z(1, RP), frame_coords=z(T, 2, N), orders=orders(), batch_size=2,
                                           flow_opt_state=z(1, 2 * RP)), ["flow_params", "frame_coords", "flow_opt_state"]),
    "star_forward": (ST.star_forward, lambda: dict(spec=STAR, params=z(STAR.n_params), coords=z(N, 2)), ["params", "coords"]),
    "star_loss_grad": (ST.star_loss_grad, lambda: dict(spec=STAR, params=z(STAR.n_params), coords=z(N, 2), labels=z(N)),
                       ["params", "coords", "labels"]),
    "star_fit": (ST.star_fit, lambda: dict(spec=STAR, params=z(STAR.n_params), coords=z(N, 2), labels=z(N), batch_index=index(),
                                           opt_state=z(2 * STAR.n_params)), ["params", "coords", "labels", "opt_state"]),
    "fit_minibatch": (MB.fit_minibatch, lambda: dict(spec=ISPEC, params=z(NI, P), pool_coords=z(2, N), pool_targets=z(NI, N), index=index(),
                                                     opt_state=z(NI, 2 * P + 8)), ["params", "pool_coords", "pool_targets", "opt_state"]),
    "cdn_fit_minibatch": (MB.cdn_fit_minibatch,
                          lambda: dict(ispec=ISPEC, fspec=FSPEC, icnn_params=z(NI, P), flow_params=z(NI, FP), pool_coords=z(2, N),
                                       pool_targets=z(NI, N), index=index(), icnn_opt_state=z(NI, 2 * P + 8), flow_opt_state=z(NI, 2 * FP)),
                          ["icnn_params", "flow_params", "pool_coords", "pool_targets", "icnn_opt_state", "flow_opt_state"]),
    "sym_forward": (SY.sym_forward, lambda: dict(spec=SSPEC, params=z(NI, SP), pose=z(NI, 3), grid=grid()), ["params", "pose"]),
    "sym_loss_grad": (SY.sym_loss_grad, lambda: dict(spec=SSPEC, params=z(NI, SP), pose=z(NI, 3), grid=grid(), targets=z(NI, N)),
                      ["params", "pose", "targets"]),
    "sym_fit": (SY.sym_fit, lambda: dict(spec=SSPEC, params=z(NI, SP), pose=z(NI, 3), grid=grid(), targets=z(NI, N), steps=STEPS,
                                         opt_state=z(NI, 2 * SP + 8), pose_opt_state=z(NI, 6)),
                ["params", "pose", "targets", "opt_state", "pose_opt_state"]),
    "sym_fit_minibatch": (SY.sym_fit_minibatch,
                          lambda: dict(spec=SSPEC, params=z(NI, SP), pose=z(NI, 3), pool_coords=z(2, N), pool_targets=z(NI, N), index=index(),
                                       opt_state=z(NI, 2 * SP + 8), pose_opt_state=z(NI, 6)),
                          ["params", "pose", "pool_coords", "pool_targets", "opt_state", "pose_opt_state"]),
    "joint_step": (J.joint_step, lambda: dict(icnn_row(), **joint_args()), ["params", "opt_state", "seg", "target"]),
    "wide_joint_step": (J.wide_joint_step, lambda: dict(icnn_row(), **joint_args()), ["params", "opt_state", "seg", "target"]),
    "joint_prior_step": (J.joint_prior_step, lambda: dict(icnn_row(), **prior_args()), ["params", "opt_state", "seg", "target", "seg_term"]),
    "wide_joint_prior_step": (J.wide_joint_prior_step, lambda: dict(icnn_row(), **prior_args()),
                              ["params", "opt_state", "seg", "target", "seg_term"]),
    "pcn_joint_step": (J.pcn_joint_step, lambda: dict(flow_rows("rspec", RSPEC, RP), **joint_args()),
                       ["icnn_params", "flow_params", "icnn_opt_state", "flow_opt_state", "seg", "target"]),
    "pcn_wide_joint_step": (J.pcn_wide_joint_step, lambda: dict(flow_rows("rspec", RSPEC, RP), **joint_args()),
                            ["icnn_params", "flow_params", "icnn_opt_state", "flow_opt_state", "seg", "target"]),
    "cdn_joint_step": (J.cdn_joint_step, lambda: dict(flow_rows("fspec", FSPEC, FP), **joint_args()),
                       ["icnn_params", "flow_params", "icnn_opt_state", "flow_opt_state", "seg", "target"]),
}
CHANNEL_AXIS = {"pool_coords", "frame_coords", "coords"}     # spoiled by one more channel: their last axis is what the other widths follow


def spoiled(name, t):
    """One more column (channel, for the tensors whose last axis sets n_pool / HW)."""
    if name in CHANNEL_AXIS and t.shape[-1] != 2:       # (the star prior's coords are [n, 2]: their last axis is the channel)
        return torch.cat([t, t[..., :1, :]], -2)
    return torch.cat([t, t[..., :1]], -1)


# ---- the descriptor every fit / step wrapper hands the library ---------------------------------------------------------------------------
# kind, lr, beta1, beta2, eps, weight_decay, clamp | plateau .. plateau_eps | freeze_skips, freeze_input, logits_at_last_forward
B = (0.9, 0.999, 1e-8)
OPT_DESCS = {
    "fit": ((ADAM, 2e-3, *B, 0.0, 1), (0, 0, 0), True),
    "cdn_fit": ((ADAM, 3e-3, *B, 0.0, 1), (0, 0, 0), True),
    "pcn_fit": ((ADAMAX, 1e-3, *B, 0.0, 1), (0, 0, 0), True),
    "fit_identity": ((ADAMAX, 1e-2, *B, 1e-5, 0), (0, 0, 0), False),
    "pcn_fit_sequence": ((ADAMAX, 1e-3, *B, 0.0, 1), (0, 0, 0), True),
    "fit_identity_sequence": ((ADAMAX, 1e-2, *B, 1e-5, 0), (0, 0, 0), False),
    "star_fit": ((ADAM, 1e-2, *B, 0.0, 0), (0, 0, 0), False),
    "fit_minibatch": ((ADAM, 2e-3, *B, 0.0, 1), (0, 0, 0), True),
    "cdn_fit_minibatch": ((ADAM, 3e-3, *B, 0.0, 1), (0, 0, 0), True),
    "sym_fit": ((ADAM, 1e-3, *B, 0.0, 0), (1, 0, 0), True),
    "sym_fit_minibatch": ((ADAM, 1e-3, *B, 0.0, 0), (1, 0, 0), True),
    "joint_step": ((ADAM, 1e-3, *B, 0.0, 1), (0, 0, 0), False),
    "wide_joint_step": ((ADAM, 1e-3, *B, 0.0, 1), (0, 0, 0), False),
    "joint_prior_step": ((ADAM, 1e-3, *B, 0.0, 1), (0, 0, 0), False),
    "wide_joint_prior_step": ((ADAM, 1e-3, *B, 0.0, 1), (0, 0, 0), False),
    "pcn_joint_step": ((ADAM, 1e-3, *B, 0.0, 1), (0, 0, 0), False),
    "pcn_wide_joint_step": ((ADAM, 1e-3, *B, 0.0, 1), (0, 0, 0), False),
    "cdn_joint_step": ((ADAM, 1e-3, *B, 0.0, 1), (0, 0, 0), False),
}


@pytest.fixture
def recorded(monkeypatch):
    """The wrappers run on CPU tensors up to the call, which is recorded instead of made: (entry, args)."""
    calls = []
    monkeypatch.setattr(X, "on_gpu", lambda **tensors: None)
    monkeypatch.setattr(X, "workspace", lambda *a, **k: None)
    monkeypatch.setattr(X, "cached_workspace", lambda *a, **k: None)
    monkeypatch.setattr(X, "call", lambda entry, *args, **k: calls.append((entry, args)))
    return calls


def _fields(od):
    return tuple(getattr(od, name) for name, _ in L.InrOptDesc._fields_)


def _as_stored(values):
    return tuple(ctypes.c_float(v).value if isinstance(v, float) else v for v in values)


OPT_CASES = [(name, None) for name in sorted(OPT_DESCS)] + [(name, PL) for name in sorted(OPT_DESCS) if OPT_DESCS[name][2]]


@pytest.mark.parametrize("name,plateau", OPT_CASES, ids=[f"{n}-{'plateau' if p else 'defaults'}" for n, p in OPT_CASES])
def test_opt_desc_of_every_fit_and_step_wrapper(recorded, name, plateau):
    head, tail, _ = OPT_DESCS[name]      # (the third entry: whether the wrapper takes a plateau argument)
    fn, valid, _ = WRAPPERS[name]
    fn(**valid(), **({"plateau": plateau} if plateau is not None else {}))
    (entry, args), = recorded
    (od,) = [a for a in args if isinstance(a, L.InrOptDesc)]
    assert _fields(od) == _as_stored(head + (ON if plateau is not None else OFF) + tail), entry


def test_opt_desc_builder_is_the_only_constructor():
    import glob
    import os
    root = os.path.dirname(os.path.abspath(A.__file__))
    hits = [f for f in glob.glob(os.path.join(root, "**", "*.py"), recursive=True)
            if "InrOptDesc(" in open(f).read().replace("class InrOptDesc(", "") and os.path.basename(f) != "_call.py"]
    assert hits == []


# ---- the argument checks -----------------------------------------------------------------------------------------------------------------
CASES = [(name, arg) for name, (_, _, args) in sorted(WRAPPERS.items()) for arg in args]


@pytest.mark.parametrize("name,arg", CASES, ids=[f"{n}-{a}" for n, a in CASES])
def test_one_spoiled_width_is_a_value_error_naming_the_argument(name, arg):
    fn, valid, _ = WRAPPERS[name]
    kw = valid()
    kw[arg] = spoiled(arg, kw[arg])
    with pytest.raises(ValueError, match=rf"\b{arg}\b"):
        fn(**kw)
    kw = valid()
    kw[arg] = kw[arg].double()
    with pytest.raises(ValueError, match=rf"\b{arg}\b.*float32"):
        fn(**kw)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_the_valid_set_stops_at_the_device_check(name):
    """... so nothing past the checks ran: the shapes above are accepted, only the CPU is not."""
    fn, valid, _ = WRAPPERS[name]
    with pytest.raises(L.InrfitError, match="must live on the GPU"):
        fn(**valid())


def test_rows_messages_and_order():
    with pytest.raises(ValueError, match=r"flow_params: expected shape \(2, 7\), got shape \(2, 6\)"):
        X.rows(z(2, 6), "flow_params", 2, 7)
    with pytest.raises(ValueError, match=r"dout: expected shape \('n', 2, 12\), got shape \(3, 12\)"):
        X.rows(z(3, 12), "dout", None, (2, 12))
    with pytest.raises(ValueError, match="params: expected 5 floats"):
        X.flat(z(2, 3), "params", 5)
    with pytest.raises(ValueError, match="must be float32"):       # dtype before shape before device
        X.rows(z(2, 6).double(), "x", 2, 7)
    with pytest.raises(L.InrfitError, match="x must live on the GPU"):
        K._check_dev(z(3), "x")
    assert not issubclass(L.InrfitError, ValueError)


# ---- the workspace query ------------------------------------------------------------------------------------------------------------------
def test_workspace_raises_under_the_entrys_name():
    with pytest.raises(L.InrfitError, match="inrfit_workspace_bytes failed"):
        X.workspace("inrfit_workspace_bytes", A.IcnnSpec(1777, 2, 1).desc(), grid().desc(), 1, device="cpu")
    ws = X.workspace("inrfit_workspace_bytes", ISPEC.desc(), grid().desc(), 1, device="cpu")     # the query answers on the host
    d, g = ISPEC.desc(), grid().desc()
    nbytes = L.load().inrfit_workspace_bytes(ctypes.byref(d), ctypes.byref(g), 1)
    assert ws.dtype == torch.float32 and ws.numel() == nbytes // 4 + 1
    assert X.workspace("inrfit_workspace_bytes", d, g, 1, device="cpu", slack=64).numel() == nbytes // 4 + 64


def test_cached_workspace_and_poison(monkeypatch):
    monkeypatch.setattr(X, "_ws_cache", {})
    sizes = iter([400, 400, 400])
    a = X.cached_workspace("k", lambda: next(sizes), "cpu", refresh_under_poison=True)
    assert a.numel() == 100 + 64 and X.cached_workspace("k", lambda: next(sizes), "cpu", refresh_under_poison=True) is a
    monkeypatch.setattr(L, "POISON", True)
    assert X.cached_workspace("k", lambda: next(sizes), "cpu", refresh_under_poison=False) is a       # the segmentation networks keep theirs
    b = X.cached_workspace("k", lambda: next(sizes), "cpu", refresh_under_poison=True)
    assert b is not a and bool(torch.isnan(b).all())
    with pytest.raises(L.InrfitError, match="some query failed"):
        X.cached_workspace("other", lambda: -3, "cpu", refresh_under_poison=True, what="some query")


# ---- marshalling -------------------------------------------------------------------------------------------------------------------------
def test_call_marshals_and_appends_workspace_and_stream(monkeypatch):
    seen = []

    class Stub:
        def inrfit_backward(self, *args):
            seen.append(args)
            return 0

        inrfit_miou = inrfit_backward

        def inrfit_fit(self, *args):
            return -2

        def inrfit_strerror(self, rc):
            return b"stub error"

    monkeypatch.setattr(L, "load", lambda: Stub())
    monkeypatch.setattr(X, "_stream_ptr", lambda device: 4242)
    md, gd, t, dl, g, ws = ISPEC.desc(), grid().desc(), z(3), z(5), z(3), z(10)
    X.call("inrfit_backward", md, t, gd, dl, 7, g, None, ws=ws, device=None)      # (model, params, grid, dlogits, n, grads, dcoords)
    X.call("inrfit_miou", t, dl, 1, 3, 0.5, 0.5, 1, g, device=None)
    (a, b) = seen
    assert type(a[0]) is type(ctypes.byref(md)) and a[0]._obj is md and a[2]._obj is gd      # a Structure arrives by reference
    assert (a[1], a[3], a[4], a[5], a[6]) == (t.data_ptr(), dl.data_ptr(), 7, g.data_ptr(), None)   # tensors as pointers, None stays
    assert a[7:] == (ws.data_ptr(), 40, 4242)                                           # workspace, its bytes, the stream
    assert b == (t.data_ptr(), dl.data_ptr(), 1, 3, 0.5, 0.5, 1, g.data_ptr(), 4242)    # no workspace: the stream alone
    arr, sched = (ctypes.c_int32 * 2)(1, 2), (ctypes.c_double * 5)()
    got = X._marshal("inrfit_pcn_fit_sequence", (md, RSPEC.desc(), t, t, t, t, t, t, arr, 1, 12, 1, 1, X.loss_desc("se", "none", 1.0, 0.0, 0.0),
                                                 X.opt_desc("adam", 1e-3, (0.9, 0.999), 1e-8), sched, 0.0, 0, t, t))
    assert got[8] is arr and got[15] is sched and got[13]._obj.kind == L.INR_LOSS_SE   # ctypes arrays pass through
    with pytest.raises(L.InrfitError, match="inrfit_fit failed: stub error"):
        X.call("inrfit_fit", device=None)


def test_fit_outputs_and_trim():
    hist, logits, status = X.fit_outputs(2, 0, (2, 5), True, True, "cpu")
    assert tuple(hist.shape) == (2, 1) and tuple(logits.shape) == (2, 5)
    assert status.dtype == torch.int32 and status.tolist() == [0, 0]
    assert tuple(X.trim(hist, 0).shape) == (2, 0) and X.trim(None, 3) is None
    assert X.fit_outputs(2, 3, None, False, False, "cpu")[:2] == (None, None)
    assert tuple(X.trim(z(4), 3).shape) == (3,)
