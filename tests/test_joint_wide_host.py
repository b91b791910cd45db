"""The layer-by-layer joint step's host side (no GPU): the five exported symbols, the binding against the header, the ABI version,
the argument errors that must come back before anything touches a device, and JointTrainer's routing with and without
fused_layer_by_layer."""
import ctypes as C
import os
import re

import pytest
import torch

import awesome_amd as A
from awesome_amd import _lib as L
from awesome_amd import joint as J
from awesome_amd import rnvp as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["inrfit_wide_joint_step_workspace_bytes", "inrfit_pcn_wide_joint_step_workspace_bytes", "inrfit_wide_joint_step",
       "inrfit_pcn_wide_joint_step", "inrfit_wide_joint_prior_step"]
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


def _codes():
    """The error codes by name, from the header."""
    text = open(os.path.join(ROOT, "include", "inrfit.h")).read()
    return {k: int(v) for k, v in re.findall(r"(INR_E[A-Z]+)\s*=\s*(-?\d+)", text)}


def test_error_codes_are_the_headers():
    c = _codes()
    assert (c["INR_EINVAL"], c["INR_EUNSUPPORTED"], c["INR_EWORKSPACE"]) == (EINVAL, EUNSUPPORTED, EWORKSPACE)


def test_library_exports_the_five_symbols_and_abi_is_8():
    lib = L.load()
    for name in NEW:
        assert name in L.EXPORTS and getattr(lib, name) is not None
    ver = C.c_int(0)
    lib.inrfit_query(C.byref(ver), None, None)
    assert ver.value == L.INRFIT_ABI_VERSION == 8


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "inrfit.h")).read()
    m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


@pytest.mark.parametrize("new,old", [("inrfit_wide_joint_step", "inrfit_joint_step"), ("inrfit_pcn_wide_joint_step", "inrfit_pcn_joint_step"),
                                     ("inrfit_wide_joint_prior_step", "inrfit_joint_prior_step"),
                                     ("inrfit_wide_joint_step_workspace_bytes", "inrfit_joint_step_workspace_bytes")])
def test_binding_matches_the_header_and_the_fused_counterpart(new, old):
    rt_new, args_new = _header_arity(new)
    rt_old, args_old = _header_arity(old)
    assert (rt_new, args_new) == (rt_old, args_old)                       # the argument list of the fused call, unchanged
    restype, argtypes = L.EXPORTS[new]
    assert (restype, argtypes) == L.EXPORTS[old]
    assert len(argtypes) == len(args_new) and restype is (C.c_int64 if rt_new == "int64_t" else C.c_int)
    for decl, ct in zip(args_new, argtypes):                              # pointers, 64-bit sizes, floats and ints line up
        want = (C.c_int64 if decl.startswith("int64_t") else C.c_float if decl.startswith("float ") else C.c_int) if "*" not in decl else None
        assert (ct is want) if want is not None else (ct is C.c_void_p or issubclass(ct, C._Pointer)), (decl, ct)


def test_pcn_workspace_binding():
    rt, args = _header_arity("inrfit_pcn_wide_joint_step_workspace_bytes")
    restype, argtypes = L.EXPORTS["inrfit_pcn_wide_joint_step_workspace_bytes"]
    assert rt == "int64_t" and restype is C.c_int64 and len(args) == len(argtypes) == 3


WIDE = A.IcnnSpec(n_hidden=136, in_features=2, n_layers=1)
FUSED = A.IcnnSpec(n_hidden=130, in_features=2, n_layers=1)
ENCODE = A.IcnnSpec(n_hidden=64, in_features=2, n_layers=1, act0="cos", n_out=2)
FAKE = 0x1000          # a non-null "device pointer": every call below must return before anything dereferences or launches


def _grid(n=460):
    g = L.InrGridDesc(L.INR_GRID_EXPLICIT, 0, 0, n, None, None, None, FAKE, n)
    return g


def _opt(kind=L.INR_OPT_ADAM):
    return L.InrOptDesc(kind, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0, 0)


def _rnvp():
    return R.RnvpSpec(2, 16, 4, "tanh", None, (0.0, 0.0), (1.0, 1.0)).desc()


def _call(entry, spec=WIDE, grid=None, desc=None, opt=None, step=1, ws=FAKE, ws_bytes=1 << 40, ptr=FAKE, dseg=FAKE):
    lib = L.load()
    md, gd, od = spec.desc(), grid or _grid(), opt or _opt()
    if entry == "prior":
        d = desc or J.joint_prior_desc()
        return lib.inrfit_wide_joint_prior_step(C.byref(md), ptr, FAKE, C.byref(gd), FAKE, FAKE, C.byref(d), None, C.byref(od), step,
                                                None, dseg, None, None, ws, ws_bytes, None)
    d = desc or J.joint_desc()
    if entry == "pcn":
        rd = _rnvp()
        return lib.inrfit_pcn_wide_joint_step(C.byref(md), C.byref(rd), ptr, FAKE, FAKE, FAKE, C.byref(gd), FAKE, FAKE, C.byref(d),
                                              C.byref(od), 0.0, step, None, dseg, None, None, ws, ws_bytes, None)
    return lib.inrfit_wide_joint_step(C.byref(md), ptr, FAKE, C.byref(gd), FAKE, FAKE, C.byref(d), C.byref(od), step, None, dseg, None,
                                      None, ws, ws_bytes, None)


@pytest.mark.parametrize("entry", ["icnn", "pcn", "prior"])
def test_argument_errors_come_back_before_anything_is_launched(entry):
    assert _call(entry, ptr=None) == EINVAL                       # null parameters
    assert _call(entry, dseg=None) == EINVAL
    assert _call(entry, spec=FUSED) == EUNSUPPORTED               # a shape with a fused kernel
    assert _call(entry, spec=ENCODE) == EUNSUPPORTED              # an encode shape
    assert _call(entry, ws=None) == EINVAL
    assert _call(entry, ws_bytes=1024) == EWORKSPACE
    assert _call(entry, step=0) == EINVAL
    assert _call(entry, opt=_opt(kind=7)) == EINVAL
    lib, md, gd = L.load(), WIDE.desc(), _grid()
    need = (lib.inrfit_pcn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(_rnvp()), C.byref(gd)) if entry == "pcn"
            else lib.inrfit_wide_joint_step_workspace_bytes(C.byref(md), C.byref(gd)))
    assert need > 0 and _call(entry, ws_bytes=need - 1) == EWORKSPACE


def test_prior_step_argument_errors():
    assert _call("prior", desc=J.joint_prior_desc(align_rule=L.ALIGN_HARD, align_begin=460)) == EINVAL     # a bad align_begin
    assert _call("prior", desc=J.joint_prior_desc(align_rule=L.ALIGN_SOFT, align_begin=-1)) == EINVAL
    assert _call("prior", desc=J.joint_prior_desc(data_count=461)) == EINVAL
    assert _call("prior", desc=J.joint_prior_desc(align_rule=3)) == EINVAL


def test_joint_step_refuses_the_forms_the_fused_call_refuses():
    assert _call("icnn", desc=J.joint_desc(form=L.JOINT_AWESOME_PIXEL)) == EUNSUPPORTED
    assert _call("icnn", desc=J.joint_desc(form=L.JOINT_AWESOME_IMAGE, noneclass=2.0)) == EUNSUPPORTED
    assert _call("pcn", desc=J.joint_desc(form=L.JOINT_AWESOME_IMAGE, class_targets=True)) == EUNSUPPORTED


def test_workspace_calls_refuse_the_same_shapes():
    lib, gd = L.load(), _grid()
    for spec in (FUSED, ENCODE):
        md = spec.desc()
        assert lib.inrfit_wide_joint_step_workspace_bytes(C.byref(md), C.byref(gd)) == EUNSUPPORTED
        assert lib.inrfit_pcn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(_rnvp()), C.byref(gd)) == EUNSUPPORTED
    md = WIDE.desc()
    assert lib.inrfit_joint_step_workspace_bytes(C.byref(md), C.byref(gd)) > 0        # (unchanged: the plain workspace call serves it)
    assert lib.inrfit_wide_joint_step_workspace_bytes(C.byref(md), None) == EINVAL


# ---- JointTrainer's plan, without a device: _plan_fused reads the wrapper, the optimizer and the bank's device type only ------------
class _Bank:
    device = torch.device("cuda", 0)


def _plan(prior, crit, **switches):
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ForwardModule, WrapperModule
    from awesome_amd.prior_bank import _ordered_parameters
    tr = JointTrainer.__new__(JointTrainer)
    tr.wrapper = WrapperModule(ForwardModule(), prior)
    tr.bank, tr.criterion = _Bank(), crit
    tr.optimizer = torch.optim.Adam(list(_ordered_parameters(prior)), lr=1e-3)
    tr.fused_convexity_losses = switches.get("fused_convexity_losses", False)
    tr.fused_layer_by_layer = switches.get("fused_layer_by_layer", False)
    return tr._plan_fused()


def test_joint_trainer_routing_with_and_without_the_switch():
    from awesome_amd.measures import AwesomeImageLossJoint, FBMSJointLoss
    from awesome_amd.model import ConvexDiffeomorphismNet, ConvexNextNet, real_nvp_path_connected_net
    fbms = FBMSJointLoss(alpha=1.0, beta=2.0)
    wide = lambda: ConvexNextNet(n_hidden=256, in_features=2, n_hidden_layers=1)                      # noqa: E731
    deep = lambda: ConvexNextNet(n_hidden=130, in_features=2, n_hidden_layers=3)                      # noqa: E731
    pcn = lambda h: real_nvp_path_connected_net(channels=2, hidden_units=16, flow_n_flows=4, flow_output_fn="tanh",   # noqa: E731
                                                convex_net_hidden_units=h, convex_net_hidden_layers=2)
    for make in (wide, deep, lambda: pcn(256)):
        assert _plan(make(), fbms) is None                                                            # default: the autograd step
        plan = _plan(make(), fbms, fused_layer_by_layer=True)
        assert plan is not None and plan["wide"] is True
    assert _plan(wide(), fbms, fused_layer_by_layer=True)["family"] == "icnn"
    assert _plan(pcn(256), fbms, fused_layer_by_layer=True)["family"] == "pcn"
    # shapes with a fused kernel: the same plan with and without the switch, not marked
    for sw in (False, True):
        assert _plan(ConvexNextNet(n_hidden=130, in_features=2, n_hidden_layers=2), fbms, fused_layer_by_layer=sw)["wide"] is False
        assert _plan(pcn(64), fbms, fused_layer_by_layer=sw)["wide"] is False
    # ConvexDiffeomorphismNet over a layer-by-layer ICNN stays on autograd
    cdn = ConvexDiffeomorphismNet(n_hidden=144, n_hidden_layers=1, nf_layers=4, nf_hidden=24, diffeo_args=dict(backbone="normal_block"))
    assert _plan(cdn, fbms, fused_layer_by_layer=True) is None
    # the convexity route needs its own switch as well
    joint = AwesomeImageLossJoint(alpha=0.7, beta=3.0, gamma=0.2)
    assert _plan(wide(), joint, fused_layer_by_layer=True) is None
    assert _plan(wide(), joint, fused_layer_by_layer=True, fused_convexity_losses=True)["wide"] is True
    assert _plan(wide(), joint, fused_convexity_losses=True) is None


def test_run_py_reads_the_switch_and_the_config_sets_it():
    text = open(os.path.join(ROOT, "scripts", "run.py")).read()
    assert 'fused_layer_by_layer=bool(aa.get("fused_layer_by_layer", False))' in text
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "c5_refine_noisy256_wide256.yaml")))["AwesomeConfig"]
    assert cfg["agent_args"]["fused_layer_by_layer"] is True and cfg["prior_model_args"]["convex_net_hidden_units"] == 256
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "c5_refine_noisy256.yaml")))["AwesomeConfig"]
    cfg["agent_args"].pop("fused_layer_by_layer")
    cfg["prior_model_args"]["convex_net_hidden_units"] = base["prior_model_args"]["convex_net_hidden_units"]
    cfg["name_experiment"] = base["name_experiment"]
    assert cfg == base
