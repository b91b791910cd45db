"""ConvexDiffeomorphismNet over a layer-by-layer ICNN, the host side (no GPU): JointTrainer's routing with one, both and only the second
switch, run.py's reading of the switches, the new config against its fused twin, the new symbols in header, map and binding, and the
workspace queries (host computations)."""
import ctypes as C
import fnmatch
import os
import re

import pytest
import torch

import awesome_amd as A
from awesome_amd import _lib as L
from awesome_amd import flow as FL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["inrfit_cdn_wide_joint_step", "inrfit_cdn_wide_joint_step_workspace_bytes", "inrfit_cdn_wide_fit_minibatch",
       "inrfit_cdn_wide_minibatch_workspace_bytes"]
EINVAL, EUNSUPPORTED = -1, -2


class _Bank:
    device = torch.device("cuda", 0)


def _cdn(h=144, layers=1, backbone="normal_block"):
    from awesome_amd.model import ConvexDiffeomorphismNet
    return ConvexDiffeomorphismNet(n_hidden=h, n_hidden_layers=layers, nf_layers=4, nf_hidden=24, diffeo_args=dict(backbone=backbone))


def _plan(prior, crit, **switches):
    """JointTrainer._plan_fused without a device (tests/test_joint_wide_host.py::_plan, with the second switch)."""
    from awesome_amd.agent import JointTrainer
    from awesome_amd.model import ForwardModule, WrapperModule
    from awesome_amd.prior_bank import _ordered_parameters
    tr = JointTrainer.__new__(JointTrainer)
    tr.wrapper = WrapperModule(ForwardModule(), prior)
    tr.bank, tr.criterion = _Bank(), crit
    tr.optimizer = switches.pop("optimizer", torch.optim.Adam)(list(_ordered_parameters(prior)), lr=1e-3)
    tr.fused_convexity_losses = False
    tr.fused_layer_by_layer = switches.get("fused_layer_by_layer", False)
    tr.fused_cdn_layer_by_layer = switches.get("fused_cdn_layer_by_layer", False)
    return tr._plan_fused()


def test_plan_with_one_switch_both_switches_and_only_the_second():
    from awesome_amd.agent import JointTrainer
    from awesome_amd.measures import FBMSJointLoss
    fbms = FBMSJointLoss(alpha=1.0, beta=2.0)
    for h, layers in ((144, 1), (64, 3)):
        assert _plan(_cdn(h, layers), fbms) is None
        assert _plan(_cdn(h, layers), fbms, fused_layer_by_layer=True) is None                 # the first switch alone: autograd, as before
        plan = _plan(_cdn(h, layers), fbms, fused_layer_by_layer=True, fused_cdn_layer_by_layer=True)
        assert plan is not None and plan["family"] == "cdn" and plan["wide"] is True
    both = dict(fused_layer_by_layer=True, fused_cdn_layer_by_layer=True)
    assert _plan(_cdn(), fbms, optimizer=torch.optim.Adamax, **both) is None                   # the flow's step is Adam's only
    assert _plan(_cdn(backbone="resnet"), fbms, **both) is None                                # no composite at all
    for sw in ({}, both):                                                                      # a fused shape: the same plan either way
        plan = _plan(_cdn(64, 2), fbms, **sw)
        assert plan["family"] == "cdn" and plan["wide"] is False
    with pytest.raises(ValueError, match="needs fused_layer_by_layer=True"):
        JointTrainer(None, _Bank(), fbms, None, fused_cdn_layer_by_layer=True)


def test_module_routes():
    """_generic() is the 'resnet' backbone's alone; a layer-by-layer ICNN answers _specs and packs bank rows in the C ABI's order."""
    from awesome_amd.prior_bank import _ordered_parameters
    wide, res = _cdn(), _cdn(backbone="resnet")
    assert not wide._generic() and res._generic()
    assert wide._generic_pretrain() and wide._engine_name() == "generic"                       # pretrain's default: the generic loop
    wide._device_fit_layer_by_layer = True
    assert not wide._generic_pretrain() and wide._engine_name() == "device"
    ispec, fspec = wide._specs()
    assert not ispec.fused() and (ispec.n_hidden, fspec.width, fspec.num_coupling) == (144, 24, 4)
    ps = _ordered_parameters(wide)
    assert sum(p.numel() for p in ps) == ispec.n_params + fspec.n_params == sum(p.numel() for p in wide.parameters())
    flat = wide._engine_pack(wide.state_dict())
    assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for p in ps]))
    back = wide._engine_unpack(flat)
    assert all(torch.equal(back[k].reshape(v.shape), v) for k, v in wide.state_dict().items())


def test_run_py_reads_both_switches_and_the_config_sets_them():
    text = open(os.path.join(ROOT, "scripts", "run.py")).read()
    assert 'fused_layer_by_layer=bool(aa.get("fused_layer_by_layer", False))' in text
    assert 'fused_cdn_layer_by_layer=bool(aa.get("fused_cdn_layer_by_layer", False))' in text
    import inspect
    from awesome_amd.model import ConvexDiffeomorphismNet
    assert "device_fit_layer_by_layer" in inspect.signature(ConvexDiffeomorphismNet.pretrain).parameters   # pretrain_args reach it as kwargs
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "c2_blob256_cdn_wide256.yaml")))["AwesomeConfig"]
    aa = cfg["agent_args"]
    assert aa["fused_layer_by_layer"] is True and aa["fused_cdn_layer_by_layer"] is True and aa["joint_epochs"] == 1
    assert aa["pretrain_args"]["device_fit_layer_by_layer"] is True and aa["pretrain_args"]["lr"] == 0.003
    assert cfg["prior_model_args"]["n_hidden"] == 256 and cfg["optimizer_type"] == "torch.optim.Adam"
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "c2_blob256_cdn.yaml")))["AwesomeConfig"]
    aa.pop("fused_layer_by_layer")
    aa.pop("fused_cdn_layer_by_layer")
    aa["pretrain_args"].pop("device_fit_layer_by_layer")
    cfg["prior_model_args"]["n_hidden"] = base["prior_model_args"]["n_hidden"]
    cfg["name_experiment"] = base["name_experiment"]
    assert cfg == base


def test_the_config_decodes():
    from awesome_amd.run.config import AwesomeConfig
    from awesome_amd.measures import SE, FBMSJointLoss, UnariesConversionLoss
    from awesome_amd.model import ConvexDiffeomorphismNet
    cfg = AwesomeConfig.load_from_file(os.path.join(ROOT, "config", "c2_blob256_cdn_wide256.yaml"))
    pre = cfg.pretrain_args()
    assert isinstance(pre["criterion"], UnariesConversionLoss) and isinstance(pre["criterion"].criterion, SE)
    assert pre["device_fit_layer_by_layer"] is True and isinstance(cfg.build_loss(), FBMSJointLoss)
    mt = cfg.prior_model_factory()
    assert mt is ConvexDiffeomorphismNet
    assert not mt(**cfg.prior_model_args)._specs()[0].fused()


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "inrfit.h")).read()
    m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def test_new_symbols_in_header_map_and_binding():
    lib = L.load()
    text = open(os.path.join(ROOT, "awesome_amd", "csrc", "inrfit.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", text)
    for name in NEW:
        assert name in L.EXPORTS and getattr(lib, name) is not None
        assert any(fnmatch.fnmatch(name, p.strip()) for p in patterns), name
    ver = C.c_int(0)
    lib.inrfit_query(C.byref(ver), None, None)
    assert ver.value == L.INRFIT_ABI_VERSION == 8
    # each new call has the argument list of its fused counterpart, in the header and in the binding
    for new, old in (("inrfit_cdn_wide_joint_step", "inrfit_cdn_joint_step"), ("inrfit_cdn_wide_fit_minibatch", "inrfit_cdn_fit_minibatch"),
                     ("inrfit_cdn_wide_minibatch_workspace_bytes", "inrfit_minibatch_workspace_bytes"),
                     ("inrfit_cdn_wide_joint_step_workspace_bytes", "inrfit_pcn_wide_joint_step_workspace_bytes")):
        rt_new, args_new = _header_arity(new)
        rt_old, args_old = _header_arity(old)
        assert rt_new == rt_old and [a.replace("InrRnvpDesc* rnvp", "InrFlowDesc* flow") for a in args_old] == args_new
        restype, argtypes = L.EXPORTS[new]
        assert restype is L.EXPORTS[old][0] and len(argtypes) == len(args_new)
        for decl, ct in zip(args_new, argtypes):
            want = (C.c_int64 if decl.startswith("int64_t") else C.c_float if decl.startswith("float ") else C.c_int) if "*" not in decl else None
            assert (ct is want) if want is not None else (ct is C.c_void_p or issubclass(ct, C._Pointer)), (decl, ct)


WIDE, DEEP, FUSED = A.IcnnSpec(144, 2, 1), A.IcnnSpec(64, 2, 3), A.IcnnSpec(130, 2, 1)
ENCODE = A.IcnnSpec(n_hidden=64, in_features=2, n_layers=1, act0="cos", n_out=2)


def _grid(n):
    return L.InrGridDesc(L.INR_GRID_EXPLICIT, 0, 0, n, None, None, None, 0x1000, n)


def test_workspace_queries():
    """inrfit_cdn_workspace_bytes answers for the layer-by-layer shapes, grows with n_points and n_images and holds the flow's own
    buffers; the joint step's query adds to it; the shapes the flow does not take keep their answers."""
    lib = L.load()
    fd = FL.FlowSpec(24, 4).desc()
    for spec in (WIDE, DEEP):
        md = spec.desc()
        sizes = [lib.inrfit_cdn_workspace_bytes(C.byref(md), C.byref(fd), C.byref(_grid(n)), 1) for n in (1, 63, 64, 437, 480, 4096, 65536)]
        assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        g = _grid(437)
        own = lib.inrfit_cdn_workspace_bytes(None, C.byref(fd), C.byref(g), 1)
        one = lib.inrfit_cdn_workspace_bytes(C.byref(md), C.byref(fd), C.byref(g), 1)
        assert 0 < own < one < lib.inrfit_cdn_workspace_bytes(C.byref(md), C.byref(fd), C.byref(g), 3)
        assert lib.inrfit_cdn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(fd), C.byref(g)) > one
        assert lib.inrfit_cdn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(fd), None) == EINVAL
        mb = [lib.inrfit_cdn_wide_minibatch_workspace_bytes(C.byref(md), C.byref(fd), b, 1) for b in (1, 100, 300)]
        assert 0 < mb[0] <= mb[1] <= mb[2]
        assert lib.inrfit_minibatch_workspace_bytes(C.byref(md), C.byref(fd), 100, 1) == EUNSUPPORTED      # the fused shapes' call
    g = _grid(437)
    for spec in (A.IcnnSpec(1777, 2, 1), A.IcnnSpec(144, 3, 1), ENCODE):
        md = spec.desc()
        assert lib.inrfit_cdn_workspace_bytes(C.byref(md), C.byref(fd), C.byref(g), 1) == EUNSUPPORTED
        assert lib.inrfit_cdn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(fd), C.byref(g)) == EUNSUPPORTED
        assert lib.inrfit_cdn_wide_minibatch_workspace_bytes(C.byref(md), C.byref(fd), 100, 1) == EUNSUPPORTED
    md = FUSED.desc()
    assert lib.inrfit_cdn_workspace_bytes(C.byref(md), C.byref(fd), C.byref(g), 1) > 0
    assert lib.inrfit_cdn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(fd), C.byref(g)) == EUNSUPPORTED
    assert lib.inrfit_cdn_wide_minibatch_workspace_bytes(C.byref(md), C.byref(fd), 100, 1) == EUNSUPPORTED
    bad = FL.FlowSpec(24, 3).desc()
    md = WIDE.desc()
    assert lib.inrfit_cdn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(bad), C.byref(g)) == EUNSUPPORTED


def test_argument_errors_come_back_before_anything_is_launched():
    """The joint step and the minibatch fit over a layer-by-layer shape: every refusal with fake pointers, in the fused calls' order."""
    from awesome_amd import joint as J
    lib = L.load()
    FAKE = 0x1000
    fd, gd, desc = FL.FlowSpec(24, 4).desc(), _grid(437), J.joint_desc()

    def opt(kind=L.INR_OPT_ADAM):
        return L.InrOptDesc(kind, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0, 0)

    def joint(spec=WIDE, od=None, ptr=FAKE, dseg=FAKE, ws=FAKE, wsb=1 << 40, step=1, fdesc=fd, d=desc):
        md, od = spec.desc(), od or opt()
        return lib.inrfit_cdn_wide_joint_step(C.byref(md), C.byref(fdesc), ptr, FAKE, FAKE, FAKE, C.byref(gd), FAKE, FAKE, C.byref(d),
                                              C.byref(od), 0.0, step, None, dseg, None, None, ws, wsb, None)

    assert joint(ptr=None) == EINVAL and joint(dseg=None) == EINVAL
    assert joint(od=opt(L.INR_OPT_ADAMAX)) == EINVAL
    assert joint(spec=FUSED, od=opt(L.INR_OPT_ADAMAX)) == EINVAL               # the Adam-only check comes before the model check
    assert joint(spec=FUSED) == EUNSUPPORTED and joint(spec=ENCODE) == EUNSUPPORTED
    assert joint(spec=A.IcnnSpec(144, 3, 1)) == EUNSUPPORTED and joint(fdesc=FL.FlowSpec(24, 3).desc()) == EUNSUPPORTED
    assert joint(ws=None) == EINVAL and joint(wsb=1024) == -3 and joint(step=0) == EINVAL
    assert joint(d=J.joint_desc(form=L.JOINT_AWESOME_PIXEL)) == EUNSUPPORTED
    md = WIDE.desc()
    need = lib.inrfit_cdn_wide_joint_step_workspace_bytes(C.byref(md), C.byref(fd), C.byref(gd))
    assert need > 0 and joint(wsb=need - 1) == -3

    ld = L.InrLossDesc(L.LOSS_KINDS["bce"], L.WEIGHT_MODES["none"], 1.0, 0.0, 0.0)

    def mb(spec=WIDE, od=None, ptr=FAKE, ws=FAKE, wsb=16, batch=64, fdesc=fd):
        md, od = spec.desc(), od or opt()
        return lib.inrfit_cdn_wide_fit_minibatch(C.byref(md), C.byref(fdesc), ptr, FAKE, FAKE, FAKE, FAKE, FAKE, 500, FAKE, None, batch,
                                                 C.byref(ld), C.byref(od), 0.0, 1, 3, 0, None, None, ws, wsb, None)

    assert mb(ptr=None) == EINVAL and mb(batch=0) == EINVAL and mb(od=opt(L.INR_OPT_ADAMAX)) == EINVAL
    assert mb(spec=FUSED) == EUNSUPPORTED and mb(spec=ENCODE) == EUNSUPPORTED and mb(fdesc=FL.FlowSpec(24, 3).desc()) == EUNSUPPORTED
    assert mb(ws=None) == EINVAL and mb() == -3
