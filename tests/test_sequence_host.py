"""Host side of the sequence pretraining calls (inrfit_pcn_fit_sequence, inrfit_rnvp_fit_identity_sequence): where the frame orders
come from, the argument checks (all answered before any device call), the exports, the normalized (T, H, W) grid against the
reference class's values, and the config that switches both on.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import sequence_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


@pytest.mark.parametrize("T,batch", [(5, 2), (4, 1), (5, 5), (3, 7)])
def test_orders_are_the_dataloaders(T, batch):
    """Under torch.manual_seed(s) the orders equal what a real DataLoader(TensorDataset(arange(T)), batch_size, shuffle=True) yields:
    one loader iterated several epochs (the identity pre-fit), a new loader per epoch (the main loop)."""
    from awesome_amd import rnvp as R
    for one_loader in (True, False):
        torch.manual_seed(123)
        want = Q.dataloader_orders(T, batch, 4, one_loader)
        torch.manual_seed(123)
        got = R.sequence_orders(T, batch, 4, shuffle=True, one_loader=one_loader)
        assert got.dtype == torch.int64 and torch.equal(got, want)
        assert all(sorted(r) == list(range(T)) for r in got.tolist())
    assert len({tuple(r) for r in want.tolist()}) > 1 or T < 3          # (the epochs are shuffled apart)
    assert torch.equal(R.sequence_orders(T, batch, 3, shuffle=False), Q.identity_orders(3, T))
    assert R.sequence_orders(T, batch, 0).shape == (0, T)


_PCN_FAULTS = [
    (dict(ip=None), EINVAL), (dict(fp=None), EINVAL), (dict(iopt=None), EINVAL), (dict(fopt=None), EINVAL), (dict(coords=None), EINVAL),
    (dict(targets=None), EINVAL), (dict(order=None), EINVAL), (dict(opt=None), EINVAL), (dict(loss=None), EINVAL),
    (dict(epoch_loss=None), EINVAL), (dict(status=None), EINVAL), (dict(ws=None), EINVAL),
    (dict(batch=0), EINVAL), (dict(T=0), EINVAL), (dict(HW=0), EINVAL), (dict(epochs=-1), EINVAL), (dict(step0=-1), EINVAL),
    (dict(step0=1), EINVAL),                                        # a sequence fit is a cold fit
    (dict(order=[[0, 1, 2, 3, 4], [0, 1, 2, 3, 5]]), EINVAL),       # an id equal to T
    (dict(order=[[0, 1, -1, 3, 4], [0, 1, 2, 3, 4]]), EINVAL),      # a negative id
    (dict(order=[[0, 1, 2, 3, 4], [0, 1, 1, 3, 4]]), EINVAL),       # a repeated id
    (dict(ws_bytes=1024), EWORKSPACE),
]


@pytest.mark.parametrize("fault,code", _PCN_FAULTS)
def test_pcn_sequence_single_fault_codes(fault, code):
    """inrfit_pcn_fit_sequence answers an argument list with one fault on the host with the documented code (the pointers are not
    device memory: a call that got past its checks would not return a code)."""
    from awesome_amd import _lib
    assert Q.call_pcn_sequence(_lib.load(), Q.sequence_args(**fault)) == code


def test_pcn_sequence_model_faults():
    from awesome_amd import _lib as L
    lib = L.load()
    md, rd, ld, od = Q.abi_descs()
    wide = L.InrModelDesc(L.INR_MODEL_ICNN, 256, Q.CH, 1, 0, 0.0, 0, 0)       # a layer-by-layer shape
    deep = L.InrModelDesc(L.INR_MODEL_ICNN, 130, Q.CH, 3, 0, 0.0, 0, 0)
    for m in (wide, deep):
        assert lib.inrfit_supported(C.byref(m)) == 1                           # (inrfit_pcn_fit takes it; the sequence call does not)
        assert Q.call_pcn_sequence(lib, Q.sequence_args(model=C.byref(m))) == EUNSUPPORTED
        assert lib.inrfit_pcn_sequence_workspace_bytes(C.byref(m), C.byref(rd), 63, 5, 2) == EUNSUPPORTED
    assert Q.call_pcn_sequence(lib, Q.sequence_args(model=None)) == EUNSUPPORTED
    bad = L.InrRnvpDesc()
    assert Q.call_pcn_sequence(lib, Q.sequence_args(rnvp=C.byref(bad))) == EUNSUPPORTED
    bad_opt = L.InrOptDesc(7, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 0.5, 1e-4, 0.0, 1e-8, 0, 0, 0)
    assert Q.call_pcn_sequence(lib, Q.sequence_args(opt=C.byref(bad_opt))) == EINVAL
    bad_loss = L.InrLossDesc(L.INR_LOSS_EXTERNAL, L.INR_WEIGHT_NONE, 1.0, 0.0, 0.0)
    assert Q.call_pcn_sequence(lib, Q.sequence_args(loss=C.byref(bad_loss))) == EINVAL


_ID_FAULTS = [
    (dict(fp=None), EINVAL), (dict(fopt=None), EINVAL), (dict(coords=None), EINVAL), (dict(order=None), EINVAL), (dict(opt=None), EINVAL),
    (dict(epoch_loss=None), EINVAL), (dict(ws=None), EINVAL),
    (dict(batch=0), EINVAL), (dict(T=0), EINVAL), (dict(HW=0), EINVAL), (dict(epochs=-1), EINVAL), (dict(step0=-1), EINVAL),
    (dict(order=[[0, 1, 2, 3, 4], [5, 1, 2, 3, 4]]), EINVAL),
    (dict(order=[[0, 1, 2, 3, -2], [0, 1, 2, 3, 4]]), EINVAL),
    (dict(order=[[4, 4, 2, 3, 0], [0, 1, 2, 3, 4]]), EINVAL),
    (dict(ws_bytes=1024), EWORKSPACE),
]


@pytest.mark.parametrize("fault,code", _ID_FAULTS)
def test_identity_sequence_single_fault_codes(fault, code):
    from awesome_amd import _lib as L
    lib = L.load()
    assert Q.call_identity_sequence(lib, Q.sequence_args(**fault)) == code
    bad = L.InrRnvpDesc()
    assert Q.call_identity_sequence(lib, Q.sequence_args(rnvp=C.byref(bad))) == EUNSUPPORTED


def test_workspace_query():
    """The size query covers both batch shapes of an epoch (the full batches and a shorter last one) behind the staging buffers, and
    answers its own faults."""
    from awesome_amd import _lib as L
    lib = L.load()
    md, rd, _, _ = Q.abi_descs()
    q = lambda m, hw, T, b: lib.inrfit_pcn_sequence_workspace_bytes(C.byref(m) if m is not None else None, C.byref(rd), hw, T, b)  # noqa: E731
    g = L.InrGridDesc(L.INR_GRID_EXPLICIT, 0, 0, 2 * 63, None, None, None, None, 0)
    step = lib.inrfit_pcn_workspace_bytes(C.byref(md), C.byref(rd), C.byref(g), 1)
    staging = (Q.CH + 1) * 2 * 63 * 4
    assert step + staging <= q(md, 63, 5, 2) <= step + staging + 8 * 256
    assert q(md, 63, 5, 9) == q(md, 63, 5, 5)                       # a batch never holds more than T frames
    assert 0 < q(None, 63, 5, 2) < q(md, 63, 5, 2)                  # the identity pre-fit has no ICNN behind the flow
    assert q(md, 63, 5, 0) == EINVAL and q(md, 0, 5, 2) == EINVAL and q(md, 63, 0, 2) == EINVAL
    assert lib.inrfit_pcn_sequence_workspace_bytes(C.byref(md), None, 63, 5, 2) == EUNSUPPORTED


def test_exports_and_declarations():
    """The three symbols are in the header with the signatures the binding declares, the version script exports them, and the ABI
    version did not move."""
    from awesome_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "inrfit.h")).read()
    lib = L.load()
    ctype = {"const InrModelDesc*": C.POINTER(L.InrModelDesc), "const InrRnvpDesc*": C.POINTER(L.InrRnvpDesc),
             "const InrLossDesc*": C.POINTER(L.InrLossDesc), "const InrOptDesc*": C.POINTER(L.InrOptDesc),
             "const int32_t*": C.POINTER(C.c_int32), "float*": C.c_void_p, "const float*": C.c_void_p, "int32_t*": C.c_void_p,
             "void*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "const double*": C.POINTER(C.c_double), "float": C.c_float}
    for name, ret in (("inrfit_pcn_sequence_workspace_bytes", C.c_int64), ("inrfit_pcn_fit_sequence", C.c_int),
                      ("inrfit_rnvp_fit_identity_sequence", C.c_int)):
        m = re.search(r"(int64_t|int)\s+" + name + r"\(([^)]*)\);", hdr)
        assert m, name
        declared = [ctype[" ".join(a.split()[:-1])] for a in m.group(2).replace("\n", " ").split(",")]
        restype, argtypes = L.EXPORTS[name]
        assert restype is ret and ({"int64_t": C.c_int64, "int": C.c_int}[m.group(1)] is ret)
        assert argtypes == declared, name
        assert hasattr(lib, name)
    assert "global: inrfit_*;" in open(os.path.join(ROOT, "awesome_amd", "csrc", "inrfit.map")).read()
    order_arg = [a for a in re.search(r"inrfit_pcn_fit_sequence\(([^)]*)\)", hdr).group(1).split(",") if a.split()[-1] == "order"]
    assert order_arg and "const int32_t*" in order_arg[0]
    assert "#define INRFIT_ABI_VERSION 8" in hdr and L.INRFIT_ABI_VERSION == 8


def test_normalized_grid_matches_the_reference_class(golden_dir):
    """create_normalized_grid((T, H, W)) / ((H, W)) against the values the reference class produced (tools/gen_golden_sequence.py,
    tests/golden/PROVENANCE_sequence.txt)."""
    from awesome_amd.model.path_connected_net import PathConnectedNet
    ref = np.load(os.path.join(golden_dir, "normalized_grid_reference.npz"))
    for key in ref.files:
        shape = tuple(int(v) for v in key.split("_")[1:])
        got = PathConnectedNet.create_normalized_grid(shape)
        assert got.dtype == torch.float32 and tuple(got.shape) == ref[key].shape, key
        np.testing.assert_array_equal(got.numpy(), ref[key], err_msg=key)
    g = PathConnectedNet.create_normalized_grid((5, 7, 9))
    assert g.shape == (5, 3, 7, 9) and float(g.min()) == 0.0 and float(g.max()) == 1.0
    assert torch.equal(g[:, 2, 0, 0], torch.arange(5) / 4) and torch.equal(g[0, 0, 0], torch.arange(9) / 8)


def test_reference_config_switches_reach_pretrain_args():
    """config/c4_sequence128x16_reference.yaml decodes, and is c4 with batch_size 2 and both switches on."""
    from awesome_amd.run.config import AwesomeConfig
    cfg = AwesomeConfig.load_from_file(os.path.join(ROOT, "config", "c4_sequence128x16_reference.yaml"))
    base = AwesomeConfig.load_from_file(os.path.join(ROOT, "config", "c4_sequence128x16.yaml"))
    pre, pre0 = dict(cfg.agent_args["pretrain_args"]), dict(base.agent_args["pretrain_args"])
    assert pre.pop("reference_prefits") is True and pre.pop("sequence_device_loop") is True and pre.pop("batch_size") == 2
    assert pre == pre0 and "reference_prefits" not in pre0 and "sequence_device_loop" not in pre0
    assert cfg.prior_model_args == base.prior_model_args and cfg.dataset_args == base.dataset_args
    assert cfg.name_experiment == "c4_sequence128x16_reference"
    # the defaults of the module: both off
    from awesome_amd.model.path_connected_net import PathConnectedNet
    import inspect
    assert "reference_prefits=False" in inspect.getsource(PathConnectedNet.pretrain_frames)
    sig = inspect.signature(PathConnectedNet.fit_sequence).parameters
    assert sig["device_loop"].default is False and sig["orders"].default is None
    sig = inspect.signature(PathConnectedNet.learn_flow_identity).parameters
    assert sig["batch_size"].default is None and sig["device_loop"].default is False and sig["orders"].default is None


def test_oracle_loop_runs_the_odd_case():
    """The oracle's mini-batch loop itself runs T = 5 at batch size 2 (a last batch of one frame) - the case the GPU test compares
    the device loop with."""
    from oracle import inr_oracle as O
    from awesome_amd.model import real_nvp_path_connected_net
    rows, uns, coords, un_t = Q.frames("t5_7x9")
    assert coords.shape == (5, 3, 63) and un_t.shape == (5, 63) and 0 < float(un_t.mean()) < 1
    torch.manual_seed(2)
    m = real_nvp_path_connected_net(channels=3, hidden_units=32, flow_n_flows=6, flow_output_fn="tanh", convex_net_hidden_units=32,
                                    convex_net_hidden_layers=1)
    sd0 = Q.oracle_state(m.state_dict())
    masks = O.rnvp_masks(3, 6)
    pf, losses = O.fit_pcn_minibatch(sd0, rows, uns, 2, 2, masks, torch.zeros(3), torch.ones(3), lr=2e-3, plateau=dict(patience=0, factor=0.5))
    assert len(losses) == 2 and all(np.isfinite(losses)) and set(pf) == set(sd0)
    # the test-side identity loop: last batch's loss per epoch, and it moves the flow only
    x = [r.clone() for r in rows]
    sd, hist = Q.fit_flow_identity_minibatch(sd0, x, Q.shuffled_orders(2, 5, seed=1), 2, masks, torch.zeros(3), torch.ones(3))
    assert len(hist) == 2 and all(np.isfinite(hist))
    assert all(torch.equal(sd[k], sd0[k]) for k in sd0 if not k.startswith("flow_net."))
    assert any(not torch.equal(sd[k], sd0[k]) for k in sd0 if k.startswith("flow_net."))
