"""The notebooks' encode nets at their own shapes (ABI 8: n_features, n_out, no hidden layer) - what can be checked without a GPU: the
C ABI's support rules and parameter counts against the host-side spec, and the module construction against the notebook classes'
state_dicts (tests/golden/encode_notebooks.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from awesome_amd import _lib, build
    build.build(force=False, verbose=False)   # cross-compiles for gfx950 without a GPU
    return _lib.load()


def _desc(h, c, l, act0=0, omega=0.0, f=0, o=0):
    from awesome_amd import _lib
    return _lib.InrModelDesc(_lib.INR_MODEL_ICNN, h, c, l, act0, omega, f, o)


def test_abi_version_is_8(lib):
    from awesome_amd import _lib
    ver = ctypes.c_int()
    assert lib.inrfit_query(ctypes.byref(ver), None, None) == 0
    assert ver.value == 8 == _lib.INRFIT_ABI_VERSION
    assert lib.inrfit_build_info().decode().startswith("libinrfit abi 8;")


def test_notebook_shape_parameter_count(lib):
    from awesome_amd import IcnnSpec, _lib
    md = _desc(350, 2, 3, _lib.INR_ACT_COS, 0.0, 20, 3)
    # W_in [20][2] + b_in [20] | W_0 [350][20] + b_0 + S_0 [350][2] | 2 x (W_k [350][350] + b_k + S_k) | W_o [3][350] + b_o [3] + S_o [3][2]
    assert 20 * 2 + 20 + (350 * 20 + 350 + 700) + 2 * (350 * 350 + 350 + 700) + 3 * 350 + 3 + 6 == 256269
    assert lib.inrfit_param_count(ctypes.byref(md)) == 256269
    spec = IcnnSpec(350, 2, 3, act0="cos", n_features=20, n_out=3)
    assert spec.n_params == 256269 and spec.general and not spec.fused()
    assert lib.inrfit_opt_state_floats(ctypes.byref(md)) == 2 * 256269 + _lib.INR_OPT_HEADER_FLOATS
    assert lib.inrfit_supported(ctypes.byref(md)) == 1
    shapes = dict(spec.keys_shapes())
    assert shapes["input.weight"] == (20, 2) and shapes["skip.0.ln.weight"] == (350, 20) and shapes["skip.1.ln.weight"] == (350, 350)
    assert shapes["out.ln.weight"] == (3, 350) and shapes["out.ln.bias"] == (3,) and shapes["out.skp.weight"] == (3, 2)


@pytest.mark.parametrize("h,c,l,f,o", [(24, 2, 3, 20, 1), (130, 2, 1, 20, 1), (64, 3, 2, 0, 2), (200, 2, 0, 0, 1), (16, 2, 0, 7, 4)])
def test_param_count_matches_spec(lib, h, c, l, f, o):
    from awesome_amd import IcnnSpec, _lib
    spec = IcnnSpec(h, c, l, act0="sin", omega=3.0, n_features=f, n_out=o)
    md = spec.desc()
    assert lib.inrfit_param_count(ctypes.byref(md)) == spec.n_params
    assert lib.inrfit_supported(ctypes.byref(md)) == 1
    assert spec.general and not spec.fused()


def test_support_rules(lib):
    from awesome_amd import _lib
    sin, cos, relu = _lib.INR_ACT_SIN, _lib.INR_ACT_COS, _lib.INR_ACT_RELU
    # the sine notebook's direct read-out (no hidden layer) behind a periodic layer 0; never behind relu
    assert lib.inrfit_supported(ctypes.byref(_desc(16, 2, 0, sin, 31.4))) == 1
    assert lib.inrfit_supported(ctypes.byref(_desc(200, 2, 0, cos))) == 1
    assert lib.inrfit_supported(ctypes.byref(_desc(64, 2, 0))) == 0
    assert lib.inrfit_supported(ctypes.byref(_desc(64, 2, 0, relu, 0.0, 20, 1))) == 0
    # n_out: 1..4, 0 = 1;  n_features: 1..1024, 0 = n_hidden
    assert lib.inrfit_supported(ctypes.byref(_desc(64, 2, 1, relu, 0.0, 0, 4))) == 1
    assert lib.inrfit_supported(ctypes.byref(_desc(64, 2, 1, relu, 0.0, 0, 5))) == 0
    assert lib.inrfit_param_count(ctypes.byref(_desc(64, 2, 1, relu, 0.0, 0, 5))) == -1
    assert lib.inrfit_supported(ctypes.byref(_desc(64, 2, 1, relu, 0.0, 1025, 1))) == 0
    zero = _desc(130, 2, 1, relu, 0.0, 0, 0)
    assert lib.inrfit_param_count(ctypes.byref(zero)) == 17813 == lib.inrfit_param_count(ctypes.byref(_desc(130, 2, 1)))
    same = _desc(130, 2, 1, relu, 0.0, 130, 1)   # n_features = n_hidden, one output: the ICNN itself
    assert lib.inrfit_param_count(ctypes.byref(same)) == 17813


def test_general_shapes_are_refused_by_composites_and_joint_steps(lib):
    """Composite priors, joint steps and the fused-kernel measurement hook have no form of these shapes: INR_EUNSUPPORTED before
    any device is touched."""
    from awesome_amd import _lib
    gd = _lib.InrGridDesc(0, 4, 4, 16, None, None, None, None, 0)
    fd = _lib.InrFlowDesc(32, 2, 0)
    rd = _lib.InrRnvpDesc()
    ctypes.memset(ctypes.byref(rd), 0, ctypes.sizeof(rd))
    for md in (_desc(64, 2, 1, 0, 0.0, 20, 1), _desc(64, 2, 1, 0, 0.0, 0, 3), _desc(64, 2, 0, _lib.INR_ACT_SIN, 3.0)):
        assert lib.inrfit_cdn_workspace_bytes(ctypes.byref(md), ctypes.byref(fd), ctypes.byref(gd), 1) == -2
        assert lib.inrfit_pcn_workspace_bytes(ctypes.byref(md), ctypes.byref(rd), ctypes.byref(gd), 1) < 0
        buf = ctypes.create_string_buffer(64)
        assert lib.inrfit_step_only(ctypes.byref(md), buf, ctypes.byref(gd), buf, ctypes.byref(_lib.InrLossDesc()), 1, 1, buf, 64,
                                    None) == -2
        assert lib.inrfit_workspace_bytes(ctypes.byref(md), ctypes.byref(gd), 1) > 0   # ... but the layer-by-layer path takes them


def test_fourier_net_matches_the_notebook_class_construction():
    """FourierFeatureNet(d_in=2, d_features=20, n_hidden=24, n_hidden_layers=3, d_out=1, factor=30) is `ourSimpleNetwork(2, 20, 24, 1,
    30)`: the same state_dict shapes, and - built under the fixture's seed, in the notebook's creation order - the same values."""
    from awesome_amd.model import FourierFeatureNet
    z = np.load(os.path.join(ROOT, "tests", "golden", "encode_notebooks.npz"))
    import random
    random.seed(51)
    np.random.seed(51)
    torch.manual_seed(51)
    m = FourierFeatureNet(d_in=2, d_features=20, n_hidden=24, n_hidden_layers=3, d_out=1, factor=30)
    sd = m.state_dict()
    ref = {k[len("fourier.sd."):]: z[k] for k in z.files if k.startswith("fourier.sd.")}
    mine = {("fc4" + k[3:] if k.startswith("out.") else k): v for k, v in sd.items()}
    assert set(mine) == set(ref)
    for k, v in ref.items():
        assert tuple(mine[k].shape) == v.shape, k
        np.testing.assert_array_equal(mine[k].numpy(), v, err_msg=k)
    assert tuple(sd["A"].shape) == (2, 20) and tuple(sd["fc1.weight"].shape) == (24, 20) and tuple(sd["out.weight"].shape) == (1, 24)
    # the loader maps the notebook's head onto `out`; the flat vector follows the general layout
    m2 = FourierFeatureNet(d_in=2, d_features=20, n_hidden=24, n_hidden_layers=3, d_out=1, factor=30)
    m2.load_notebook_state_dict({k: torch.from_numpy(v) for k, v in ref.items()})
    assert torch.equal(m2.out.weight, torch.from_numpy(ref["fc4.weight"]))
    assert m2.flat_parameters().numel() == m2.spec.n_params == 20 * 2 + 20 + (24 * 20 + 24 + 48) + 2 * (24 * 24 + 24 + 48) + 24 + 1 + 2


def test_notebook_shape_modules_and_prior_refusal():
    from awesome_amd.model import FourierFeatureNet, SineLayerNet
    m = FourierFeatureNet(d_in=2, d_features=20, n_hidden=350, n_hidden_layers=3, d_out=3, factor=30)
    assert m.spec.n_params == 256269 and tuple(m.out.weight.shape) == (3, 350)
    assert m.flat_parameters().numel() == 256269
    with pytest.raises(ValueError):
        m.pretrain(None, None, "cpu", None, wrapper_module=torch.nn.Identity())
    # the defaults keep today's spec (and with it the fused kernels)
    d = FourierFeatureNet(n_hidden=130, n_hidden_layers=1)
    assert d.spec.n_features == 0 and d.spec.n_out == 1 and not d.spec.general
    s = SineLayerNet(in_features=2, n_hidden=16, n_hidden_layers=0)
    assert s.spec.n_layers == 0 and s.spec.general and tuple(s.out.weight.shape) == (1, 16)
    z = np.load(os.path.join(ROOT, "tests", "golden", "encode_notebooks.npz"))
    sd = {k[len("sine.sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sine.sd.")}
    s.load_notebook_state_dict(sd)
    assert torch.equal(s.out.weight, sd["W2.weight"]) and torch.equal(s.W1.weight, sd["W1.weight"])
    flat = s.flat_parameters()
    assert flat.numel() == s.spec.n_params == 16 * 2 + 16 + 16 + 1 + 2
