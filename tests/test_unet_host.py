"""The UNet backbone on the host (no GPU): awesome_amd.model.UNet against the reference class's fixture (tools/gen_golden_unet.py ->
tests/golden/unet_eval.npz: keys, shapes, per-tensor sums, the evaluation-mode output), the scaled widths, the config's type name in
both directions, and the argument checks of the inrfit_unet_* entry points (they answer before anything touches a device)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "unet_eval.npz"))


def _mirror(fx):
    import gen_golden_unet as G
    from awesome_amd.model import UNet
    seed = int(fx["seed"])
    torch.manual_seed(seed)
    net = UNet(in_chn=4)
    G.perturb_batchnorm_(net, seed + 1)
    return net.eval()


def test_seeded_mirror_has_the_reference_state_dict(golden_dir):
    fx = _fixture(golden_dir)
    sd = _mirror(fx).state_dict()
    assert list(sd) == [str(k) for k in fx["keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in fx["shapes"]]
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    sumsq = np.array([float((v.double() ** 2).sum()) for v in sd.values()])
    np.testing.assert_allclose(sums, fx["sums"], rtol=1e-12, atol=1e-12)      # float64 sums of the same fp32 values
    np.testing.assert_allclose(sumsq, fx["sumsq"], rtol=1e-12, atol=1e-12)
    for name in ("inc.conv.conv.0.weight", "down4.mpconv.1.conv.4.running_var", "up1.conv.conv.3.bias", "outc.conv.weight"):
        assert name in sd


def test_torch_forward_reproduces_the_reference_output(golden_dir):
    import gen_golden_unet as G
    fx = _fixture(golden_dir)
    net = _mirror(fx)
    image, feat = G.make_inputs(int(fx["seed"]) + 2)
    np.testing.assert_array_equal(image.numpy(), fx["image"])
    np.testing.assert_array_equal(feat.numpy(), fx["feat"])
    with torch.no_grad():
        out = net(image, feat)
        out3 = net(image[0], feat[0])                      # batcherized: a single item gets its batch dimension
    assert out.shape == (1, 1, 17, 31) and out3.shape == (1, 1, 17, 31)
    ref = fx["out32"]
    assert np.abs(out.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    assert torch.equal(out, out3)
    assert np.abs(fx["out64"] - ref).max() <= 1e-4 * np.abs(ref).max()   # the two recorded outputs belong together


def test_base_width_scales_every_layer():
    from awesome_amd.model import UNet
    net = UNet(in_chn=4, out_chn=3, base_width=8)
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    assert [(m.in_channels, m.out_channels) for m in convs] == [
        (4, 8), (8, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 64), (64, 64),
        (128, 32), (32, 32), (64, 16), (16, 16), (32, 8), (8, 8), (16, 8), (8, 8), (8, 3)]
    assert list(net.state_dict()) == list(UNet(in_chn=4).state_dict())
    with torch.no_grad():
        assert net.eval()(torch.rand(2, 3, 17, 31), torch.rand(2, 1, 17, 31)).shape == (2, 3, 17, 31)
    out = net.train()(torch.rand(2, 3, 16, 16), torch.rand(2, 1, 16, 16))     # training stays plain torch, autograd attached
    assert out.grad_fn is not None


def test_config_names_the_unet_in_both_directions(tmp_path):
    import yaml
    from awesome_amd import serialization as S
    from awesome_amd.model import UNet
    from awesome_amd.run.config import AwesomeConfig
    cfg = AwesomeConfig(segmentation_model_type="awesome.model.unet.UNet", segmentation_model_args=dict(in_chn=4),
                        segmentation_training_mode="none")
    assert S.resolve_type(cfg.segmentation_model_type, "segmentation_model_type") is UNet
    assert S.dynamic_import("awesome.model.unet.UNet") is UNet
    assert S.reference_class_name(UNet) == "awesome.model.unet.UNet"
    path = cfg.save_to_file(str(tmp_path / "unet.yaml"))
    assert yaml.safe_load(open(path))["AwesomeConfig"]["segmentation_model_type"] == "awesome.model.unet.UNet"
    back = AwesomeConfig.load_from_file(path)
    assert back.segmentation_model_type == "awesome.model.unet.UNet" and back.segmentation_model_args == dict(in_chn=4)
    cfg2 = AwesomeConfig(segmentation_model_type=UNet)     # a type object is written under the reference's name, too
    assert cfg2.to_tagged_dict()["AwesomeConfig"]["segmentation_model_type"]["value"] == "awesome.model.unet.UNet"
    net = S.resolve_type(back.segmentation_model_type)(**back.segmentation_model_args)
    assert isinstance(net, UNet) and net.base_width == 64


def test_run_py_keeps_the_checkpoint_path_for_the_configs_own_backbone_only(tmp_path):
    import importlib.util
    from awesome_amd.run.config import AwesomeConfig
    spec = importlib.util.spec_from_file_location("_run_script_unet", os.path.join(ROOT, "scripts", "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    assert run.ALIASES["awesome.model.unet.UNet"] == "awesome_amd.model.UNet"
    path = AwesomeConfig(segmentation_model_type="awesome.model.unet.UNet", segmentation_model_args=dict(in_chn=4),
                         segmentation_model_state_dict_path="./data/checkpoints/unet.pth").save_to_file(str(tmp_path / "unet.yaml"))
    cfg = run.get_config(["--config-path", path])
    assert cfg.segmentation_model_state_dict_path == "./data/checkpoints/unet.pth"
    assert run.dynamic_import(cfg.segmentation_model_type).__name__ == "UNet"
    cfg = run.get_config(["--config-path", path, "--segmentation-model-type", "awesome_amd.model.ConvSegStandIn"])
    assert cfg.segmentation_model_state_dict_path is None          # a replaced backbone does not get the UNet's checkpoint


# ---- the C ABI, checked on the host -----------------------------------------------------------------------------------------------
_EINVAL, _EUNSUPPORTED, _EWORKSPACE = -1, -2, -3
_P = 0x10000      # a 16-byte aligned non-null pointer that is never dereferenced: every fault below is answered before a launch


def _args(**over):
    from awesome_amd import _lib as L
    a = dict(in_chn=4, out_chn=1, base_width=8, height=32, width=32, strip_points=0, bn_eps=1e-5, desc_null=False,
             conv_w=[_P] * 19, conv_b=[_P] * 19, gamma=[_P] * 18, beta=[_P] * 18, mean=[_P] * 18, var=[_P] * 18,
             packed=_P, input=_P, logits=_P, ws=_P, wsb=1 << 40)
    a.update(over)
    d = L.InrUNetDesc(a["in_chn"], a["out_chn"], a["base_width"], a["height"], a["width"], a["strip_points"], a["bn_eps"])
    a["desc"] = None if a["desc_null"] else C.byref(d)
    a["_keep"] = d
    for k in ("conv_w", "conv_b", "gamma", "beta", "mean", "var"):
        if a[k] is not None:
            arr = (C.c_void_p * len(a[k]))(*a[k])
            a[k] = C.cast(arr, C.c_void_p)
            a["_keep_" + k] = arr
    return a


_ENTRY = {
    "workspace_bytes": lambda lib, a: lib.inrfit_unet_workspace_bytes(a["desc"]),
    "packed_floats": lambda lib, a: lib.inrfit_unet_packed_floats(a["desc"]),
    "pack": lambda lib, a: lib.inrfit_unet_pack(a["desc"], a["conv_w"], a["conv_b"], a["gamma"], a["beta"], a["mean"], a["var"],
                                                a["packed"], None),
    "forward": lambda lib, a: lib.inrfit_unet_forward(a["desc"], a["packed"], a["input"], a["logits"], a["ws"], a["wsb"], None),
}

_FAULTS = [
    ("workspace_bytes", dict(desc_null=True), _EINVAL),
    ("workspace_bytes", dict(height=15), _EINVAL),
    ("workspace_bytes", dict(width=8), _EINVAL),
    ("workspace_bytes", dict(in_chn=0), _EINVAL),
    ("workspace_bytes", dict(out_chn=0), _EINVAL),
    ("workspace_bytes", dict(base_width=0), _EINVAL),
    ("workspace_bytes", dict(base_width=10), _EUNSUPPORTED),
    ("workspace_bytes", dict(base_width=68), _EUNSUPPORTED),
    ("workspace_bytes", dict(out_chn=9), _EUNSUPPORTED),
    ("packed_floats", dict(base_width=6), _EUNSUPPORTED),
    ("pack", dict(desc_null=True), _EINVAL),
    ("pack", dict(conv_w=None), _EINVAL),
    ("pack", dict(conv_b=[_P] * 18 + [None]), _EINVAL),
    ("pack", dict(var=None), _EINVAL),
    ("pack", dict(mean=[_P] * 7 + [None] + [_P] * 10), _EINVAL),
    ("pack", dict(packed=None), _EINVAL),
    ("pack", dict(in_chn=-1), _EINVAL),
    ("pack", dict(base_width=12, out_chn=9), _EUNSUPPORTED),
    ("pack", dict(base_width=128), _EUNSUPPORTED),
    ("forward", dict(desc_null=True), _EINVAL),
    ("forward", dict(packed=None), _EINVAL),
    ("forward", dict(input=None), _EINVAL),
    ("forward", dict(logits=None), _EINVAL),
    ("forward", dict(ws=None), _EINVAL),
    ("forward", dict(height=15), _EINVAL),
    ("forward", dict(width=15, wsb=16), _EINVAL),                # the size is checked before the workspace
    ("forward", dict(base_width=2), _EUNSUPPORTED),
    ("forward", dict(base_width=2, wsb=16), _EUNSUPPORTED),
    ("forward", dict(out_chn=16), _EUNSUPPORTED),
    ("forward", dict(wsb=16), _EWORKSPACE),
    ("forward", dict(base_width=64, height=64, width=48, wsb=1 << 20), _EWORKSPACE),
]


@pytest.mark.parametrize("entry,fault,code", _FAULTS, ids=[f"{i}-{e}-{'-'.join(f)}" for i, (e, f, _) in enumerate(_FAULTS)])
def test_single_fault_codes(entry, fault, code):
    """Every inrfit_unet_* entry point answers an input with one fault on the host, with the documented code."""
    from awesome_amd import _lib
    lib = _lib.load()
    assert _ENTRY[entry](lib, _args(**fault)) == code


def test_sizes_follow_the_layout():
    """Kp = 9 C_in + 1 rounded up to 16 per convolution; the workspace grows with the image and exactly covers what a larger strip
    needs (the strip bounds Col, not the maps)."""
    from awesome_amd import _lib as L
    lib = L.load()

    def kp(cin):
        return (9 * cin + 1 + 15) // 16 * 16

    def packed(b, cin, oc):
        down, up = [b, 2 * b, 4 * b, 8 * b, 8 * b], [4 * b, 2 * b, b, b]
        n = b * kp(cin) + b * kp(b)
        for l in range(1, 5):
            n += down[l] * kp(down[l - 1]) + down[l] * kp(down[l])
        deep = down[4]
        for u in range(4):
            n += up[u] * kp(down[3 - u] + deep) + up[u] * kp(up[u])
            deep = up[u]
        return n + oc * ((b + 1 + 15) // 16 * 16)
    for b, cin, oc in ((8, 4, 1), (64, 4, 1), (12, 3, 3)):
        d = L.InrUNetDesc(cin, oc, b, 32, 32, 0, 1e-5)
        assert lib.inrfit_unet_packed_floats(C.byref(d)) == packed(b, cin, oc)
        d2 = L.InrUNetDesc(cin, oc, b, 480, 640, 0, 1e-5)
        assert lib.inrfit_unet_packed_floats(C.byref(d2)) == packed(b, cin, oc)     # independent of the image
        small, large = lib.inrfit_unet_workspace_bytes(C.byref(d)), lib.inrfit_unet_workspace_bytes(C.byref(d2))
        assert 0 < small < large and small % 256 == 0 and large % 256 == 0
    d = L.InrUNetDesc(4, 1, 64, 480, 640, 0, 1e-5)
    d512 = L.InrUNetDesc(4, 1, 64, 480, 640, 512, 1e-5)
    assert lib.inrfit_unet_workspace_bytes(C.byref(d512)) < lib.inrfit_unet_workspace_bytes(C.byref(d))
    # Col of the widest layer stays in the tens of MB: the whole workspace minus the maps (2 per level) is below 128 MB
    hw = [480 * 640, 240 * 320, 120 * 160, 60 * 80, 30 * 40]
    maps = sum(2 * c * p * 4 for c, p in zip([64, 128, 256, 512, 512], hw))
    assert 0 < lib.inrfit_unet_workspace_bytes(C.byref(d)) - maps < 128 << 20


def test_binding_lists_the_unet_entry_points():
    from awesome_amd import _lib
    for name in ("inrfit_unet_packed_floats", "inrfit_unet_workspace_bytes", "inrfit_unet_pack", "inrfit_unet_forward"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    header = open(os.path.join(ROOT, "include", "inrfit.h")).read()
    for f in ("in_chn", "out_chn", "base_width", "height", "width", "strip_points", "bn_eps"):
        assert f in header.split("typedef struct InrUNetDesc")[1].split("InrUNetDesc;")[0]
    assert [n for n, _ in _lib.InrUNetDesc._fields_] == ["in_chn", "out_chn", "base_width", "height", "width", "strip_points", "bn_eps"]
