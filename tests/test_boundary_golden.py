"""Host-side mirrors of the reference's boundary classes against fixtures dumped from the REAL classes
(tools/gen_golden_boundary.py): PriorCache layout, PriorManager swap, FBMSJointLoss (both clip branches), the centre-of-mass
translate of ConvexDiffeomorphismNet, and the oracle's restatement of the same pieces.  CPU only (no kernel runs here)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import inr_oracle as O  # checker only


def _z(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def test_prior_cache_state_layout_matches_reference(golden_dir):
    from awesome_amd.dataset.prior_dataset import PriorManager
    from awesome_amd.model import ConvexNextNet
    from awesome_amd.util.prior_cache import PriorCache
    z = _z(golden_dir, "prior_cache_state.npz")
    model_args = dict(n_hidden=16, in_features=2, n_hidden_layers=1)
    torch.manual_seed(41)   # gen_prior_cache seeds the same way (seed_all(41)); numpy / random are not consumed
    cache = PriorCache(ConvexNextNet, model_args)
    model = ConvexNextNet(**model_args)
    s3, s7 = cache[3], cache[7]
    with PriorManager(model, prior_state=(3, s3), prior_cache=cache, model_device=torch.device("cpu")):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.25)
    st = cache.get_state()
    assert set(st) == {"model_type", "model_args", "store_device", "cache"}
    assert st["model_args"] == str(z["model_args"])                     # same JSON text (indent 4)
    assert st["store_device"] == str(z["store_device"])
    assert str(z["model_type"]).rsplit(".", 1)[-1] == st["model_type"].rsplit(".", 1)[-1] == "ConvexNextNet"
    assert sorted(st["cache"].keys()) == json.loads(str(z["cache_keys"]))
    assert list(st["cache"]["3"].keys()) == json.loads(str(z["state_keys"]))
    # same seeded construction order -> the very same generated priors, and the swap stored the modified state under key 3
    for k in ("3", "7"):
        for n, v in st["cache"][k].items():
            np.testing.assert_array_equal(v.numpy(), z[f"cache.{k}.{n}"], err_msg=f"{k}.{n}")
            assert v.dtype == torch.float32 and v.device.type == "cpu"
    # round trip
    c2 = PriorCache(None, None)
    c2.set_state(st)
    assert c2.model_args == model_args and sorted(c2.keys()) == [3, 7]
    assert torch.equal(c2[3]["input.weight"], st["cache"]["3"]["input.weight"])


def test_reference_prior_cache_file_roundtrip(tmp_path, golden_dir):
    """A cache written here loads through the reference's `PriorCache.load` recipe (torch.load + set_state): plain dict of CPU
    tensors, string keys, dotted model_type, JSON model_args."""
    from awesome_amd.model import ConvexNextNet
    from awesome_amd.util.prior_cache import PriorCache, dynamic_import
    cache = PriorCache(ConvexNextNet, dict(n_hidden=16))
    cache[5] = ConvexNextNet(n_hidden=16).state_dict()
    f = tmp_path / "prior_cache_epoch_0.pth"
    cache.save(str(f))
    raw = torch.load(str(f), weights_only=False)
    assert isinstance(raw["model_args"], str) and json.loads(raw["model_args"]) == {"n_hidden": 16}
    assert dynamic_import(raw["model_type"]) is ConvexNextNet
    back = PriorCache.load(str(f))
    assert list(back.keys()) == [5] and back.model_type is ConvexNextNet


def test_fbms_joint_loss_matches_reference(golden_dir):
    from awesome_amd.measures import FBMSJointLoss
    z = _z(golden_dir, "fbms_joint_loss.npz")
    branches = []
    for case in range(3):
        out = torch.from_numpy(z[f"c{case}.output"]).requires_grad_(True)
        tgt = torch.from_numpy(z[f"c{case}.target"])
        crit = FBMSJointLoss(criterion=torch.nn.BCELoss(), alpha=1.0, beta=float(z[f"c{case}.beta"]))
        loss = crit(out, tgt)
        loss.backward()
        assert float(loss) == pytest.approx(float(z[f"c{case}.loss"]), rel=1e-6)
        np.testing.assert_allclose(out.grad.numpy(), z[f"c{case}.grad"], rtol=1e-5, atol=1e-9)
        seg, prior = out.detach()[:, :1], out.detach()[:, 1:]
        branches.append(bool(float(z[f"c{case}.beta"]) * ((seg - prior) ** 2).mean() > torch.nn.BCELoss()(seg, tgt)))
        # the oracle's restatement
        o2 = torch.from_numpy(z[f"c{case}.output"]).requires_grad_(True)
        l2 = O.fbms_joint_loss(o2, tgt, alpha=1.0, beta=float(z[f"c{case}.beta"]), kind="bce", mode="none")
        l2.backward()
        assert float(l2) == pytest.approx(float(z[f"c{case}.loss"]), rel=1e-6)
        np.testing.assert_allclose(o2.grad.numpy(), z[f"c{case}.grad"], rtol=1e-5, atol=1e-9)
    assert True in branches and False in branches        # both sides of the penalty clip are covered


@pytest.mark.parametrize("tag", ["l2_w130_k6", "l1_w24_k4"])
def test_cdn_translate_matches_reference(golden_dir, tag):
    """ConvexDiffeomorphismNet.translate_only_point (the centre-of-mass warm start): same new linear layer as the class.  Compared
    in float64 (the class's own solve in float64: cdn_class_translate_f64.npz): the fp32 least-squares solve of three points
    (condition number ~900) ends ~1e-4 apart on two BLAS builds, in float64 ~1e-13."""
    from awesome_amd.model.diffeomorphism_net import translate_linear, translate_only_point_args
    z = _z(golden_dir, f"cdn_class_{tag}.npz")
    zf = _z(golden_dir, "cdn_class_translate_f64.npz")
    np.testing.assert_array_equal(zf[f"{tag}.sd.linear.weight"], z["sd.linear.weight"].astype(np.float64))   # same net
    np.testing.assert_array_equal(zf[f"{tag}.sd.linear.bias"], z["sd.linear.bias"].astype(np.float64))
    w0, b0 = torch.from_numpy(z["sd.linear.weight"]).double(), torch.from_numpy(z["sd.linear.bias"]).double()
    grid = torch.from_numpy(z["grid"]).double()
    pts = translate_only_point_args(torch.from_numpy(z["tr_src"]), torch.from_numpy(z["tr_dst"]), grid.squeeze(), 2)
    w1, b1 = translate_linear(w0, b0, *pts)
    assert w1.dtype == b1.dtype == torch.float64
    np.testing.assert_allclose(w1.numpy(), zf[f"{tag}.sd_tr.linear.weight"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(b1.numpy(), zf[f"{tag}.sd_tr.linear.bias"], rtol=1e-9, atol=1e-12)
    # and nothing else moved
    for k in z.files:
        if k.startswith("sd_tr.") and not k.startswith("sd_tr.linear."):
            np.testing.assert_array_equal(z[k], z["sd." + k[6:]])


@pytest.mark.parametrize("tag,k", [("l2_w130_k6", 6), ("l1_w24_k4", 4)])
def test_oracle_cdn_forward_matches_the_class(golden_dir, tag, k):
    """The oracle's ICNN(flow(Ax + b)) against ConvexDiffeomorphismNet.forward / get_deformation / BCE gradients of the class
    itself (round 1 pinned it on a hand composition of the sub-modules)."""
    z = _z(golden_dir, f"cdn_class_{tag}.npz")
    sd = {n[3:]: torch.from_numpy(z[n]).clone().requires_grad_(True) for n in z.files if n.startswith("sd.")}
    grid, un = torch.from_numpy(z["grid"]), torch.from_numpy(z["unaries"])
    rows = grid[0].reshape(2, -1).t()
    logits = O.convex_diffeo_forward(sd, rows, k)
    np.testing.assert_allclose(logits.detach().numpy().reshape(z["logits"].shape), z["logits"], rtol=1e-5, atol=2e-6)
    loss = torch.nn.BCELoss()(torch.sigmoid(logits).reshape(un.shape), un)
    assert float(loss) == pytest.approx(float(z["loss"]), rel=1e-6)
    loss.backward()
    for n, p in sd.items():
        ref = z["grad." + n]
        # (weight_v of a weight-normed 1x1 layer has an analytically zero gradient: 1e-9 of rounding on both sides)
        np.testing.assert_allclose(p.grad.numpy().reshape(ref.shape), ref, rtol=2e-4, atol=2e-6 * float(np.abs(ref).max()) + 1e-8,
                                   err_msg=n)


def test_oracle_encode_stage_matches_the_notebook_classes(golden_dir):
    """The encode networks (Fourier features; sine layer) restated in the oracle against the notebooks' own classes executed in the
    build container (tests/golden/encode_notebooks.npz): outputs, input gradients, parameter gradients."""
    z = _z(golden_dir, "encode_notebooks.npz")
    for tag, fwd, post in (("fourier", O.fourier_mlp_forward, lambda y: (y ** 2).mean()),
                           ("sine", O.sine_net_forward, lambda y: (torch.sigmoid(y) ** 2).mean())):
        sd = {k[len(tag) + 4:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith(tag + ".sd.")}
        for k, v in sd.items():
            if v.is_floating_point() and k not in ("A", "b", "offset"):
                v.requires_grad_(True)
        x = torch.from_numpy(z[tag + ".x"]).clone().requires_grad_(True)
        y = fwd(sd, x)
        np.testing.assert_allclose(y.detach().numpy(), z[tag + ".y"], rtol=1e-5, atol=1e-6)
        post(y).backward()
        np.testing.assert_allclose(x.grad.numpy(), z[tag + ".dx"], rtol=1e-4, atol=1e-8)
        for k in z.files:
            if k.startswith(tag + ".grad."):
                name = k[len(tag) + 6:]
                np.testing.assert_allclose(sd[name].grad.numpy(), z[k], rtol=1e-4, atol=1e-8, err_msg=k)
    # the generic form the kernels are checked against (icnn_forward with act0) IS that arithmetic: same features, same first layer
    # (in float64: x @ A + b and linear(x, A^T, b) are two BLAS calls whose fp32 roundings of the arguments (~1e2) differ by an ulp
    # on some BLAS builds, ~4e-6 after the cosine)
    sd = {k[11:]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith("fourier.sd.")}
    x = torch.from_numpy(z["fourier.x"]).double()
    feats = torch.cos(x @ sd["A"] + sd["b"])
    np.testing.assert_allclose(O.encode_layer(torch.nn.functional.linear(x, sd["A"].t(), sd["b"]), "cos").numpy(), feats.numpy(), rtol=1e-6, atol=1e-6)
    p = {"input.weight": sd["A"].t().contiguous(), "input.bias": sd["b"],
         "skip.0.ln.weight": torch.nn.functional.pad(sd["fc1.weight"], (0, 0, 0, 0))[:20, :], "skip.0.ln.bias": sd["fc1.bias"][:20],
         "skip.0.skp.weight": torch.zeros(20, 2, dtype=x.dtype), "out.ln.weight": torch.ones(1, 20, dtype=x.dtype),
         "out.ln.bias": torch.zeros(1, dtype=x.dtype), "out.skp.weight": torch.zeros(1, 2, dtype=x.dtype)}
    ref = torch.relu(torch.nn.functional.linear(feats, sd["fc1.weight"][:20], sd["fc1.bias"][:20])).sum(1, keepdim=True)
    np.testing.assert_allclose(O.icnn_forward(p, x, act0="cos").numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    sds = {k[8:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sine.sd.")}
    xs = torch.from_numpy(z["sine.x"])
    pre = torch.nn.functional.linear(xs + sds["offset"], sds["W1.weight"], sds["W1.bias"])
    np.testing.assert_allclose(O.encode_layer(pre, "sin", 10 * 3.141592).numpy(), torch.sin(10 * 3.141592 * pre).numpy(), rtol=0, atol=0)


def test_oracle_rotation_symmetric_net_matches_the_notebook_class(golden_dir):
    """The rotational-symmetry teaser network (rotation_symmetric.ipynb cell 2) restated in the oracle against the notebook's own
    class executed in the build container (tests/golden/teaser_rotation_symmetric.npz): outputs with and without the symmetry
    prior, input gradients, gradients of every parameter (offset and orientation included), and 8 full-batch Adam steps of the
    notebook's loss."""
    z = _z(golden_dir, "teaser_rotation_symmetric.npz")
    x0 = torch.from_numpy(z["x"])
    for tag, sp in (("free", False), ("sym", True)):
        sd = {k[3:]: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files if k.startswith("sd.")}
        x = x0.clone().requires_grad_(True)
        y = O.rotation_symmetric_forward(sd, x, sp)
        np.testing.assert_allclose(y.detach().numpy(), z[tag + ".y"], rtol=1e-5, atol=1e-6)
        (torch.sigmoid(y) ** 2).mean().backward()
        np.testing.assert_allclose(x.grad.numpy(), z[tag + ".dx"], rtol=1e-4, atol=1e-8)
        for k, v in sd.items():
            np.testing.assert_allclose(v.grad.numpy(), z[f"{tag}.grad.{k}"], rtol=1e-4, atol=1e-8, err_msg=k)
    sd = {k[3:]: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files if k.startswith("sd.")}
    labels = torch.from_numpy(z["labels"])
    back, fore = labels < 0.5, labels > 0.5
    opt = torch.optim.Adam(list(sd.values()), lr=1e-3)
    losses = []
    for _ in range(8):
        ob = torch.sigmoid(O.rotation_symmetric_forward(sd, x0[back], True)).squeeze()
        of = torch.sigmoid(O.rotation_symmetric_forward(sd, x0[fore], True)).squeeze()
        loss = 2 * ((ob - labels[back]) ** 2).mean() + ((of - labels[fore]) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    np.testing.assert_allclose(losses, z["adam8.loss"], rtol=1e-5)
    for k, v in sd.items():
        np.testing.assert_allclose(v.detach().numpy(), z["adam8.sd." + k], rtol=1e-4, atol=2e-6, err_msg=k)


def test_oracle_star_shaped_net_matches_the_notebook_class(golden_dir):
    """The star-shape teaser network (star.ipynb cell 2) restated in the oracle against the notebook's own class
    (tests/golden/teaser_star_shaped.npz): outputs, input gradients, all parameter gradients, 8 Adam steps + W2_r projection."""
    z = _z(golden_dir, "teaser_star_shaped.npz")
    x0 = torch.from_numpy(z["x"])
    sd = {k[3:]: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files if k.startswith("sd.")}
    x = x0.clone().requires_grad_(True)
    y = O.star_shaped_forward(sd, x)
    np.testing.assert_allclose(y.detach().numpy(), z["y"], rtol=1e-5, atol=1e-6)
    (torch.sigmoid(y) ** 2).mean().backward()
    np.testing.assert_allclose(x.grad.numpy(), z["dx"], rtol=1e-4, atol=1e-8)
    for k, v in sd.items():
        np.testing.assert_allclose(v.grad.numpy(), z["grad." + k], rtol=1e-4, atol=1e-8, err_msg=k)
    sd = {k[3:]: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files if k.startswith("sd.")}
    labels = torch.from_numpy(z["labels"])
    opt = torch.optim.Adam(list(sd.values()), lr=1e-2)
    losses = []
    for _ in range(8):
        loss = ((torch.sigmoid(O.star_shaped_forward(sd, x0)).squeeze() - labels) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            sd["W2_r.weight"].clamp_(min=0)
        losses.append(float(loss.detach()))
    np.testing.assert_allclose(losses, z["adam8.loss"], rtol=1e-4)
    for k, v in sd.items():
        np.testing.assert_allclose(v.detach().numpy(), z["adam8.sd." + k], rtol=1e-3, atol=1e-5, err_msg=k)


def test_oracle_star_training_loop_matches_the_notebook_class(golden_dir):
    """O.star_shaped_fit (star.ipynb cell 3 restated on given minibatches) against the recorded 8-step trajectory of the notebook's
    class (full batch, the centre trainable from the start), and its `epoch == k` switch: the centre does not move before epoch k + 1."""
    z = _z(golden_dir, "teaser_star_shaped.npz")
    sd = {k[3:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith("sd.")}
    x, labels = torch.from_numpy(z["x"]), torch.from_numpy(z["labels"])
    full = torch.arange(x.shape[0])[None].repeat(8, 1)
    out, losses = O.star_shaped_fit(sd, x, labels, full, lr=1e-2, offset_free_epoch=None, offset_trainable_from_start=True)
    np.testing.assert_allclose(losses, z["adam8.loss"], rtol=1e-4)
    for k, v in out.items():
        np.testing.assert_allclose(v.numpy(), z["adam8.sd." + k], rtol=1e-3, atol=1e-5, err_msg=k)
    g = torch.Generator().manual_seed(3)
    idx = torch.stack([torch.randperm(x.shape[0], generator=g)[:100] for _ in range(6)])
    out3, _ = O.star_shaped_fit(sd, x, labels, idx[:4], offset_free_epoch=2)     # epochs 0..3: the centre steps once (epoch 3)
    out2, _ = O.star_shaped_fit(sd, x, labels, idx[:3], offset_free_epoch=2)     # epochs 0..2: not yet
    assert torch.equal(out2["offset"], sd["offset"]) and not torch.equal(out3["offset"], sd["offset"])
    # Adam's first step moves a parameter by lr whatever the gradient's size: the centre's own step count starts at its first gradient
    np.testing.assert_allclose((out3["offset"] - sd["offset"]).abs().numpy(), 1e-2, rtol=1e-3)


def test_weighted_loss_on_class_labels_with_noneclass_matches_reference(golden_dir):
    """WeightedLoss(criterion, mode, noneclass) of the reference's FBMS configs (awesome/measures/weighted_loss.py:11-92): the
    oracle's restatement and the host mirror against the reference class's own values and gradients, alone and inside FBMSJointLoss
    (both clip branches)."""
    from awesome_amd.measures import FBMSJointLoss, SE, WeightedLoss
    z = np.load(os.path.join(golden_dir, "weighted_loss_noneclass.npz"))
    out, tgt = torch.from_numpy(z["output"]), torch.from_numpy(z["target"])
    for kind in ("bce", "se"):
        for mode in ("none", "sssdms", "equal"):
            for tag, nc in (("all", None), ("nc2", 2.0)):
                t = tgt if nc is not None else torch.where(tgt == 2.0, torch.ones_like(tgt), tgt)
                key = f"{kind}.{mode}.{tag}"
                o = out[:, :1].clone().requires_grad_(True)
                lo = O.weighted_loss(o, t, kind=kind, mode=mode, noneclass=nc, class_targets=True)
                lo.backward()
                assert float(lo.detach()) == pytest.approx(float(z[key + ".loss"]), rel=1e-6), key
                np.testing.assert_allclose(o.grad.numpy(), z[key + ".grad"], rtol=1e-5, atol=1e-9, err_msg=key)
                inner = torch.nn.BCELoss() if kind == "bce" else SE("mean")
                o2 = out[:, :1].clone().requires_grad_(True)
                lm = WeightedLoss(inner, mode=mode, noneclass=nc)(o2, t)
                lm.backward()
                assert float(lm.detach()) == pytest.approx(float(z[key + ".loss"]), rel=1e-6), key
                np.testing.assert_allclose(o2.grad.numpy(), z[key + ".grad"], rtol=1e-5, atol=1e-9, err_msg=key)
    for case in range(2):
        beta = float(z[f"fbms{case}.beta"])
        o = out.clone().requires_grad_(True)
        lo = O.fbms_joint_loss(o, tgt, alpha=1.0, beta=beta, kind="bce", mode="sssdms", noneclass=2.0, class_targets=True)
        lo.backward()
        assert float(lo.detach()) == pytest.approx(float(z[f"fbms{case}.loss"]), rel=1e-6)
        np.testing.assert_allclose(o.grad.numpy(), z[f"fbms{case}.grad"], rtol=1e-5, atol=1e-9)
        o2 = out.clone().requires_grad_(True)
        lm = FBMSJointLoss(criterion=WeightedLoss(torch.nn.BCELoss(), mode="sssdms", noneclass=2), alpha=1.0, beta=beta)(o2, tgt)
        lm.backward()
        assert float(lm.detach()) == pytest.approx(float(z[f"fbms{case}.loss"]), rel=1e-6)
        np.testing.assert_allclose(o2.grad.numpy(), z[f"fbms{case}.grad"], rtol=1e-5, atol=1e-9)


def test_simple_resnet_backbone_is_constructed_like_the_reference_class(golden_dir):
    """NormalizingFlow1D's 'resnet' backbone (SimpleResnet / ResidualBlock1D, diffeomorphism_net.py:107-166; real_nvp/resnet_1d.py:66-95):
    the same parameter names in the same order as the class, and - from the same seed - the same initial values (creation order and the
    random draws of the initialisers, including the ones weights_init_normal spends on the derived `.weight`)."""
    import json
    import random
    from awesome_amd.model import ConvexDiffeomorphismNet
    z = _z(golden_dir, "cdn_class_resnet.npz")
    random.seed(23)
    np.random.seed(23)
    torch.manual_seed(23)
    m = ConvexDiffeomorphismNet(**json.loads(str(z["kwargs"])))
    sd = m.state_dict()
    ref = {k[3:]: z[k] for k in z.files if k.startswith("sd.")}
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), ref[k].reshape(v.shape), err_msg=k)
    with pytest.raises(NotImplementedError):
        m._specs()                       # no fused flow kernel for a backbone that normalises over the points
