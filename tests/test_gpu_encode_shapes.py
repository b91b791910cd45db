"""The notebooks' encode nets at their own shapes on the layer-by-layer path (ABI 8: n_features, n_out, no hidden layer):
`ourSimpleNetwork` (imageRepresentationTest.ipynb cells 5-6: cos(x @ A + b), 20 features -> 3 x 350 relu -> 3 outputs -> sigmoid, MSELoss,
Adam 1e-3) and `myNet` (repeating.ipynb cells 3-4: sin(10 pi W1(x + offset)) -> W2, 2 MSE(bg) + MSE(fg) on 500 + 500 samples per epoch).
References: the notebook classes' own numbers (tests/golden/encode_notebooks.npz) and the oracle restatements pinned to them
(O.fourier_mlp_forward, O.sine_net_forward).  Bars as in test_gpu_encode.py: outputs 1e-4, gradients 3e-3 of the tensor maximum."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import inr_oracle as O  # noqa: E402  (checker only)

GOLD = "tests/golden/encode_notebooks.npz"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gold():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), GOLD))


def _close(got, ref, bar=3e-3, name=""):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, rtol=bar, atol=bar * float(np.abs(ref).max()) + 1e-9, err_msg=name)


def _notebook_sd(m):
    """The module's state as `ourSimpleNetwork`'s state_dict (the head is the notebook's fc{L+1})."""
    n = m.spec.n_layers
    return {("fc%d" % (n + 1) + k[3:] if k.startswith("out.") else k): v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _logits_chain(sd, x):
    """fourier_mlp_forward without the final sigmoid (the kernels return logits)."""
    z = torch.cos(x @ sd["A"] + sd["b"])
    n = sum(1 for k in sd if k.startswith("fc") and k.endswith(".weight"))
    for k in range(1, n):
        z = F.relu(F.linear(z, sd[f"fc{k}.weight"], sd[f"fc{k}.bias"]))
    return F.linear(z, sd[f"fc{n}.weight"], sd[f"fc{n}.bias"])


def _coords(w, h):
    return O.positional_grid(w, h).reshape(2, -1).t().contiguous()   # (N, 2), point p = row * w + col, like Grid.linspace


def test_reference_replay_of_both_notebook_classes(dev):
    """encode_notebooks.npz was generated at ourSimpleNetwork(2, 20, 24, 1, 30) - 20 features under 24-unit layers - and myNet(16) - no
    hidden layer: load the classes' state_dicts through the loaders, replay the fixture's losses and compare with its numbers."""
    from awesome_amd.model import FourierFeatureNet, SineLayerNet
    z = _gold()
    m = FourierFeatureNet(d_in=2, d_features=20, n_hidden=24, n_hidden_layers=3, d_out=1, factor=30).to(dev)
    m.load_notebook_state_dict({k[11:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("fourier.sd.")})
    x = torch.from_numpy(z["fourier.x"]).to(dev).requires_grad_(True)
    y = torch.sigmoid(m(x))                                     # the fixture's y is post-sigmoid
    assert y.shape == (120, 1)
    np.testing.assert_allclose(y.detach().cpu().numpy(), z["fourier.y"], atol=1e-4, rtol=1e-4)
    (y ** 2).mean().backward()
    _close(x.grad, z["fourier.dx"], name="fourier dx")
    for k in z.files:
        if k.startswith("fourier.grad."):
            name = k[13:].replace("fc4.", "out.")
            _close(dict(m.named_parameters())[name].grad, z[k], name=k)
    assert m.A.grad is None and m.b.grad is None

    s = SineLayerNet(in_features=2, n_hidden=16, n_hidden_layers=0).to(dev)
    s.load_notebook_state_dict({k[8:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sine.sd.")})
    x2 = torch.from_numpy(z["sine.x"]).to(dev).requires_grad_(True)
    y2 = s(x2)
    np.testing.assert_allclose(y2.detach().cpu().numpy(), z["sine.y"], atol=1e-4, rtol=1e-4)
    (torch.sigmoid(y2) ** 2).mean().backward()
    _close(x2.grad, z["sine.dx"], name="sine dx")
    for k in z.files:
        if k.startswith("sine.grad."):
            name = k[10:].replace("W2.", "out.")
            _close(dict(s.named_parameters())[name].grad, z[k], name=k)


def test_notebook_shape_on_a_ragged_grid(dev):
    """2 -> 20 -> 3 x 350 -> 3 on 37 x 41 points: logits, the MSE-on-sigmoid loss against RGB targets, every gradient and dL/dcoords."""
    import awesome_amd as A
    from awesome_amd.model import FourierFeatureNet
    torch.manual_seed(5)
    m = FourierFeatureNet(d_in=2, d_features=20, n_hidden=350, n_hidden_layers=3, d_out=3, factor=30).to(dev)
    W, H = 37, 41
    xc = _coords(W, H)
    tgt = torch.rand(W * H, 3)
    sd = _notebook_sd(m)
    for k, v in sd.items():
        if k.startswith("fc"):
            v.requires_grad_(True)
    xo = xc.clone().requires_grad_(True)
    yo = O.fourier_mlp_forward(sd, xo)
    lo = F.mse_loss(yo, tgt)
    lo.backward()
    # logits through the C ABI: [1, 3, N]
    flat = m.flat_parameters()[None].contiguous()
    grid = A.Grid.explicit(xc.t().contiguous().to(dev))
    logits = A.forward(m.spec, flat, grid)
    assert logits.shape == (1, 3, W * H)
    np.testing.assert_allclose(logits[0].t().cpu().numpy(), _logits_chain({k: v.detach() for k, v in sd.items()}, xc).numpy(), atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(torch.sigmoid(logits[0].t()).cpu().numpy(), yo.detach().numpy(), atol=1e-4, rtol=1e-4)
    loss, grads = A.loss_grad(m.spec, flat, grid, tgt.t().contiguous()[None].to(dev))
    assert float(loss[0]) == pytest.approx(float(lo.detach()), rel=1e-4)
    got = A.unpack_params(m.spec, grads[0].cpu())
    for k in range(1, 4):
        _close(got[f"skip.{k - 1}.ln.weight"], sd[f"fc{k}.weight"].grad, name=f"fc{k}.weight")
        _close(got[f"skip.{k - 1}.ln.bias"], sd[f"fc{k}.bias"].grad, name=f"fc{k}.bias")
    _close(got["out.ln.weight"], sd["fc4.weight"].grad, name="fc4.weight")
    _close(got["out.ln.bias"], sd["fc4.bias"].grad, name="fc4.bias")
    # the module surface: (N, 3) logits, autograd into the layers and into the coordinates
    x = xc.to(dev).requires_grad_(True)
    y = m(x)
    assert y.shape == (W * H, 3)
    F.mse_loss(torch.sigmoid(y), tgt.to(dev)).backward()
    _close(x.grad, xo.grad, name="dcoords")
    for k in range(1, 4):
        _close(getattr(m, f"fc{k}").weight.grad, sd[f"fc{k}.weight"].grad, name=f"module fc{k}")
    _close(m.out.weight.grad, sd["fc4.weight"].grad, name="module out")
    # (B, C, H, W) in, (B, 3, H, W) out
    img = O.positional_grid(W, H)[None].to(dev)
    assert m(img).shape == (1, 3, H, W)


def test_notebook_shape_full_size_loss_grad(dev):
    """One loss_grad of the notebook shape at 256 x 256 (65 536 points: many chunks of every split contraction) against the oracle in
    float64: loss rel 2e-5, gradients 3e-3 of the maximum."""
    import awesome_amd as A
    from awesome_amd.model import FourierFeatureNet
    torch.manual_seed(7)
    m = FourierFeatureNet(d_in=2, d_features=20, n_hidden=350, n_hidden_layers=3, d_out=3, factor=30).to(dev)
    S = 256
    xc = _coords(S, S)
    tgt = torch.stack([(xc[:, 0] * 3).sin() * 0.5 + 0.5, xc[:, 1], (xc[:, 0] > 0.5).float()], 1)   # an RGB picture
    sd = {k: v.double() for k, v in _notebook_sd(m).items()}
    for k, v in sd.items():
        if k.startswith("fc"):
            v.requires_grad_(True)
    lo = F.mse_loss(O.fourier_mlp_forward(sd, xc.double()), tgt.double())
    lo.backward()
    flat = m.flat_parameters()[None].contiguous()
    loss, grads = A.loss_grad(m.spec, flat, A.Grid.linspace(S, S, dev), tgt.t().contiguous()[None].to(dev))
    assert float(loss[0]) == pytest.approx(float(lo.detach()), rel=2e-5)
    got = A.unpack_params(m.spec, grads[0].cpu())
    for k in range(1, 4):
        _close(got[f"skip.{k - 1}.ln.weight"], sd[f"fc{k}.weight"].grad, name=f"fc{k}.weight")
        _close(got[f"skip.{k - 1}.ln.bias"], sd[f"fc{k}.bias"].grad, name=f"fc{k}.bias")
    _close(got["out.ln.weight"], sd["fc4.weight"].grad, name="fc4.weight")
    _close(got["out.ln.bias"], sd["fc4.bias"].grad, name="fc4.bias")


def _fit_notebook_shape(dev, steps=5):
    import awesome_amd as A
    from awesome_amd.model import FourierFeatureNet
    torch.manual_seed(11)
    m = FourierFeatureNet(d_in=2, d_features=20, n_hidden=350, n_hidden_layers=3, d_out=3, factor=30)
    S = 64
    xc = _coords(S, S)
    tgt = torch.stack([xc[:, 0], 1 - xc[:, 1], ((xc - 0.5) ** 2).sum(1).sqrt()], 1)
    flat = m.flat_parameters()[None].contiguous().to(dev)
    res = A.fit(m.spec, flat.clone(), A.Grid.linspace(S, S, dev), tgt.t().contiguous()[None].to(dev), steps, lr=1e-3, loss="se",
                optimizer="adam", **FourierFeatureNet.fit_options)
    return m, flat, xc, tgt, res


def test_notebook_shape_fit_trajectory(dev):
    """64 x 64, Adam lr 1e-3 on the layers with the features frozen (the notebook's buffers), 5 steps: the loss history and the parameters
    against an oracle Adam loop; A and b are bit-unchanged; the logits come back [1, 3, N]."""
    import awesome_amd as A
    m, flat, xc, tgt, res = _fit_notebook_shape(dev)
    assert int(res.status[0]) == 0 and res.logits.shape == (1, 3, xc.shape[0])
    p = {k: v.clone() for k, v in _notebook_sd(m).items()}
    learn = {k: v.requires_grad_(True) for k, v in p.items() if k.startswith("fc")}
    st = O.AdamState(learn)
    losses = []
    for _ in range(5):
        for v in learn.values():
            v.grad = None
        lo = F.mse_loss(O.fourier_mlp_forward(p, xc), tgt)
        lo.backward()
        O.adam_step(learn, {k: v.grad for k, v in learn.items()}, st, lr=1e-3)
        losses.append(float(lo.detach()))
    np.testing.assert_allclose(res.loss_hist[0].cpu().numpy(), np.asarray(losses, np.float32), rtol=1e-4)
    got = A.unpack_params(m.spec, res.params[0].cpu())
    ref0 = A.unpack_params(m.spec, flat[0].cpu())
    assert torch.equal(got["input.weight"], ref0["input.weight"]) and torch.equal(got["input.bias"], ref0["input.bias"])
    # Adam moves a weight by ~lr per step whatever the size of its gradient: where a gradient is ~0, m / sqrt(v) follows its rounding
    # (and the CPU oracle's BLAS rounding differs from box to box), so a few isolated weights part by a fraction of a step.  Bar: the
    # usual fit bar (rtol 1e-3, atol 5e-6) for >= 99.5 % of every tensor and on average, every element within one step (lr)
    pairs = [(f"skip.{k - 1}.ln.weight", f"fc{k}.weight") for k in range(1, 4)] + [(f"skip.{k - 1}.ln.bias", f"fc{k}.bias") for k in range(1, 4)]
    for mine, ref in pairs + [("out.ln.weight", "fc4.weight"), ("out.ln.bias", "fc4.bias")]:
        d = learn[ref].detach()
        err = (got[mine] - d).abs()
        ok = err <= 5e-6 + 1e-3 * d.abs()
        assert float(ok.float().mean()) >= 0.995, (mine, int((~ok).sum()))
        assert float(err.max()) < 1e-3 and float(err.mean()) < 5e-6, (mine, float(err.max()), float(err.mean()))
    assert float(got["out.skp.weight"].abs().max()) == 0.0


def test_notebook_shape_fit_is_deterministic(dev):
    _, _, _, _, r1 = _fit_notebook_shape(dev)
    _, _, _, _, r2 = _fit_notebook_shape(dev)
    assert torch.equal(r1.params, r2.params) and torch.equal(r1.loss_hist, r2.loss_hist) and torch.equal(r1.logits, r2.logits)


def test_sine_notebook_loop(dev):
    """myNet(200) and its loop: per epoch 500 + 500 seeded samples of the background / foreground pixels, loss 2 MSE(bg) + 1 MSE(fg)
    (INR_WEIGHT_EXPLICIT c_fg = 2/500 on targets < 0.5, c_bg = 1/500), Adam lr 1e-2 continued across the epochs' fit calls, each on an
    explicit grid of its 1000 samples - against the same loop on the oracle."""
    import awesome_amd as A
    from awesome_amd.model import SineLayerNet
    n = 48
    yy, xx = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    lik = 0.5 + 0.45 * torch.sin(2 * np.pi * (xx + 0.5 * yy).float() / 12.0)      # a repeating pattern
    lik = torch.where((lik - 0.5).abs() < 0.02, lik + 0.05, lik)

    def pix(mask):
        idx = torch.nonzero(mask)
        return torch.stack([idx[:, 0] / n - 0.5, idx[:, 1] / n - 0.5], 1).float(), lik[mask]

    pb, lb = pix(lik < 0.5)
    pf, lf = pix(lik > 0.5)
    torch.manual_seed(1)
    m = SineLayerNet(in_features=2, n_hidden=200, n_hidden_layers=0)
    sd = {"offset": m.offset.detach().clone(), "W1.weight": m.W1.weight.detach().clone(), "W1.bias": m.W1.bias.detach().clone(),
          "W2.weight": m.out.weight.detach().clone(), "W2.bias": m.out.bias.detach().clone()}
    learn = {k: v.requires_grad_(True) for k, v in sd.items() if k != "offset"}
    st = O.AdamState(learn)
    flat = m.flat_parameters()[None].contiguous().to(dev)
    opt = A.icnn.new_opt_state(m.spec, 1, dev)
    gen = torch.Generator().manual_seed(3)
    got_losses, ref_losses = [], []
    for epoch in range(5):
        ib = torch.randperm(pb.shape[0], generator=gen)[:500]
        i_f = torch.randperm(pf.shape[0], generator=gen)[:500]
        xb, xf, tb, tf = pb[ib], pf[i_f], lb[ib], lf[i_f]
        # oracle: the notebook's loss on the notebook's net
        for v in learn.values():
            v.grad = None
        ob = torch.sigmoid(O.sine_net_forward(sd, xb)).squeeze()
        of = torch.sigmoid(O.sine_net_forward(sd, xf)).squeeze()
        lo = 2 * F.mse_loss(ob, tb) + 1 * F.mse_loss(of, tf)
        lo.backward()
        O.adam_step(learn, {k: v.grad for k, v in learn.items()}, st, lr=1e-2)
        ref_losses.append(float(lo.detach()))
        # device: one step on this epoch's samples
        grid = A.Grid.explicit(torch.cat([xb, xf], 0).t().contiguous().to(dev))
        res = A.fit(m.spec, flat, grid, torch.cat([tb, tf])[None].to(dev), 1, lr=1e-2, loss="se", weight_mode="explicit", c_fg=2 / 500,
                    c_bg=1 / 500, optimizer="adam", opt_state=opt, step0=epoch, want_logits=False, **SineLayerNet.fit_options)
        assert int(res.status[0]) == 0
        got_losses.append(float(res.loss_hist[0, 0]))
    np.testing.assert_allclose(np.asarray(got_losses), np.asarray(ref_losses), rtol=1e-4)
    got = A.unpack_params(m.spec, flat[0].cpu())
    np.testing.assert_allclose(got["input.weight"].numpy(), learn["W1.weight"].detach().numpy(), rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(got["input.bias"].numpy(), learn["W1.bias"].detach().numpy(), rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(got["out.ln.weight"].numpy(), learn["W2.weight"].detach().numpy(), rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(got["out.ln.bias"].numpy(), learn["W2.bias"].detach().numpy(), rtol=2e-3, atol=2e-5)
