"""The two backbones of the host driver (csrc/inrfit.hip: FusedIcnn, WideIcnn) obey one step protocol, with and without the
RealNVP in front of them:

* a fit of k steps equals, bit for bit, k calls of one step each that hand on the optimizer states and pass `step0` - parameters,
  both moments and the header (the whole optimizer state), the loss history and the status;
* `logits_at_last_forward` returns the logits of the last training forward, i.e. of the parameters BEFORE the last optimizer step:
  the same numbers as an inference pass at those parameters.

Shapes: the fused kernels' widest (h = 130, one and two hidden layers) and the layer-by-layer path's narrowest pair (h = 136 x 1: the
first row stride past the fused kernels; h = 64 x 3: deep); a 24 x 20 grid and a ragged 23 x 19 one (437 points: a multiple of neither
16 nor 64); one and two images; 3 steps under Adamax with a plateau scheduler of patience 1, so that the header's learning-rate
slots and counters change between the calls.

Bars.  The first property compares two runs of the same kernels on the same inputs in the same order: equality.  The second compares
the training pass's logits with the inference pass's at identical parameters.  Layer by layer both are the same kernels (the
`train` flag only adds outputs): equality.  The fused step kernel's training and inference instantiations evaluate the same fp32
expressions with explicit fmaf and -ffp-contract=off (awesome_amd/build.py), in the same order: equality as well."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"fused-130x1": (130, 1), "fused-130x2": (130, 2), "wide-136x1": (136, 1), "wide-64x3": (64, 3)}
GRIDS = {"24x20": (24, 20), "23x19": (23, 19)}
STEPS = 3
KW = dict(lr=4e-3, optimizer="adamax", plateau=dict(patience=1, factor=0.5))


@pytest.fixture(scope="module")
def dev():
    import awesome_amd._lib as L
    L.load()
    return torch.device("cuda:0")


def _case(shape, grid, n, deform, dev):
    """(spec, rspec or None, ICNN params [n, P], RealNVP params [n, RP] or None, grid, targets [n, N])"""
    import awesome_amd as A
    from awesome_amd import icnn as K
    from awesome_amd import rnvp as R
    from awesome_amd.model import ConvexNextNet
    h, layers = SHAPES[shape]
    W, H = GRIDS[grid]
    spec, g = A.IcnnSpec(h, 2, layers), K.Grid.linspace(W, H, dev)
    rows = []
    for i in range(n):
        torch.manual_seed(100 * h + 10 * layers + W + i)
        rows.append(A.pack_state_dict(spec, ConvexNextNet(n_hidden=h, n_hidden_layers=layers, in_features=2).state_dict()))
    ip = torch.stack(rows).to(dev).contiguous()
    gen = torch.Generator().manual_seed(h + W)
    tg = (torch.rand(n, W * H, generator=gen) > 0.55).float().to(dev)
    if deform == "none":
        return spec, None, ip, None, g, tg
    rspec = R.RnvpSpec(2, 32, 4, "tanh", None, (-0.1, 0.0), (1.2, 1.0))
    rows = []
    for i in range(n):
        torch.manual_seed(7 * h + W + i)
        p = R.init_rnvp_params(rspec)
        rows.append(p + 0.1 * torch.randn(p.shape))   # every parameter non-trivial (the factory zeroes the MLPs' last layers)
    fp = R.actnorm_init(rspec, torch.stack(rows).to(dev).contiguous(), g)
    return spec, rspec, ip, fp, g, tg


def _fit(case, ip, fp, steps, step0=0, iopt=None, fopt=None, gate=False):
    """-> dict of every tensor the fit leaves behind"""
    from awesome_amd import icnn as K
    from awesome_amd import rnvp as R
    spec, rspec, _, _, g, tg = case
    if rspec is None:
        r = K.fit(spec, ip, g, tg, steps, opt_state=iopt, step0=step0, gate_logits=gate, **KW)
        return dict(params=r.params, opt=r.opt_state, hist=r.loss_hist, logits=r.logits, status=r.status)
    r = R.pcn_fit(spec, rspec, ip, fp, g, tg, steps, icnn_opt_state=iopt, flow_opt_state=fopt, step0=step0, gate_logits=gate,
                  flow_weight_decay=1e-5, **KW)
    return dict(params=r.icnn_params, opt=r.icnn_opt_state, flow=r.flow_params, flow_opt=r.flow_opt_state, hist=r.loss_hist, logits=r.logits,
                status=r.status)


def _forward(case, ip, fp):
    from awesome_amd import icnn as K
    from awesome_amd import rnvp as R
    spec, rspec, _, _, g, _ = case
    return K.forward(spec, ip, g) if rspec is None else R.pcn_forward(spec, rspec, ip, fp, g)


def _clone(t):
    return None if t is None else t.clone()


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("deform", ["none", "rnvp"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fit_of_k_steps_equals_k_fits_of_one_step(dev, shape, deform, grid, n):
    case = _case(shape, grid, n, deform, dev)
    one = _fit(case, _clone(case[2]), _clone(case[3]), STEPS)
    ip, fp, iopt, fopt, hist, status = _clone(case[2]), _clone(case[3]), None, None, [], torch.zeros(n, dtype=torch.int32, device=dev)
    for it in range(STEPS):
        r = _fit(case, ip, fp, 1, step0=it, iopt=iopt, fopt=fopt)
        ip, fp, iopt, fopt = r["params"], r.get("flow"), r["opt"], r.get("flow_opt")
        hist.append(r["hist"].clone())
        status |= r["status"]
    assert torch.isfinite(one["hist"]).all() and int(one["status"].abs().sum()) == 0
    assert not torch.equal(one["params"], case[2])                     # the steps did move the parameters
    assert torch.equal(ip, one["params"]), (ip - one["params"]).abs().max()
    assert torch.equal(iopt, one["opt"]), (iopt - one["opt"]).abs().max()   # both moments and the header
    if deform == "rnvp":
        assert not torch.equal(one["flow"], case[3])
        assert torch.equal(fp, one["flow"]) and torch.equal(fopt, one["flow_opt"])
    assert torch.equal(torch.cat(hist, 1), one["hist"])
    assert torch.equal(status, one["status"])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("deform", ["none", "rnvp"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_logits_at_last_forward_are_those_of_the_parameters_before_the_last_step(dev, shape, deform, grid, n):
    case = _case(shape, grid, n, deform, dev)
    before = _fit(case, _clone(case[2]), _clone(case[3]), STEPS - 1)
    want = _forward(case, before["params"], before.get("flow"))
    gated = _fit(case, _clone(case[2]), _clone(case[3]), STEPS, gate=True)
    plain = _fit(case, _clone(case[2]), _clone(case[3]), STEPS)
    print("max |gated - forward(before)|", float((gated["logits"] - want).abs().max()))
    assert torch.equal(gated["params"], plain["params"])               # the switch changes what is returned, not what is computed
    assert not torch.equal(gated["logits"], plain["logits"])
    assert torch.equal(gated["logits"], want)
