"""The binding's argument checks with CUDA tensors: a tensor of the wrong width is a ValueError in front of every launch - the
parameters are bit for bit what they were - and a valid call of every family still returns finite results of the documented shapes.
h = 8, a 4 x 3 grid (N = 12), two images; tests/test_binding_host.py holds the full table on the CPU."""
import pytest
import torch

import awesome_amd as A
from awesome_amd import flow as FL
from awesome_amd import icnn as K
from awesome_amd import joint as J
from awesome_amd import minibatch as MB
from awesome_amd import rnvp as R
from awesome_amd import star as ST
from awesome_amd import symmetric as SY

pytestmark = pytest.mark.gpu

H, N, NI, STEPS = 8, 12, 2, 3
ISPEC, SSPEC = A.IcnnSpec(H, 2, 1), A.IcnnSpec(H, 3, 1)
FSPEC, RSPEC = FL.FlowSpec(8, 2), R.RnvpSpec(2, 8, 2)
P, SP, FP, RP = ISPEC.n_params, SSPEC.n_params, FSPEC.n_params, RSPEC.n_params


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(g, *shape, scale=0.3):
    return scale * torch.randn(*shape, generator=g)


def _cases(dev):
    """name -> (function, its valid arguments, the parameter tensors it updates in place, the names of its second parameter tensor and of
    that tensor's optimizer state)."""
    g = torch.Generator().manual_seed(0)
    grid = K.Grid.linspace(4, 3, dev)
    tg = (torch.rand(NI, N, generator=g) > 0.5).float().to(dev)
    ip, sp = _rand(g, NI, P).abs().to(dev), _rand(g, NI, SP).to(dev)
    cp = _rand(g, NI, FP)
    cp[:, :4] = torch.eye(2).reshape(-1)
    rp = R.actnorm_init(RSPEC, torch.stack([R.init_rnvp_params(RSPEC) + _rand(g, RP, scale=0.1) for _ in range(NI)]).to(dev), grid)
    pose = (torch.tensor([0.45, 0.55, 0.3]) + _rand(g, NI, 3, scale=0.05)).to(dev)
    zeros = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    return {
        "cdn_fit": (FL.cdn_fit, dict(ispec=ISPEC, fspec=FSPEC, icnn_params=ip.clone(), flow_params=cp.to(dev), grid=grid, targets=tg, steps=STEPS,
                                     icnn_opt_state=zeros(NI, 2 * P + 8), flow_opt_state=zeros(NI, 2 * FP)),
                    ("icnn_params", "flow_params"), "flow_params", "flow_opt_state"),
        "pcn_fit": (R.pcn_fit, dict(ispec=ISPEC, rspec=RSPEC, icnn_params=ip.clone(), flow_params=rp.clone(), grid=grid, targets=tg, steps=STEPS,
                                    icnn_opt_state=zeros(NI, 2 * P + 8), flow_opt_state=zeros(NI, 2 * RP)),
                    ("icnn_params", "flow_params"), "flow_params", "flow_opt_state"),
        "sym_fit": (SY.sym_fit, dict(spec=SSPEC, params=sp.clone(), pose=pose, grid=grid, targets=tg, steps=STEPS, opt_state=zeros(NI, 2 * SP + 8),
                                     pose_opt_state=zeros(NI, 6)), ("params", "pose"), "pose", "pose_opt_state"),
        "pcn_joint_step": (J.pcn_joint_step,
                           dict(ispec=ISPEC, rspec=RSPEC, icnn_params=ip[:1].clone(), flow_params=rp[:1].clone(), icnn_opt_state=zeros(1, 2 * P + 8),
                                flow_opt_state=zeros(1, 2 * RP), grid=grid, seg=torch.rand(N, generator=g).to(dev), target=tg[0].clone(),
                                desc=J.joint_desc(), step=1, lr=1e-3), ("icnn_params", "flow_params"), "flow_params", "flow_opt_state"),
    }


NAMES = ["cdn_fit", "pcn_fit", "sym_fit", "pcn_joint_step"]


@pytest.mark.parametrize("name", NAMES)
def test_wrong_widths_are_refused_before_any_launch(dev, name):
    """The second parameter tensor (flow_params; the pose of sym_fit) one float short, the targets one column long, an optimizer state of
    the wrong width: ValueError each, and the parameter tensors are bit for bit what they were."""
    fn, kw, params, second, state = _cases(dev)[name]
    target = "target" if "target" in kw else "targets"
    before = {k: kw[k].clone() for k in params}
    spoil = {second: lambda t: t[..., :-1].contiguous(),
             target: lambda t: torch.cat([t, t[..., :1]], -1),
             state: lambda t: t[..., :-2].contiguous()}
    for arg, change in spoil.items():
        bad = dict(kw, **{arg: change(kw[arg])})
        with pytest.raises(ValueError, match=rf"\b{arg}\b"):
            fn(**bad)
        torch.cuda.synchronize()
        for k in params:
            assert torch.equal(kw[k], before[k]), (arg, k)


@pytest.mark.parametrize("name", NAMES)
def test_valid_calls_still_work(dev, name):
    fn, kw, params, _, _ = _cases(dev)[name]
    before = {k: kw[k].clone() for k in params}
    r = fn(**kw)
    torch.cuda.synchronize()
    if name == "pcn_joint_step":
        assert tuple(r.loss.shape) == (4,) and tuple(r.dseg.shape) == (N,) and tuple(r.prior_logits.shape) == (N,)
        outs = [r.loss, r.dseg, r.prior_logits]
    else:
        assert tuple(r.loss_hist.shape) == (NI, STEPS)
        outs = [r.loss_hist] + ([r.logits] if name != "sym_fit" else [])
        if name != "sym_fit":
            assert tuple(r.logits.shape) == (NI, N)
    assert int(r.status.abs().sum()) == 0
    for t in outs + [kw[k] for k in params]:
        assert bool(torch.isfinite(t).all())
    assert any(not torch.equal(kw[k], before[k]) for k in params)          # in place: the step was taken


def test_plain_icnn_minibatch_and_star_still_work(dev):
    g = torch.Generator().manual_seed(1)
    grid = K.Grid.linspace(4, 3, dev)
    tg = (torch.rand(NI, N, generator=g) > 0.5).float().to(dev)
    ip = _rand(g, NI, P).abs().to(dev)
    r = K.fit(ISPEC, ip.clone(), grid, tg, STEPS)
    assert tuple(r.loss_hist.shape) == (NI, STEPS) and tuple(r.logits.shape) == (NI, N) and tuple(r.opt_state.shape) == (NI, 2 * P + 8)
    assert bool(torch.isfinite(r.loss_hist).all()) and bool(torch.isfinite(r.logits).all())
    assert tuple(K.forward(ISPEC, ip, grid).shape) == (NI, N)
    pool = torch.rand(2, N, generator=g).to(dev)
    index = torch.stack([torch.randperm(N, generator=g)[:5] for _ in range(STEPS)]).to(torch.int32)
    m = MB.fit_minibatch(ISPEC, ip.clone(), pool, tg, index)
    assert tuple(m.loss_hist.shape) == (NI, STEPS) and m.logits is None and bool(torch.isfinite(m.loss_hist).all())
    with pytest.raises(ValueError, match="pool_targets"):
        MB.fit_minibatch(ISPEC, ip.clone(), pool, tg[:, :-1], index)
    star = ST.StarSpec(H)
    sp = _rand(g, star.n_params).to(dev)
    s = ST.star_fit(star, sp, pool.t().contiguous(), tg[0].clone(), index)
    assert tuple(s.loss_hist.shape) == (STEPS,) and tuple(s.opt_state.shape) == (2 * star.n_params,)
    assert bool(torch.isfinite(s.loss_hist).all()) and bool(torch.isfinite(s.params).all())
    with pytest.raises(ValueError, match="params"):
        ST.star_fit(star, sp[:-1].contiguous(), pool.t().contiguous(), tg[0].clone(), index)
