"""The pixel-minibatch fits on the host (no GPU): the binding, the argument checks of both entry points, the size query, the index
tables, and the float32 / float64 restatements the GPU parity test leans on."""
import ctypes

import pytest
import torch

from tests import minibatch_cases as MC
from tests.test_abi import _declared_functions

_FAKE = 0x1000   # a device pointer that is never dereferenced: every case below is answered on the host
_EINVAL, _EUNSUPPORTED, _EWORKSPACE = -1, -2, -3


def test_exports_still_equal_the_header():
    from awesome_amd import _lib
    names = _declared_functions()
    assert set(_lib.EXPORTS) == set(names)
    for must in ("inrfit_minibatch_workspace_bytes", "inrfit_fit_minibatch", "inrfit_cdn_fit_minibatch"):
        assert must in names
    lib = _lib.load()
    ver = ctypes.c_int()
    assert lib.inrfit_query(ctypes.byref(ver), None, None) == 0 and ver.value == 8   # additions only


# ---- single-fault table: a valid call with ONE argument spoiled, answered before the first HIP call --------------------------------
def _args(**over):
    from awesome_amd import _lib as L
    a = dict(model=(130, 2, 1, 0, 0, 0), flow=(16, 2, L.INR_FLOW_NORMAL_BLOCK), loss=(L.INR_LOSS_SE, L.INR_WEIGHT_NONE), opt=L.INR_OPT_ADAM,
             params=_FAKE, opt_state=_FAKE, flow_params=_FAKE, flow_opt_state=_FAKE, pool_coords=_FAKE, pool_targets=_FAKE, n_pool=1000,
             index=_FAKE, counts=None, batch=200, n=1, steps=3, step0=0, ws=_FAKE, wsb=1 << 40)
    a.update(over)
    h, c, layers, act0, nf, no = a["model"]
    a["model"] = L.InrModelDesc(L.INR_MODEL_ICNN, h, c, layers, act0, 1.0, nf, no)
    a["flow"] = L.InrFlowDesc(*a["flow"])
    a["loss"] = None if a["loss"] is None else L.InrLossDesc(*a["loss"], 1.0, 0.0, 0.0)
    a["opt"] = None if a["opt"] is None else L.InrOptDesc(a["opt"], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0, 0)
    if a["counts"] is not None:
        a["counts"] = (ctypes.c_int32 * len(a["counts"]))(*a["counts"])
    return a


_ENTRY = {
    "fit": lambda lib, a: lib.inrfit_fit_minibatch(a["model"], a["params"], a["opt_state"], a["pool_coords"], a["pool_targets"], a["n_pool"],
                                                   a["index"], a["counts"], a["batch"], a["loss"], a["opt"], a["n"], a["steps"], a["step0"],
                                                   None, None, a["ws"], a["wsb"], None),
    "cdn": lambda lib, a: lib.inrfit_cdn_fit_minibatch(a["model"], a["flow"], a["params"], a["flow_params"], a["opt_state"],
                                                       a["flow_opt_state"], a["pool_coords"], a["pool_targets"], a["n_pool"], a["index"],
                                                       a["counts"], a["batch"], a["loss"], a["opt"], 0.0, a["n"], a["steps"], a["step0"],
                                                       None, None, a["ws"], a["wsb"], None),
}
_WIDE, _FOURIER, _HUGE = (150, 2, 1, 0, 0, 0), (48, 2, 3, 1, 20, 3), (1777, 2, 1, 0, 0, 0)
_BOTH = [
    (dict(pool_coords=None), _EINVAL),
    (dict(pool_targets=None), _EINVAL),
    (dict(index=None), _EINVAL),
    (dict(params=None), _EINVAL),
    (dict(opt_state=None), _EINVAL),
    (dict(opt=None), _EINVAL),
    (dict(loss=None), _EINVAL),
    (dict(n_pool=0), _EINVAL),
    (dict(batch=0), _EINVAL),
    (dict(n=0), _EINVAL),
    (dict(steps=-1), _EINVAL),
    (dict(step0=-1), _EINVAL),
    (dict(counts=[200, 0, 5]), _EINVAL),
    (dict(counts=[200, 201, 5]), _EINVAL),
    (dict(loss=(2, 0)), _EINVAL),                         # INR_LOSS_EXTERNAL
    (dict(loss=(0, 9)), _EINVAL),
    (dict(opt=7), _EINVAL),
    (dict(ws=None), _EINVAL),
    (dict(model=_HUGE), _EUNSUPPORTED),
    (dict(model=_HUGE, wsb=16), _EUNSUPPORTED),           # the shape is answered in front of the workspace
    (dict(model=_HUGE, n_pool=0), _EINVAL),               # ... and behind the plain arguments
    (dict(wsb=16), _EWORKSPACE),
    (dict(wsb=200 * 4 * 3 + 1024), _EWORKSPACE),          # the staging buffers fit, the step's workspace does not
    (dict(counts=[200, 3, 64], wsb=16), _EWORKSPACE),
]
_FAULTS = [("fit", f, c) for f, c in _BOTH] + [("cdn", f, c) for f, c in _BOTH] + [
    ("fit", dict(model=_WIDE, wsb=16), _EWORKSPACE),      # the layer-by-layer path's own checks
    ("fit", dict(model=_WIDE, ws=None), _EINVAL),
    ("fit", dict(model=_FOURIER, loss=(0, 1)), _EINVAL),  # several outputs: no class weights from the targets
    ("fit", dict(model=(130, 2, 1, 7, 0, 0)), _EINVAL),   # act0
    ("cdn", dict(flow_params=None), _EINVAL),
    ("cdn", dict(flow_opt_state=None), _EINVAL),
    ("cdn", dict(opt=1), _EINVAL),                        # Adamax: the flow's optimizer step is Adam's only
    ("cdn", dict(flow=(16, 3, 0)), _EUNSUPPORTED),
    ("cdn", dict(flow=(0, 2, 0)), _EUNSUPPORTED),
    ("cdn", dict(model=(130, 3, 1, 0, 0, 0)), _EUNSUPPORTED),   # the flow is 2-D only
    ("cdn", dict(model=_WIDE), _EUNSUPPORTED),            # the coupling flow runs over the fused backbone only
]


@pytest.mark.parametrize("entry,fault,code", _FAULTS, ids=[f"{e}-{'-'.join(f)}-{i}" for i, (e, f, _) in enumerate(_FAULTS)])
def test_single_fault_codes(entry, fault, code):
    from awesome_amd import _lib
    assert _ENTRY[entry](_lib.load(), _args(**fault)) == code


def test_size_query_argument_codes():
    from awesome_amd import _lib as L
    lib = L.load()
    a = _args()
    assert lib.inrfit_minibatch_workspace_bytes(a["model"], None, 200, 1) > 0
    assert lib.inrfit_minibatch_workspace_bytes(a["model"], a["flow"], 200, 1) > lib.inrfit_minibatch_workspace_bytes(a["model"], None, 200, 1)
    assert lib.inrfit_minibatch_workspace_bytes(a["model"], None, 0, 1) == _EINVAL
    assert lib.inrfit_minibatch_workspace_bytes(a["model"], None, 200, 0) == _EINVAL
    assert lib.inrfit_minibatch_workspace_bytes(_args(model=_HUGE)["model"], None, 200, 1) == _EUNSUPPORTED
    assert lib.inrfit_minibatch_workspace_bytes(None, None, 200, 1) == _EUNSUPPORTED
    assert lib.inrfit_minibatch_workspace_bytes(_args(model=_WIDE)["model"], a["flow"], 200, 1) == _EUNSUPPORTED
    assert lib.inrfit_minibatch_workspace_bytes(a["model"], _args(flow=(16, 3, 0))["flow"], 200, 1) == _EUNSUPPORTED


@pytest.mark.parametrize("model,n_images", [((130, 2, 1, 0, 0, 0), 1), ((130, 2, 1, 0, 0, 0), 2), (_WIDE, 1), (_FOURIER, 1)],
                         ids=["fused", "fused-2", "layer-by-layer", "fourier"])
def test_workspace_holds_every_count(model, n_images):
    """batch = 300: at least the staging bytes plus inrfit_workspace_bytes of an explicit grid of c points, for every c in 1..300."""
    from awesome_amd import _lib as L
    lib = L.load()
    md = _args(model=model)["model"]
    C_, O_ = md.in_features, max(md.n_out, 1)
    total = lib.inrfit_minibatch_workspace_bytes(md, None, 300, n_images)
    staging = C_ * 300 * 4 + n_images * O_ * 300 * 4
    worst = 0
    for c in range(1, 301):
        gd = L.InrGridDesc(L.INR_GRID_EXPLICIT, 0, 0, c, None, None, None, _FAKE, 0)
        own = lib.inrfit_workspace_bytes(md, gd, n_images)
        assert own > 0
        worst = max(worst, own)
    assert total >= staging + worst
    # ... and a call with exactly that much is not turned away for its workspace, whatever the counts (steps = 0: no launch follows;
    # the counts are looked at for steps entries only, so the carve is probed through the query's own bound instead)
    assert total < staging + worst + 4096   # no more than the alignment of its three parts on top


def test_dataloader_batches():
    from awesome_amd.minibatch import dataloader_batches
    for n, bs, epochs in ((150, 64, 3), (131, 64, 2), (128, 64, 2), (5, 64, 2), (7, 1, 1)):
        index, counts = dataloader_batches(n, bs, epochs, torch.Generator().manual_seed(n))
        b = min(bs, n)
        per = -(-n // b)
        assert index.dtype == torch.int32 and tuple(index.shape) == (epochs * per, b) and tuple(counts.shape) == (epochs * per,)
        assert counts.tolist() == ([b] * (n // b) + ([n % b] if n % b else [])) * epochs
        assert int(index.min()) >= 0 and int(index.max()) < n          # the padding is a valid index too
        for e in range(epochs):
            got = torch.cat([index[e * per + j, :int(counts[e * per + j])] for j in range(per)])
            assert sorted(got.tolist()) == list(range(n))
    a, _ = dataloader_batches(150, 64, 2, torch.Generator().manual_seed(1))
    b2, _ = dataloader_batches(150, 64, 2, torch.Generator().manual_seed(1))
    assert torch.equal(a, b2) and not torch.equal(a[:3], a[3:])        # seeded, and a new permutation per epoch


def test_class_balanced_batches():
    from awesome_amd.minibatch import class_balanced_batches
    labels = torch.rand(400, generator=torch.Generator().manual_seed(2))
    labels[:30] = 0.1   # few background pixels: `number` = 25 of 30-odd must still be distinct
    labels[30:] = 0.9
    idx = class_balanced_batches(labels, 9, 25, torch.Generator().manual_seed(3))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (9, 50)
    for row in idx.long():
        back, fore = row[:25], row[25:]
        assert len(set(back.tolist())) == 25 and len(set(fore.tolist())) == 25
        assert bool((labels[back] < 0.5).all()) and bool((labels[fore] >= 0.5).all())
    assert not torch.equal(idx[0], idx[1])
    with pytest.raises(ValueError):
        class_balanced_batches(labels, 2, 31, None)


def test_star_minibatches_keep_their_draw():
    """star.notebook_minibatches shares the draw: background = label > 0.5 first, the same numbers for the same seed as before."""
    from awesome_amd.star import notebook_minibatches
    labels = (torch.arange(200) % 3 == 0).float()
    idx = notebook_minibatches(labels, 70, 20, torch.Generator().manual_seed(4))
    assert tuple(idx.shape) == (70, 40) and bool((labels[idx[:, :20].long()] > 0.5).all()) and bool((labels[idx[:, 20:].long()] <= 0.5).all())
    g = torch.Generator().manual_seed(4)   # the draw written out: random keys + top-k, 64 epochs at a time, background then foreground
    back, fore = torch.nonzero(labels > 0.5).reshape(-1), torch.nonzero(labels <= 0.5).reshape(-1)
    want = torch.empty(70, 40, dtype=torch.int32)
    for s0, n in ((0, 64), (64, 6)):
        for col, pool in ((0, back), (20, fore)):
            want[s0:s0 + n, col:col + 20] = pool[torch.topk(torch.rand(n, pool.numel(), generator=g), 20, dim=1).indices].to(torch.int32)
    assert torch.equal(idx, want)


@pytest.mark.parametrize("name", MC.PARITY_CASES)
def test_restatements_are_finite_and_differ(name):
    """What the GPU parity test leans on: the float32 restatement is finite and e32 > 0 at these shapes (a bound of 4 e32 means
    something), the loop moves the parameters, and the float64 loss is a loss."""
    p64, h64, e_p, e_h, lrs = MC.references(name)
    c = MC.case(name)
    p32, h32, _ = MC.reference_loop(c, torch.float32)
    assert MC.finite(p64, h64, p32, h32)
    assert e_p > 0 and e_h > 0
    assert e_p < 1e-2 * float(p64.abs().max()) and e_h < 1e-3 * float(h64.abs().max())   # ... and is rounding, not a different loop
    start = torch.cat([x for x in MC.initial(c, "cpu") if x is not None], 1).double()
    assert float((p64 - start).abs().max()) > 1e-3
    assert bool((h64 > 0).all())


def test_cases_have_the_shapes_they_claim():
    c = MC.case("fused130")
    assert tuple(c.index.shape) == (12, 200) and c.pool_coords.shape[1] == 1440 and c.n_images == 2
    assert not torch.equal(c.pool_targets[0], c.pool_targets[1])
    assert MC.case("depth50").counts == [64, 64, 22] * 2 and MC.case("depth50").pool_coords.shape[0] == 3
    assert tuple(MC.case("fused130x2").index.shape) == (4, 67)
    assert tuple(MC.case("convexnet150").index.shape) == (5, 192)
    assert MC.case("convexnet150_loader").counts == [64, 64, 3] * 2
    assert MC.case("fourier").counts == [64, 64, 22] * 2 and tuple(MC.case("fourier").pool_targets.shape) == (1, 3, 150)
    assert tuple(MC.case("flow").index.shape) == (5, 200)
    # the plateau of depth50 changes the learning rate inside the call
    _, _, lrs = MC.reference_loop(MC.case("depth50"), torch.float64)
    assert len(set(lrs)) > 1
