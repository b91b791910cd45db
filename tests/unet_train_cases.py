"""Cases and float64 references for the tests of the UNet's training step (tests/test_gpu_unet_train.py; their CPU side:
tests/test_unet_train_host.py).  Nothing here touches the GPU or the HIP library.

Yardstick: the same module's .double() copy, run by torch on the CPU in train() mode with the same dlogits.  For every compared tensor
(logits, each parameter's gradient, each updated running mean and variance) e_torch is the error of torch's own fp32 CPU pass against
it, and the bar is the one of tests/test_gpu_unet.py, for the same reason (a different but equally long summation order):

    max|x - f64| <= 4 e_torch + 1e-6 max|f64|

The biases of the 18 convolutions in front of a BatchNorm have a gradient that is zero in exact arithmetic (the normalisation removes
the mean), so their float64 gradient is rounding noise: for them e_torch and the floor come from the same convolution's WEIGHT gradient.

Conditioning.  A ReLU input or a max-pool tie that changes sides between fp32 and float64 moves a gradient by one whole pixel's
contribution, which no rounding bar covers.  So a case is accepted only if, with e_l = max|z32 - z64| over layer l's pre-ReLU values
between torch's two CPU passes,

    no pre-ReLU value has |z64| <= 4 e_l, and
    no pool window with a positive maximum has its two largest values within 4 e_l of each other.

`build` searches at most MAX_SEEDS seeds and fails loudly if none qualifies.  The full-width case cannot be found by search (tens of
offenders among 1.3 M pre-activations per seed); its BatchNorms get a small |gamma| and beta = +-1 per channel instead, so every
channel is entirely on or entirely off: no ReLU kinks by construction, while the products run at their full M, N and K.  The pool
condition is checked for it like for the others.  These are properties of the inputs which torch's two CPU passes establish; no result
of the code under test enters."""
import copy
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MARGIN = 4.0
MAX_SEEDS = 64
FIRST_SEED = 307
POOLED = (1, 3, 5, 7)       # the convolutions (state_dict order) whose ReLU'd output a max-pool reads

# name -> h, w, base_width, out_chn, strip_points, on/off BatchNorms
CASES = {
    "32x32-b4": (32, 32, 4, 1, 0, False),          # bottom level 2 x 2; fewer channels than one gather group
    "16x32-b4": (16, 32, 4, 1, 0, False),          # bottom level 1 x 2: the smallest shape torch accepts
    "37x50-b4": (37, 50, 4, 1, 0, False),          # odd at several levels: asymmetric pads, the pool drops rows and columns
    "37x50-b8": (37, 50, 8, 1, 0, False),
    "37x50-b4-o3": (37, 50, 4, 3, 0, False),       # several output channels
    "40x56-b8-s512": (40, 56, 8, 1, 512, False),   # strips end inside image rows, several weight-gradient partials
    "64x48-b64-onoff": (64, 48, 64, 1, 0, True),   # full widths, split-K levels, per-layer strips that differ
}


def bn_layers(net):
    out = []
    for blk in net.blocks():
        out += [blk.conv[1], blk.conv[4]]
    return out


def onoff_batchnorm_(net, seed):
    """gamma = +-(0.1 .. 0.2), beta = +-1 per channel: a channel is on or off (almost) as a whole, so next to no value lies near the
    kink.  Neighbouring pixels of an 'on' channel differ by about |gamma| / 10, and among the 60 000 pool windows of 'on' channels
    about ten would have their two largest values within 4 e_l (measured); so in the four maps a max-pool reads only every eighth
    channel is on (two thirds elsewhere), which leaves one or two such windows per seed - few enough for the seed search."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for l, bn in enumerate(bn_layers(net)):
            n = bn.weight.numel()
            sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
            bn.weight.copy_(sign * (0.1 + 0.1 * torch.rand(n, generator=g)))
            bn.bias.copy_(torch.where(torch.rand(n, generator=g) < (0.125 if l in POOLED else 0.65), 1.0, -1.0))
    return net


def make_net(base, out_chn, seed, onoff=False):
    import gen_golden_unet as G
    from awesome_amd.model import UNet
    torch.manual_seed(seed)
    net = UNet(in_chn=4, out_chn=out_chn, base_width=base)
    G.perturb_batchnorm_(net, seed + 1)
    if onoff:
        onoff_batchnorm_(net, seed + 3)
    return net.train()


def make_inputs(h, w, out_chn, seed):
    import gen_golden_unet as G
    image, feat = G.make_inputs(seed, h, w)
    g = torch.Generator().manual_seed(seed + 7)
    return image, feat, torch.randn(1, out_chn, h, w, generator=g)


def run_torch(net, image, feat, dlogits, dtype, backward=True, grad_hook=None):
    """One training-mode forward (and backward from dlogits) of a copy of `net` in `dtype` on the CPU.
    -> dict: logits, grads (parameters() order), means / vars (the updated running statistics), z (the 18 pre-ReLU maps).
    grad_hook: (layer index, function on the gradient at that layer's pre-ReLU map) - to build a deliberately wrong gradient."""
    m = copy.deepcopy(net).to(dtype).train()
    for mod in m.modules():
        if isinstance(mod, nn.ReLU):
            mod.inplace = False
    z, handles = [], []
    for i, bn in enumerate(bn_layers(m)):
        def hook(_mod, _inp, out, i=i):
            z.append(out.detach().clone())
            if grad_hook is not None and grad_hook[0] == i:
                out.register_hook(grad_hook[1])
        handles.append(bn.register_forward_hook(hook))
    with torch.enable_grad():
        logits = m.forward_torch(image.to(dtype), feat.to(dtype))
        if backward:
            logits.backward(dlogits.to(dtype))
    for h in handles:
        h.remove()
    bns = bn_layers(m)
    return dict(logits=logits.detach(), grads=[p.grad for p in m.parameters()] if backward else None,
                means=[bn.running_mean.clone() for bn in bns], vars=[bn.running_var.clone() for bn in bns], z=z)


def offenders(z32, z64):
    """(ReLU kinks, pool ties) per the module docstring, counted over all layers."""
    kinks = ties = 0
    for l, (a, b) in enumerate(zip(z32, z64)):
        e = float((a.double() - b).abs().max())
        kinks += int((b.abs() <= MARGIN * e).sum())
        if l in POOLED:
            r = torch.relu(b)
            H, W = r.shape[-2] // 2 * 2, r.shape[-1] // 2 * 2
            win = r[..., :H, :W].unfold(2, 2, 2).unfold(3, 2, 2).reshape(*r.shape[:2], H // 2, W // 2, 4)
            top = win.topk(2, dim=-1).values
            ties += int(((top[..., 0] > 0) & (top[..., 0] - top[..., 1] <= MARGIN * e)).sum())
    return kinks, ties


_built = {}


def build(name):
    """The case's CPU module (train mode), inputs, dlogits and both CPU references, computed once and shared; treat as read-only."""
    if name in _built:
        return _built[name]
    h, w, base, out_chn, strip, onoff = CASES[name]
    tried = []
    for seed in range(FIRST_SEED, FIRST_SEED + MAX_SEEDS):
        net = make_net(base, out_chn, seed, onoff)
        image, feat, dlogits = make_inputs(h, w, out_chn, seed + 2)
        f32 = run_torch(net, image, feat, dlogits, torch.float32, backward=False)
        f64 = run_torch(net, image, feat, dlogits, torch.float64, backward=False)
        bad = offenders(f32["z"], f64["z"])
        tried.append((seed, bad))
        if bad == (0, 0):
            break
    else:
        raise AssertionError(f"unet_train_cases: no seed of {MAX_SEEDS} gives a conditioned case {name}: (seed, (kinks, ties)) {tried}")
    case = dict(name=name, seed=seed, net=net, image=image, feat=feat, dlogits=dlogits, strip=strip,
                f32=run_torch(net, image, feat, dlogits, torch.float32), f64=run_torch(net, image, feat, dlogits, torch.float64))
    _built[name] = case
    return case


def tensors(res, net):
    """[(name, tensor, index of the tensor that lends e_torch and the floor, or None)] of a run_torch-shaped result."""
    names = [n for n, _ in net.named_parameters()]
    out = [("logits", res["logits"], None)]
    for i, (n, g) in enumerate(zip(names, res["grads"])):
        # parameters() order: per convolution weight, bias, gamma, beta - the bias borrows from the weight in front of it
        lend = len(out) - 1 if (i % 4 == 1 and i < 72) else None
        out.append(("grad " + n, g, lend))
    out += [(f"running_mean {i}", t, None) for i, t in enumerate(res["means"])]
    out += [(f"running_var {i}", t, None) for i, t in enumerate(res["vars"])]
    return out


def compare(got, case, what, collect=None):
    """Assert the bar for every tensor of `got` (a run_torch-shaped dict, any device / dtype); -> the largest e / e_torch ratio seen
    among the tensors whose e_torch is not zero.  Every figure is printed before it is asserted."""
    net = case["net"]
    t64, t32, tg = tensors(case["f64"], net), tensors(case["f32"], net), tensors(got, net)
    assert len(tg) == len(t64)
    worst, worst_name, nearest, nearest_name, failures = 0.0, "-", 0.0, "-", []
    for k, ((name, ref, lend), (_, f32, _), (_, x, _)) in enumerate(zip(t64, t32, tg)):
        x = x.detach().cpu().double().reshape(ref.shape)
        assert bool(torch.isfinite(x).all()), f"{what}: {name} is not finite"
        src = k if lend is None else lend
        e_torch = float((t32[src][1].double() - t64[src][1]).abs().max())
        scale = float(t64[src][1].abs().max())
        e = float((x - ref).abs().max())
        bar = 4 * e_torch + 1e-6 * scale
        if e_torch > 0 and e / e_torch > worst:
            worst, worst_name = e / e_torch, name
        if bar > 0 and e / bar > nearest:
            nearest, nearest_name = e / bar, name
        if collect is not None:
            collect.append((name, e, e_torch, bar))
        if not e <= bar:
            failures.append(f"{name}: e {e:.3e}  e_torch {e_torch:.3e}  bar {bar:.3e}  max|f64| {scale:.3e}")
    print(f"[unet train parity] {what}: worst e / e_torch {worst:.2f} ({worst_name}), worst e / bar {nearest:.2f} ({nearest_name}), "
          f"{len(failures)} of {len(tg)} tensors over the bar")
    assert not failures, what + ":\n" + "\n".join(failures)
    return worst
