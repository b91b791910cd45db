#!/usr/bin/env python3
"""tests/golden/unet_eval.npz from the reference class (CPU): awesome.model.unet.UNet(in_chn=4) under a fixed seed, its BatchNorms moved
away from the identity (`perturb_batchnorm_`), in eval() on one seeded 17 x 31 item (odd at every level: every Up block pads
asymmetrically and every max-pool drops a row and a column).

Recorded (data only, no weights: the mirror reproduces them from the seed): the state_dict's keys and shapes, per tensor the float64
sum and sum of squares, the inputs, the fp32 output and the output of a .double() copy.  Needs the reference checkout (build
container only); `python tools/gen_golden_unet.py`."""
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
SEED = 307
H, W = 17, 31


def perturb_batchnorm_(net, seed: int):
    """In state_dict order: every BatchNorm weight, bias and running mean += 0.1 randn, every running variance *= 0.5 + rand."""
    g = torch.Generator().manual_seed(seed)
    bn = {name for name, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    with torch.no_grad():
        for key, t in net.state_dict().items():
            mod, _, leaf = key.rpartition(".")
            if mod not in bn:
                continue
            if leaf in ("weight", "bias", "running_mean"):
                t.add_(0.1 * torch.randn(t.shape, generator=g, dtype=torch.float32).to(t.dtype))
            elif leaf == "running_var":
                t.mul_((0.5 + torch.rand(t.shape, generator=g, dtype=torch.float32)).to(t.dtype))
    return net


def make_inputs(seed: int, h: int = H, w: int = W):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, h, w, generator=g), torch.rand(1, 1, h, w, generator=g)


def _import_reference():
    import types
    from gen_golden_boundary import _install_inert_modules
    from gen_golden import REF
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not present; fixtures can only be generated in the build container")
    _install_inert_modules()
    sys.path.insert(0, REF)
    pkg = types.ModuleType("awesome.model")        # skip the eager package __init__ (it pulls cv2 / torchvision)
    pkg.__path__ = [os.path.join(REF, "awesome", "model")]
    sys.modules["awesome.model"] = pkg
    import awesome.model.unet as unet
    return unet


def main():
    torch.set_num_threads(1)
    unet = _import_reference()
    torch.manual_seed(SEED)
    net = unet.UNet(in_chn=4)
    perturb_batchnorm_(net, SEED + 1)
    net.eval()
    image, feat = make_inputs(SEED + 2)
    sd = net.state_dict()
    rec = dict(seed=np.int64(SEED), keys=np.array(list(sd)), shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]),
               sums=np.array([float(v.double().sum()) for v in sd.values()], np.float64),
               sumsq=np.array([float((v.double() ** 2).sum()) for v in sd.values()], np.float64),
               image=image.numpy(), feat=feat.numpy())
    with torch.no_grad():
        rec["out32"] = net(image, feat).numpy()
        rec["out64"] = copy.deepcopy(net).double()(image.double(), feat.double()).numpy()
    path = os.path.join(OUT, "unet_eval.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
