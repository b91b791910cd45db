#!/usr/bin/env python3
"""tests/golden/unet_train.npz from the reference class (CPU, float64): one training-mode forward and backward of
awesome.model.unet.UNet at channel width 4 on one seeded 37 x 50 item.

The reference class has its widths written out (64 .. 512); its own sub-modules (InConv, Down, Up, OutConv) are assembled here at
width 4 under the same names and in the same order on an instance made with decoding=True, and its own forward runs them.  The
BatchNorms are moved away from the identity (gen_golden_unet.perturb_batchnorm_).

Recorded (data only): the state_dict the step started from (float32 values), the inputs, dlogits, and in float64 the logits, every
parameter's gradient in parameters() order and the updated running statistics.  It pins that awesome_amd.model.UNet in train() is the
reference's.  Needs the reference checkout (build container only); `python tools/gen_golden_unet_train.py`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_golden_unet import OUT, _import_reference, make_inputs, perturb_batchnorm_   # noqa: E402

SEED = 307
H, W, BASE = 37, 50, 4


def reference_net(unet, base: int, in_chn: int = 4, out_chn: int = 1):
    b = base
    net = unet.UNet(decoding=True)
    net.inc = unet.InConv(in_chn, b)
    net.down1 = unet.Down(b, 2 * b)
    net.down2 = unet.Down(2 * b, 4 * b)
    net.down3 = unet.Down(4 * b, 8 * b)
    net.down4 = unet.Down(8 * b, 8 * b)
    net.up1 = unet.Up(16 * b, 4 * b)
    net.up2 = unet.Up(8 * b, 2 * b)
    net.up3 = unet.Up(4 * b, b)
    net.up4 = unet.Up(2 * b, b)
    net.outc = unet.OutConv(b, out_chn)
    return net


def main():
    torch.set_num_threads(1)
    unet = _import_reference()
    torch.manual_seed(SEED)
    net = reference_net(unet, BASE)
    perturb_batchnorm_(net, SEED + 1)
    image, feat = make_inputs(SEED + 2, H, W)
    dlogits = torch.randn(1, 1, H, W, generator=torch.Generator().manual_seed(SEED + 9))
    rec = dict(seed=np.int64(SEED), base_width=np.int64(BASE), image=image.numpy(), feat=feat.numpy(), dlogits=dlogits.numpy())
    for k, v in net.state_dict().items():
        rec["state/" + k] = v.numpy().copy()
    net = net.double().train()
    logits = net(image.double(), feat.double())
    logits.backward(dlogits.double())
    rec["logits"] = logits.detach().numpy()
    rec["param_names"] = np.array([n for n, _ in net.named_parameters()])
    for n, p in net.named_parameters():
        rec["grad/" + n] = p.grad.numpy()
    for k, v in net.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            rec["after/" + k] = v.numpy().copy()
    path = os.path.join(OUT, "unet_train.npz")
    np.savez_compressed(path, **rec)
    with open(os.path.join(OUT, "unet_train.txt"), "w") as f:
        f.write("unet_train.npz: written by tools/gen_golden_unet_train.py (seed %d).\n"
                "The reference's awesome.model.unet sub-modules assembled at channel width %d, one training-mode forward and backward in\n"
                "float64 on the CPU on a seeded %d x %d item: starting state_dict, inputs, dlogits, logits, every parameter's gradient, the\n"
                "updated running statistics.  Data only.\n" % (SEED, BASE, H, W))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
