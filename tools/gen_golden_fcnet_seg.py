#!/usr/bin/env python3
"""tests/golden/fcnet_rgbxy.npz from the reference classes (CPU, fp32): awesome.model.fc_net.FCNet as the runner builds it for the
convexity configs' FCNet half (depth 3, width 16, in_type rgbxy; in_chn = 3 + 2 coordinate features, out_chn 1) on pixel rows, and
the pixel-mode composite losses AwesomeLoss / AwesomeLossJoint (plain BCELoss, scribble_percentage 0.8) before and after the
extra-penalty hook.

Recorded: the seeded state_dict, rgb / feature rows, the target of the scribbled rows, the prior channel, the logits, both losses
in both phases and the network's gradient of each.  Needs the reference checkout (build container only);
`python tools/gen_golden_fcnet_seg.py`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_boundary import _install_inert_modules  # noqa: E402
from gen_golden import REF  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
N_SCR, N_RAND, P = 400, 100, 0.8     # ceil(400 (1 / 0.8 - 1)) = 100 random rows behind the scribbled ones
SEED = 211


def _import_reference():
    import types
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not present; fixtures can only be generated in the build container")
    _install_inert_modules()
    sys.path.insert(0, REF)
    pkg = types.ModuleType("awesome.model")        # skip the eager package __init__ (it pulls cv2 / torchvision)
    pkg.__path__ = [os.path.join(REF, "awesome", "model")]
    sys.modules["awesome.model"] = pkg
    import awesome.model.fc_net as fc_net
    import awesome.measures.awesome_loss as al
    import awesome.measures.awesome_loss_joint as alj
    return fc_net, al, alj


def main():
    torch.set_num_threads(1)
    fc_net, al, alj = _import_reference()
    torch.manual_seed(SEED)
    net = fc_net.FCNet(in_chn=5, out_chn=1, width=16, depth=3, in_type="rgbxy")
    g = torch.Generator().manual_seed(SEED + 1)
    n = N_SCR + N_RAND
    image = torch.rand(n, 3, generator=g)
    feat = torch.rand(n, 2, generator=g)
    target = torch.randint(0, 2, (N_SCR, 1), generator=g).float()
    prior = torch.rand(n, 1, generator=g) * 0.9 + 0.05
    rec = {f"sd/{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()}
    rec.update(seed=np.int64(SEED), image=image.numpy(), feat=feat.numpy(), target=target.numpy(), prior=prior.numpy(),
               scribble_percentage=np.float64(P))
    logits = net(image, feat)
    rec["logits"] = logits.detach().numpy()
    output = torch.cat([torch.sigmoid(logits), prior], dim=-1)[None]
    for name, make in (("awesome", lambda: al.AwesomeLoss(criterion=torch.nn.BCELoss(), alpha=1.0, scribble_percentage=P)),
                       ("joint", lambda: alj.AwesomeLossJoint(criterion=torch.nn.BCELoss(), alpha=1.0, beta=1.0, gamma=1.0,
                                                              scribble_percentage=P))):
        for phase, pen in (("before", False), ("after", True)):
            loss_fn = make()
            loss_fn.extra_penalty = pen
            if hasattr(loss_fn, "logger"):     # AwesomeLossJoint writes its terms to the runner's tensorboard logger: an inert one
                from unittest import mock
                loss_fn.logger, loss_fn.tracker = mock.MagicMock(), mock.MagicMock()
            loss = loss_fn(output, target[None])
            rec[f"{name}_{phase}_loss"] = np.float32(loss.item())
            grads = torch.autograd.grad(loss, list(net.parameters()), retain_graph=True)
            for (k, _), gr in zip(net.named_parameters(), grads):
                rec[f"{name}_{phase}_grad/{k}"] = gr.numpy().copy()
    path = os.path.join(OUT, "fcnet_rgbxy.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
