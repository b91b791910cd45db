#!/usr/bin/env python3
"""tests/golden/cnnnet_{xy,feat,featxy}.npz from the reference classes (CPU, fp32): awesome.model.cnn_net.CNNNet as the runner
builds it for the convexity configs (depth 2, width 16, kernel 3, in_type rgbxy; in_chn = 3 + feature channels, out_chn 1),
awesome.measures.gradient_penalty_loss.GradientPenaltyLoss with the configs' arguments, and the composite losses
AwesomeImageLoss / AwesomeImageLossJoint called with the step's `_input` before and after the extra-penalty hook.

Recorded per xytype: the seeded state_dict, image / features / target / prior channel, the logits, the three penalty means and the
BCE term, GradientPenaltyLoss's value, both composite losses before and after the hook, and the segmentation network's gradient of
each composite loss.  Needs the reference checkout (build container only); `python tools/gen_golden_cnnnet.py`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_boundary import _install_inert_modules  # noqa: E402
from gen_golden import REF  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
H, W = 40, 48
RAW = {"xy": 2, "feat": 4, "featxy": 4}    # feature channels: the coordinates, semantic features, both
GPL_ARGS = dict(apply_gradient_penalty=True, xygrad=0.01, rgbgrad=0.01, featgrad=0.0, noneclass=2.0)   # the CNNNet configs'


def _import_reference():
    import types
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not present; fixtures can only be generated in the build container")
    _install_inert_modules()
    sys.path.insert(0, REF)
    pkg = types.ModuleType("awesome.model")        # skip the eager package __init__ (it pulls cv2 / torchvision)
    pkg.__path__ = [os.path.join(REF, "awesome", "model")]
    sys.modules["awesome.model"] = pkg
    import awesome.model.cnn_net as cnn_net
    import awesome.measures.gradient_penalty_loss as gpl
    import awesome.measures.awesome_image_loss as ail
    import awesome.measures.awesome_image_loss_joint as ailj
    return cnn_net, gpl, ail, ailj


def gen(xytype, seed, refs):
    cnn_net, gpl, ail, ailj = refs
    torch.manual_seed(seed)
    raw = RAW[xytype]
    net = cnn_net.CNNNet(in_chn=3 + raw, out_chn=1, kernel_size=3, width=16, depth=2, in_type="rgbxy")
    g = torch.Generator().manual_seed(seed + 1)
    image = torch.rand(1, 3, H, W, generator=g).requires_grad_(True)
    feat = torch.rand(1, raw, H, W, generator=g).requires_grad_(True)
    target = torch.randint(0, 3, (1, 1, H, W), generator=g).float()
    prior = (torch.rand(1, 1, H, W, generator=g) * 0.9 + 0.05)
    inputs = [image, feat]
    rec = {f"sd/{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()}
    rec.update(seed=np.int64(seed), image=image.detach().numpy(), feat=feat.detach().numpy(), target=target.numpy(),
               prior=prior.numpy(), xytype=np.array(xytype))
    logits = net(image, feat)
    rec["logits"] = logits.detach().numpy()
    seg = torch.sigmoid(logits)
    # the penalty terms on their own (GradientPenaltyLoss's own split of the feature channels)
    gx = torch.autograd.grad(seg.sum(), [image, feat], retain_graph=True)
    rec["mean_rgb"] = np.float32(torch.mean(torch.abs(gx[0])).item())
    if xytype == "featxy":
        rec["mean_xy"] = np.float32(torch.mean(torch.abs(gx[1][:, :2])).item())
        rec["mean_feat"] = np.float32(torch.mean(torch.abs(gx[1][:, 2:])).item())
    else:
        rec["mean_xy" if xytype == "xy" else "mean_feat"] = np.float32(torch.mean(torch.abs(gx[1])).item())
    keep = target != 2.0
    rec["bce"] = np.float32(torch.nn.functional.binary_cross_entropy(seg[keep], target[keep]).item())
    crit = gpl.GradientPenaltyLoss(criterion=torch.nn.BCELoss(), xytype=xytype, **GPL_ARGS)
    rec["gpl"] = np.float32(crit(seg, target, _input=inputs).item())
    output = torch.cat([seg, prior], dim=1)
    for name, make in (("image", lambda: ail.AwesomeImageLoss(criterion=gpl.GradientPenaltyLoss(criterion=torch.nn.BCELoss(),
                                                                                              xytype=xytype, **GPL_ARGS),
                                                              prior_criterion=gpl.GradientPenaltyLoss(criterion=torch.nn.BCELoss(),
                                                                                                      noneclass=2.0),
                                                              alpha=1.0, beta=100.0, gamma=0.1)),
                       ("joint", lambda: ailj.AwesomeImageLossJoint(criterion=gpl.GradientPenaltyLoss(criterion=torch.nn.BCELoss(),
                                                                                                  xytype=xytype, **GPL_ARGS),
                                                                    alpha=1.0, beta=1.0, gamma=1.0))):
        for phase, pen in (("before", False), ("after", True)):
            loss_fn = make()
            loss_fn.extra_penalty = pen
            net.zero_grad()
            loss = loss_fn(output, target, _input=inputs)
            grads = torch.autograd.grad(loss, list(net.parameters()), retain_graph=True)
            rec[f"{name}_{phase}_loss"] = np.float32(loss.item())
            for (k, _), gr in zip(net.named_parameters(), grads):
                rec[f"{name}_{phase}_grad/{k}"] = gr.numpy().copy()
    path = os.path.join(OUT, f"cnnnet_{xytype}.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))


def main():
    torch.set_num_threads(1)
    refs = _import_reference()
    for i, xytype in enumerate(("xy", "feat", "featxy")):
        gen(xytype, 101 + i, refs)


if __name__ == "__main__":
    main()
