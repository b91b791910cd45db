#!/usr/bin/env python3
"""One SHA-256 per output tensor of every entry point that runs through the host driver (csrc/inrfit.hip: forward_run, loss_grad_run,
fit_run, joint_step_run, joint_prior_step_run), on small shapes with fixed seeds: both backbones (fused: h = 130 with one and two
hidden layers; layer by layer: h = 136 x 1 and h = 64 x 3), without a deformation, behind the RealNVP and - fused only - behind the
coupling flow; a 24 x 20 and a ragged 23 x 19 separable grid and the latter as explicit coordinates, one and two images.  Two builds of
the library that print the same lines compute the same bits:

    INRFIT_LIB=old/libinrfit.so INRFIT_ABI_ANY=1 python tools/driver_hashes.py > old.txt
    python tools/driver_hashes.py > new.txt && diff old.txt new.txt
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import awesome_amd as A  # noqa: E402
from awesome_amd import _lib as L  # noqa: E402
from awesome_amd import flow as F  # noqa: E402
from awesome_amd import icnn as K  # noqa: E402
from awesome_amd import joint as J  # noqa: E402
from awesome_amd import rnvp as R  # noqa: E402
from awesome_amd.model import ConvexNextNet  # noqa: E402

SHAPES = [("fused", 130, 1), ("fused", 130, 2), ("wide", 136, 1), ("wide", 64, 3)]
GRIDS = [(24, 20, False), (23, 19, False), (23, 19, True)]   # width, height, as explicit coordinates [2][N] (jittered)


def show(tag, **tensors):
    for k, t in tensors.items():
        t = t.detach().contiguous().cpu()
        h = hashlib.sha256(t.numpy().tobytes()).hexdigest()[:24]
        finite = bool(torch.isfinite(t.float()).all())
        print(f"{tag} {k} {tuple(t.shape)} {h}{'' if finite else ' NONFINITE'}", flush=True)


def icnn_params(spec, n, seed, dev):
    rows = []
    for i in range(n):
        torch.manual_seed(seed + i)
        net = ConvexNextNet(n_hidden=spec.n_hidden, n_hidden_layers=spec.n_layers, in_features=spec.in_features)
        rows.append(A.pack_state_dict(spec, net.state_dict()))
    return torch.stack(rows).to(dev).contiguous()


def rnvp_params(rspec, grid, n, seed, dev):
    rows = []
    for i in range(n):
        torch.manual_seed(seed + 50 + i)
        p = R.init_rnvp_params(rspec)
        rows.append(p + 0.1 * torch.randn(p.shape))
    fp = torch.stack(rows).to(dev).contiguous()
    return R.actnorm_init(rspec, fp, grid)


def flow_params(fspec, n, seed, dev):
    torch.manual_seed(seed + 90)
    fp = 0.3 * torch.randn(n, fspec.n_params)
    fp[:, :4] = torch.eye(2).reshape(-1) + 0.05 * fp[:, :4]   # linear.weight near the identity
    return fp.to(dev).contiguous()


def targets(n, N, seed, dev):
    g = torch.Generator().manual_seed(seed + 7)
    return (torch.rand(n, N, generator=g) > 0.55).float().to(dev)


def main():
    L.load()
    dev = torch.device("cuda:0")
    pl = dict(patience=1, factor=0.5)
    for kind, h, layers in SHAPES:
        spec = A.IcnnSpec(h, 2, layers)
        rspec = R.RnvpSpec(2, 32, 4, "tanh", None, (-0.1, 0.0), (1.2, 1.0))
        fspec = F.FlowSpec(32, 2)
        for W, H, explicit in GRIDS:
            grid, N = K.Grid.linspace(W, H, dev), W * H
            if explicit:
                g = torch.Generator().manual_seed(W)
                yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
                grid = K.Grid.explicit((torch.stack([xx.reshape(-1), yy.reshape(-1)]) + 0.01 * torch.randn(2, N, generator=g)).to(dev))
            for n in (1, 2):
                seed = 1000 * h + 10 * layers + W + n
                tag = f"{kind} h{h} L{layers} {W}x{H}{'e' if explicit else ''} n{n}"
                ip, tg = icnn_params(spec, n, seed, dev), targets(n, N, seed, dev)
                fp = rnvp_params(rspec, grid, n, seed, dev)
                # ---- the plain ICNN
                show(tag + " forward", logits=K.forward(spec, ip, grid))
                lo, gr = K.loss_grad(spec, ip, grid, tg, "bce", "sssdms")
                show(tag + " loss_grad", loss=lo, grads=gr)
                gr, dco = K.backward(spec, ip, grid, tg - 0.5, want_dcoords=True)
                show(tag + " backward", grads=gr, dcoords=dco)
                for gate in (False, True):
                    r = K.fit(spec, ip.clone(), grid, tg, 3, lr=4e-3, optimizer="adamax", plateau=pl, gate_logits=gate)
                    show(tag + f" fit gate{int(gate)}", params=r.params, opt=r.opt_state, hist=r.loss_hist, logits=r.logits, status=r.status)
                # ---- behind the RealNVP
                show(tag + " pcn_forward", logits=R.pcn_forward(spec, rspec, ip, fp, grid))
                lo, gi, gf = R.pcn_loss_grad(spec, rspec, ip, fp, grid, tg, "bce", "sssdms")
                show(tag + " pcn_loss_grad", loss=lo, gi=gi, gf=gf)
                for gate in (False, True):
                    r = R.pcn_fit(spec, rspec, ip.clone(), fp.clone(), grid, tg, 3, lr=4e-3, plateau=pl, gate_logits=gate)
                    show(tag + f" pcn_fit gate{int(gate)}", ip=r.icnn_params, fp=r.flow_params, iopt=r.icnn_opt_state, fopt=r.flow_opt_state,
                         hist=r.loss_hist, logits=r.logits, status=r.status)
                # ---- behind the coupling flow (fused backbone only)
                if kind == "fused":
                    cp = flow_params(fspec, n, seed, dev)
                    show(tag + " cdn_forward", logits=F.cdn_forward(spec, fspec, ip, cp, grid))
                    lo, gi, gf = F.cdn_loss_grad(spec, fspec, ip, cp, grid, tg)
                    show(tag + " cdn_loss_grad", loss=lo, gi=gi, gf=gf)
                    r = F.cdn_fit(spec, fspec, ip.clone(), cp.clone(), grid, tg, 3, plateau=pl)
                    show(tag + " cdn_fit", ip=r.icnn_params, fp=r.flow_params, iopt=r.icnn_opt_state, fopt=r.flow_opt_state, hist=r.loss_hist,
                         logits=r.logits, status=r.status)
                if n != 1:
                    continue
                # ---- the joint steps (one image)
                g = torch.Generator().manual_seed(seed + 3)
                seg = torch.rand(N, generator=g).to(dev)
                wide = kind == "wide"
                descs = {"fbms": J.joint_desc(), "image": J.joint_desc(form=L.JOINT_AWESOME_IMAGE),
                         "image_pen": J.joint_desc(form=L.JOINT_AWESOME_IMAGE, extra_penalty=True, gamma=0.7, alpha=0.5, beta=0.3)}
                for name, desc in descs.items():
                    p, o = ip[0].clone(), K.new_opt_state(spec, 1, dev)[0]
                    r = (J.wide_joint_step if wide else J.joint_step)(spec, p, o, grid, seg, tg[0], desc, 1, 2e-3)
                    show(tag + f" joint_step {name}", params=p, opt=o, loss=r.loss, dseg=r.dseg, logits=r.prior_logits, status=r.status)
                    p, f_, o, fo = ip.clone(), fp.clone(), K.new_opt_state(spec, 1, dev), torch.zeros(1, 2 * rspec.n_params, device=dev)
                    r = (J.pcn_wide_joint_step if wide else J.pcn_joint_step)(spec, rspec, p, f_, o, fo, grid, seg, tg[0], desc, 1, 2e-3,
                                                                              flow_weight_decay=1e-5)
                    show(tag + f" pcn_joint_step {name}", ip=p, fp=f_, iopt=o, fopt=fo, loss=r.loss, dseg=r.dseg, logits=r.prior_logits,
                         status=r.status)
                    if not wide:
                        p, f_, o, fo = ip.clone(), flow_params(fspec, 1, seed, dev), K.new_opt_state(spec, 1, dev), torch.zeros(1, 2 * fspec.n_params, device=dev)
                        r = J.cdn_joint_step(spec, fspec, p, f_, o, fo, grid, seg, tg[0], desc, 1, 2e-3)
                        show(tag + f" cdn_joint_step {name}", ip=p, fp=f_, iopt=o, fopt=fo, loss=r.loss, dseg=r.dseg, logits=r.prior_logits,
                             status=r.status)
                priors = {"data": J.joint_prior_desc(),
                          "masked_soft": J.joint_prior_desc(weight_mode="sssdms", noneclass=2.0, data_count=N - 40, c_data=0.8,
                                                            align_rule=L.ALIGN_SOFT, beta=0.4, align_begin=17)}
                for name, desc in priors.items():
                    p, o = ip[0].clone(), K.new_opt_state(spec, 1, dev)[0]
                    t = tg[0, :desc.data_count].clone() if desc.data_count else tg[0]
                    if desc.data_count:
                        t[::9] = 2.0   # the none class
                    r = (J.wide_joint_prior_step if wide else J.joint_prior_step)(spec, p, o, grid, seg, t, desc, 1, 2e-3,
                                                                                  seg_term=torch.tensor([0.25], device=dev))
                    show(tag + f" joint_prior_step {name}", params=p, opt=o, loss=r.loss, dseg=r.dseg, logits=r.prior_logits, status=r.status)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
