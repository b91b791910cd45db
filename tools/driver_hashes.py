#!/usr/bin/env python3
"""One SHA-256 per output tensor of every entry point that runs through the host driver (csrc/inrfit.hip: forward_run, loss_grad_run,
fit_run, joint_step_run, joint_prior_step_run), on small shapes with fixed seeds: both backbones (fused: h = 130 with one and two
hidden layers; layer by layer: h = 136 x 1 and h = 64 x 3), without a deformation, behind the RealNVP and - fused only - behind the
coupling flow; a 24 x 20 and a ragged 23 x 19 separable grid and the latter as explicit coordinates, one and two images.  Behind
them the wrappers with loops of their own (`extras`): the pixel-minibatch fits, the pose fits (h = 130 and the layer-by-layer 150),
the star prior (minibatch and dense, Adam and Adamax), the flow's identity pre-fit and the two sequence fits, on a 96-point pool with batches of 32 and 17.  Two builds of the
library - or two versions of the Python binding over one build - that print the same lines compute the same bits:

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
from awesome_amd import minibatch as MB  # noqa: E402
from awesome_amd import rnvp as R  # noqa: E402
from awesome_amd import star as ST  # noqa: E402
from awesome_amd import symmetric as SY  # noqa: E402
from awesome_amd.model import ConvexNextNet  # noqa: E402

SHAPES = [("fused", 130, 1), ("fused", 130, 2), ("wide", 136, 1), ("wide", 64, 3)]
GRIDS = [(24, 20, False), (23, 19, False), (23, 19, True)]   # width, height, as explicit coordinates [2][N] (jittered)


def show(tag, **tensors):
    for k, t in tensors.items():
        t = t.detach().contiguous().cpu()
        h = hashlib.sha256(t.numpy().tobytes()).hexdigest()[:24]
        finite = bool(torch.isfinite(t.float()).all())
        print(f"{tag} {k} {tuple(t.shape)} {h}{'' if finite else ' NONFINITE'}", flush=True)


POOL, TABLES = 96, ((6, 32), (5, 17))   # pool points; (steps, batch) of the two index tables


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


def tables(seed):
    """[steps, batch] int32 pool indices; the second table ragged (the last two counts short)."""
    g = torch.Generator().manual_seed(seed)
    for steps, batch in TABLES:
        index = torch.stack([torch.randperm(POOL, generator=g)[:batch] for _ in range(steps)]).to(torch.int32)
        yield index, (None if batch == 32 else [batch] * (steps - 2) + [batch - 4, 5])


def extras(dev, pl):
    g = torch.Generator().manual_seed(5)
    pool = torch.rand(2, POOL, generator=g).to(dev)
    W, H = 23, 19
    grid, N = K.Grid.linspace(W, H, dev), W * H
    rspec, fspec = R.RnvpSpec(2, 32, 4, "tanh", None, (-0.1, 0.0), (1.2, 1.0)), F.FlowSpec(32, 2)
    # ---- pixel-minibatch fits: fused, layer by layer, behind the coupling flow
    for kind, h, layers in (("fused", 130, 1), ("wide", 136, 1)):
        spec = A.IcnnSpec(h, 2, layers)
        for n in (1, 2):
            ip, tg = icnn_params(spec, n, 7000 + h + n, dev), targets(n, POOL, h + n, dev)
            for index, counts in tables(h + n):
                tag = f"{kind} h{h} L{layers} pool{POOL} b{index.shape[1]} n{n}"
                for plateau in (None, pl):
                    r = MB.fit_minibatch(spec, ip.clone(), pool, tg, index, counts, lr=4e-3, optimizer="adamax", plateau=plateau)
                    show(tag + f" fit_minibatch pl{int(plateau is not None)}", params=r.params, opt=r.opt_state, hist=r.loss_hist, status=r.status)
                if kind == "fused":
                    r = MB.cdn_fit_minibatch(spec, fspec, ip.clone(), flow_params(fspec, n, h + n, dev), pool, tg, index, counts, plateau=pl)
                    show(tag + " cdn_fit_minibatch", ip=r.icnn_params, fp=r.flow_params, iopt=r.icnn_opt_state, fopt=r.flow_opt_state,
                         hist=r.loss_hist, status=r.status)
    # ---- the pose fits: fused and layer by layer
    for h in (130, 150):
        spec = A.IcnnSpec(h, 3, 1)
        for n in (1, 2):
            ip = icnn_params(spec, n, 8000 + h + n, dev)
            pose = (torch.tensor([0.45, 0.55, 0.3]) + 0.05 * torch.randn(n, 3, generator=g)).to(dev)
            tag = f"sym h{h} n{n}"
            show(tag + " sym_forward", logits=SY.sym_forward(spec, ip, pose, grid))
            lo, gn, gp = SY.sym_loss_grad(spec, ip, pose, grid, targets(n, N, h, dev))
            show(tag + " sym_loss_grad", loss=lo, grads=gn, gpose=gp)
            r = SY.sym_fit(spec, ip.clone(), pose.clone(), grid, targets(n, N, h, dev), 5, lr=4e-3, symmetry_from_step=2, plateau=pl)
            show(tag + " sym_fit", params=r.params, pose=r.pose, opt=r.opt_state, popt=r.pose_opt_state, hist=r.loss_hist, status=r.status)
            for index, counts in tables(h + n):
                r = SY.sym_fit_minibatch(spec, ip.clone(), pose.clone(), pool, targets(n, POOL, h, dev), index, counts, lr=4e-3,
                                         symmetry_from_step=2)
                show(tag + f" sym_fit_minibatch b{index.shape[1]}", params=r.params, pose=r.pose, opt=r.opt_state, popt=r.pose_opt_state,
                     hist=r.loss_hist, status=r.status)
    # ---- the star prior
    sspec = ST.StarSpec(32)
    torch.manual_seed(11)
    sp = (0.3 * torch.randn(sspec.n_params)).to(dev)
    labels = targets(1, POOL, 3, dev)[0]
    coords = pool.t().contiguous()
    show("star forward", logits=ST.star_forward(sspec, sp, coords))
    lo, gr = ST.star_loss_grad(sspec, sp, coords, labels)
    show("star loss_grad", loss=lo, grads=gr)
    for index, _ in tables(13):
        r = ST.star_fit(sspec, sp.clone(), coords, labels, index, step0=0, offset_first_step=3)
        show(f"star fit b{index.shape[1]}", params=r.params, opt=r.opt_state, hist=r.loss_hist)
    # ---- ... and its dense many-image form on the whole pool (the centre steps from step 3 on)
    gs = torch.Generator().manual_seed(12)
    for n in (1, 2):
        dp, dt = (0.3 * torch.randn(n, sspec.n_params, generator=gs)).to(dev), targets(n, POOL, 20 + n, dev)
        lo, gr = ST.star_loss_grad_dense(sspec, dp, coords, dt)
        show(f"star n{n} loss_grad_dense", loss=lo, grads=gr)
        for optimizer in ("adam", "adamax"):
            r = ST.star_fit_dense(sspec, dp.clone(), coords, dt, 5, optimizer=optimizer, plateau=pl, offset_first_step=3)
            show(f"star n{n} fit_dense {optimizer}", params=r.params, opt=r.opt_state, hist=r.loss_hist, logits=r.logits, status=r.status)
    # ---- the flow's identity pre-fit and the sequence fits (T = 5 frames of the pool, batches of 2: the last one short)
    for n in (1, 2):
        fp = rnvp_params(rspec, grid, n, 9000 + n, dev)
        hist, opt = R.fit_identity(rspec, fp, grid, steps=5)
        show(f"fit_identity n{n}", fp=fp, opt=opt, hist=hist)
    T, ispec = 5, A.IcnnSpec(130, 2, 1)
    frames = torch.rand(T, 2, POOL, generator=g).to(dev)
    ftargets = targets(T, POOL, 17, dev)
    orders = torch.stack([torch.randperm(T, generator=g) for _ in range(3)])
    for plateau in (None, pl):
        ip, fp = icnn_params(ispec, 1, 9100, dev), rnvp_params(rspec, K.Grid.explicit(frames[0]), 1, 9100, dev)
        r = R.pcn_fit_sequence(ispec, rspec, ip, fp, frames, ftargets, orders, 2, lr=4e-3, plateau=plateau)
        show(f"pcn_fit_sequence pl{int(plateau is not None)}", ip=r.icnn_params, fp=r.flow_params, iopt=r.icnn_opt_state, fopt=r.flow_opt_state,
             epoch_loss=r.epoch_loss, status=r.status)
    fp = rnvp_params(rspec, K.Grid.explicit(frames[0]), 1, 9200, dev)
    hist, opt = R.fit_identity_sequence(rspec, fp, frames, orders, 2)
    show("fit_identity_sequence", fp=fp, opt=opt, hist=hist)


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
    extras(dev, pl)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
