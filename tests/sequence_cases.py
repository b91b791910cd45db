"""Shared pieces of tests/test_sequence_host.py and tests/test_gpu_sequence.py (sequence pretraining: mini-batch epochs and pre-fits
in one device call).  Shapes: F = 6 flows of 32 hidden units, C = 3, as tests/test_gpu_rnvp.py::test_fit_sequence_minibatches builds
them; T = 5 frames of 7 x 9 (HW = 63: odd - the element-wise gather, unaligned frame starts, a last batch of one frame at batch
size 2) and T = 4 frames of 8 x 10 (HW = 80: the 16-byte gather)."""
import ctypes as C
from typing import Dict, List, Sequence, Tuple

import torch

from oracle import inr_oracle as O

FLOWS, HID, CH = 6, 32, 3
SHAPES = {"t5_7x9": (5, 7, 9), "t4_8x10": (4, 8, 10)}
ICNNS = {"h130_l1": (130, 1), "h32_l2": (32, 2)}


def dataloader_orders(T: int, batch_size: int, epochs: int, one_loader: bool) -> torch.Tensor:
    """What a real DataLoader(TensorDataset(arange(T)), batch_size, shuffle=True) yields, under the global RNG: one loader iterated
    `epochs` times (the identity pre-fit) or a new loader per epoch (the main loop)."""
    from torch.utils.data import DataLoader, TensorDataset
    ds = TensorDataset(torch.arange(T))
    loader = DataLoader(ds, batch_size=batch_size, shuffle=True)
    rows = []
    for _ in range(epochs):
        if not one_loader:
            loader = DataLoader(ds, batch_size=batch_size, shuffle=True)
        rows.append(torch.cat([b[0] for b in loader]))
    return torch.stack(rows)


def identity_orders(epochs: int, T: int) -> torch.Tensor:
    return torch.arange(T).repeat(epochs, 1)


def shuffled_orders(epochs: int, T: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(T, generator=g) for _ in range(epochs)])


def make_model(dev, icnn: str, seed: int = 2):
    """A PathConnectedNet with non-trivial couplings and ActNorm marked initialised (s = t = 0), and its start state."""
    from awesome_amd.model import real_nvp_path_connected_net
    h, layers = ICNNS[icnn]
    torch.manual_seed(seed)
    m = real_nvp_path_connected_net(channels=CH, hidden_units=HID, flow_n_flows=FLOWS, flow_output_fn="tanh",
                                    convex_net_hidden_units=h, convex_net_hidden_layers=layers).to(dev)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith("net.2.weight") or k.endswith("net.2.bias"):
                p.copy_(0.1 * torch.randn_like(p))
        for a in m.flow_net.net.network.flows:
            if hasattr(a, "data_dep_init_done"):
                a.data_dep_init_done.fill_(1.0)
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


def oracle_state(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The float parameters of a module state, on the CPU, as the oracle's loops take them."""
    return {k: v.detach().cpu().clone() for k, v in state.items()
            if v.dtype == torch.float32 and not k.startswith("flow_net.norm") and not k.endswith("data_dep_init_done")}


def frames(shape: str) -> Tuple[List[torch.Tensor], List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """rows[t] (HW, 3), unaries[t] (HW, 1) for the oracle; coords (T, 3, HW), unaries (T, HW) for the module (CPU tensors)."""
    T, H, W = SHAPES[shape]
    grids = [O.positional_grid(W, H, float(t), float(T - 1)) for t in range(T)]
    rows = [O.pixelize(g[None]) for g in grids]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    uns = [(((yy - H // 2) ** 2 + (xx - 3 - t) ** 2) > 6).float().reshape(-1, 1) for t in range(T)]
    return rows, uns, torch.stack([g.reshape(3, -1) for g in grids]), torch.stack([u.reshape(-1) for u in uns])


def fit_flow_identity_minibatch(sd0: Dict[str, torch.Tensor], frame_rows: Sequence[torch.Tensor], orders: torch.Tensor,
                                batch_size: int, masks: torch.Tensor, vmin: torch.Tensor, vmax: torch.Tensor, lr: float = 1e-2,
                                weight_decay: float = 1e-5, new_min: float = -1.0, new_max: float = 1.0,
                                actnorm_init: bool = False) -> Tuple[Dict[str, torch.Tensor], List[float]]:
    """The reference's mini-batched learn_flow_identity (awesome/model/path_connected_net.py:200-236) from the oracle's parts, as
    O.fit_flow_identity composes them: per epoch the batches of `orders[e]`, one Adamax step each on SE('mean')(flow_net(x), x);
    the history holds every epoch's LAST batch loss.  actnorm_init: the data-dependent init on the first batch drawn."""
    T = len(frame_rows)
    sd = {k: v.detach().clone() for k, v in sd0.items()}
    if actnorm_init:
        first = torch.cat([frame_rows[t] for t in orders[0][:batch_size].tolist()], 0)
        with torch.no_grad():
            O.rnvp_flow_forward(sd, O.minmax(first, vmin.view(1, -1), vmax.view(1, -1), new_min, new_max), masks, actnorm_init=True)
    p = {k: v.detach().clone().requires_grad_(k.startswith("flow_net.")) for k, v in sd.items()}
    keys = [k for k in p if k.startswith("flow_net.")]
    sub = {k: p[k] for k in keys}
    st = O.AdamState(sub)
    hist: List[float] = []
    for order in orders.tolist():
        last = float("nan")
        for i in range(0, T, batch_size):
            rows = torch.cat([frame_rows[t] for t in order[i:i + batch_size]], 0)
            for k in keys:
                p[k].grad = None
            z = O.minmax(rows, vmin.view(1, -1), vmax.view(1, -1), new_min, new_max)
            z = O.rnvp_flow_forward(p, z, masks)
            y = O.minmax(z, new_min, new_max, vmin.view(1, -1), vmax.view(1, -1))
            loss = ((rows - y) ** 2).mean()
            loss.backward()
            O.adamax_step(sub, {k: p[k].grad for k in keys}, st, lr, weight_decay=weight_decay)
            last = float(loss.item())
        hist.append(last)
    return {k: v.detach() for k, v in p.items()}, hist


# ---- the two entry points' argument lists, for the single-fault table (host only: nothing here touches a device) --------------------
def abi_descs(h: int = 130, layers: int = 1):
    from awesome_amd import _lib as L
    md = L.InrModelDesc(L.INR_MODEL_ICNN, h, CH, layers, 0, 0.0, 0, 0)
    rd = L.InrRnvpDesc()
    rd.channels, rd.hidden_units, rd.n_flows, rd.output_fn, rd.output_scale = CH, HID, FLOWS, 1, 1.0
    for c in range(CH):
        rd.vmin[c], rd.vmax[c] = 0.0, 1.0
    rd.new_min, rd.new_max = -1.0, 1.0
    for f in range(FLOWS):
        rd.masks[f] = 1 + f % 6
    ld = L.InrLossDesc(L.INR_LOSS_SE, L.INR_WEIGHT_NONE, 1.0, 0.0, 0.0)
    od = L.InrOptDesc(L.INR_OPT_ADAMAX, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 0, 0.5, 1e-4, 0.0, 1e-8, 0, 0, 0)
    return md, rd, ld, od


FAKE = 0x1000   # a non-null "device pointer" no call may follow: every fault below is answered on the host


def sequence_args(T: int = 5, HW: int = 63, batch: int = 2, epochs: int = 2, order="identity", **over):
    """order: rows of frame ids, "identity", or None (the null-pointer fault)."""
    md, rd, ld, od = abi_descs()
    rows = [list(range(T))] * max(epochs, 0) if isinstance(order, str) else order
    flat = [int(v) for r in (rows or []) for v in r]
    a = dict(model=C.byref(md), rnvp=C.byref(rd), ip=FAKE, fp=FAKE, iopt=FAKE, fopt=FAKE, coords=FAKE, targets=FAKE,
             order=(C.c_int32 * max(len(flat), 1))(*flat) if rows is not None else None, T=T, HW=HW, batch=batch, epochs=epochs,
             loss=C.byref(ld), opt=C.byref(od),
             schedule=None, wd=1e-5, step0=0, epoch_loss=FAKE, status=FAKE, ws=FAKE, ws_bytes=1 << 40, stream=None)
    a.update(over)
    a["_keep"] = (md, rd, ld, od)
    return a


def call_pcn_sequence(lib, a) -> int:
    return lib.inrfit_pcn_fit_sequence(a["model"], a["rnvp"], a["ip"], a["fp"], a["iopt"], a["fopt"], a["coords"], a["targets"], a["order"],
                                       a["T"], a["HW"], a["batch"], a["epochs"], a["loss"], a["opt"], a["schedule"], a["wd"], a["step0"],
                                       a["epoch_loss"], a["status"], a["ws"], a["ws_bytes"], a["stream"])


def call_identity_sequence(lib, a) -> int:
    return lib.inrfit_rnvp_fit_identity_sequence(a["rnvp"], a["fp"], a["fopt"], a["coords"], a["order"], a["T"], a["HW"], a["batch"],
                                                 a["epochs"], a["opt"], a["step0"], a["epoch_loss"], a["ws"], a["ws_bytes"], a["stream"])
