"""The UNet backbone's evaluation pass on the device (include/inrfit.h: inrfit_unet_*, csrc/unet.h).

`unet_forward(net, image, features)` is what awesome_amd.model.UNet.forward does in eval() under no_grad with an fp32 network on the GPU:
every Conv2d + BatchNorm2d pair is folded into one matrix on the device (inrfit_unet_pack), and the network runs from those matrices,
one image per call (inrfit_unet_forward).  The packed weights and the workspace are cached on the module; the weights are packed
again whenever a parameter's or buffer's storage or version counter has changed (load_state_dict, an in-place edit, .to(device))."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from . import _lib as L
from .icnn import _check_dev, _stream_ptr

_CACHE = "_hip_unet_cache"


def make_desc(net, height: int, width: int, strip_points: int = 0) -> L.InrUNetDesc:
    d = L.InrUNetDesc()
    d.in_chn, d.out_chn, d.base_width = int(net.in_chn), int(net.out_chn), int(net.base_width)
    d.height, d.width, d.strip_points = int(height), int(width), int(strip_points)
    d.bn_eps = float(net.inc.conv.conv[1].eps)
    return d


def _layers(net):
    convs, bns = [], []
    for blk in net.blocks():
        convs += [blk.conv[0], blk.conv[3]]
        bns += [blk.conv[1], blk.conv[4]]
    return convs + [net.outc.conv], bns


def _signature(net):
    return tuple((t.data_ptr(), t._version) for t in list(net.parameters()) + list(net.buffers()))


def _table(tensors):
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise L.InrfitError("the UNet's parameters and running statistics must be contiguous float32 tensors on the GPU")
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return C.cast(arr, C.c_void_p), arr


def packed_weights(net, dev) -> Tensor:
    """The folded matrices of `net`, packed again when its weights have changed since the last call."""
    cache = net.__dict__.setdefault(_CACHE, {})
    sig = (_signature(net), str(dev))
    if cache.get("sig") == sig:
        return cache["packed"]
    convs, bns = _layers(net)
    if len({float(bn.eps) for bn in bns}) != 1 or any(not bn.affine or not bn.track_running_stats for bn in bns):
        raise L.InrfitError("the UNet's BatchNorms must share one eps and carry affine weights and running statistics")
    lib = L.load()
    desc = make_desc(net, 16, 16)
    n = int(lib.inrfit_unet_packed_floats(C.byref(desc)))
    if n < 0:
        L.check(n, "inrfit_unet_packed_floats")
    packed = L.scratch(n, dtype=torch.float32, device=dev)
    tables = [_table([m.weight.detach() for m in convs]), _table([m.bias.detach() for m in convs]),
              _table([m.weight.detach() for m in bns]), _table([m.bias.detach() for m in bns]),
              _table([m.running_mean for m in bns]), _table([m.running_var for m in bns])]
    rc = lib.inrfit_unet_pack(C.byref(desc), *[t[0] for t in tables], packed.data_ptr(), _stream_ptr(dev))
    L.check(rc, "inrfit_unet_pack")
    cache["sig"], cache["packed"] = sig, packed
    return packed


def _workspace(net, desc, dev) -> Tensor:
    cache = net.__dict__.setdefault(_CACHE, {})
    key = (desc.height, desc.width, desc.strip_points, str(dev))
    if cache.get("ws_key") != key:
        nbytes = int(L.load().inrfit_unet_workspace_bytes(C.byref(desc)))
        if nbytes < 0:
            L.check(nbytes, "inrfit_unet_workspace_bytes")
        cache["ws"], cache["ws_key"] = L.scratch(nbytes // 4, dtype=torch.float32, device=dev), key
    return cache["ws"]


def unet_forward(net, image: Tensor, features: Optional[Tensor], strip_points: int = 0) -> Tensor:
    """logits (B, out_chn, H, W) of `net` in evaluation mode (running statistics) on [image | features] (B, C, H, W), fp32 on the
    GPU; the images of a batch run one after the other.  strip_points: pixels per strip of the column matrix (0: the default)."""
    x = image if features is None else torch.cat((image, features), dim=1)
    if x.dim() == 3:
        x = x[None]
    x = _check_dev(x.detach(), "image")
    B, c, H, W = x.shape
    if c != net.in_chn:
        raise L.InrfitError(f"the UNet takes {net.in_chn} input channels, got {c}")
    dev = x.device
    desc = make_desc(net, H, W, strip_points)
    lib = L.load()
    with torch.cuda.device(dev):
        packed = packed_weights(net, dev)
        ws = _workspace(net, desc, dev)
        out = L.scratch(B, int(net.out_chn), H, W, dtype=torch.float32, device=dev)
        for b in range(B):
            rc = lib.inrfit_unet_forward(C.byref(desc), packed.data_ptr(), x[b].data_ptr(), out[b].data_ptr(), ws.data_ptr(),
                                         ws.numel() * 4, _stream_ptr(dev))
            L.check(rc, "inrfit_unet_forward")
    return out
