"""The two host-side pieces of JointTrainer's fused routes that every route shares and that nothing on the device would catch
(no GPU): how one training item becomes the batch-size-1 item the routes take (awesome_amd.agent._normalise_item), and how the
segmentation networks' flat gradient buffer becomes their parameters' .grad (cnnseg.assign_grads / fcseg.assign_grads).  The
expected shapes are what TorchAgent's step hands the WrapperModule: an image item (C, H, W) or (1, C, H, W), a pixel item (n, F) or
(1, n, F) (WrapperModule._forward_pixels), every other input batched the same way, non-tensor inputs passed through."""
import pytest
import torch

from awesome_amd.agent import _normalise_item

H, W, N = 6, 5, 11


def _shapes(item):
    xi, ai, n, pixel = item
    return tuple(xi.shape), tuple(tuple(a.shape) if isinstance(a, torch.Tensor) else a for a in ai), n, pixel


# (inputs' shapes; a non-tuple stands for itself), input_mode, prior_arg_mode -> (xi shape, ai shapes, n, pixel) or None
_CASES = [
    # image items: rank 3 gains the batch axis, rank 4 is taken as it is; so does every other tensor input
    ([(3, H, W)], "image", None, ((1, 3, H, W), (), H * W, False)),
    ([(1, 3, H, W)], "image", None, ((1, 3, H, W), (), H * W, False)),
    ([(3, H, W), (2, H, W)], "image", None, ((1, 3, H, W), ((1, 2, H, W),), H * W, False)),
    ([(1, 3, H, W), (1, 2, H, W)], "image", None, ((1, 3, H, W), ((1, 2, H, W),), H * W, False)),
    ([(3, H, W), (2, H, W), None], "image", None, ((1, 3, H, W), ((1, 2, H, W), None), H * W, False)),
    ([(3, H, W), (2, H, W)], "image", "xy_c_preattached", ((1, 3, H, W), ((1, 2, H, W),), H * W, False)),   # (mode: pixel items only)
    ([(2, 3, H, W)], "image", None, None),                                                                  # batch 2
    ([(2, 3, H, W), (2, 2, H, W)], "image", None, None),
    # pixel items: the rows of the one image, rank 2 as they are, rank 3 without the batch axis
    ([(N, 5)], "pixel", "xy_c_preattached", ((N, 5), (), N, True)),
    ([(1, N, 5)], "pixel", "xy_c_preattached", ((N, 5), (), N, True)),
    ([(N, 3), (N, 2)], "pixel", "xy_c_preattached", ((N, 3), ((N, 2),), N, True)),
    ([(1, N, 3), (1, N, 2)], "pixel", "xy_c_preattached", ((N, 3), ((N, 2),), N, True)),
    ([(N, 3), (N, 2), (N, 2)], "pixel", "param_clean_grid", ((N, 3), ((N, 2), (N, 2)), N, True)),
    ([(1, N, 3), (1, N, 2), (1, N, 2)], "pixel", "param_clean_grid", ((N, 3), ((N, 2), (N, 2)), N, True)),
    ([(2, N, 5)], "pixel", "xy_c_preattached", None),                                                       # batch 2
    ([(N,)], "pixel", "xy_c_preattached", None),                                                            # rank 1
    ([(1, 1, N, 5)], "pixel", "xy_c_preattached", None),                                                    # rank 4
    ([(N, 3), (N, 2)], "pixel", "param_clean_grid", None),                                                  # no clean-xy rows
    ([(N, 3), (N, 2), None], "pixel", "param_clean_grid", None),
    ([(N, 5)], "pixel", "xy", None),                                                                        # unknown modes
    ([(N, 5)], "pixel", None, None),
]


@pytest.mark.parametrize("shapes,input_mode,prior_arg_mode,want", _CASES)
def test_normalise_item(shapes, input_mode, prior_arg_mode, want):
    inputs = [torch.zeros(s) if isinstance(s, tuple) else s for s in shapes]
    got = _normalise_item(inputs, input_mode, prior_arg_mode)
    if want is None:
        assert got is None
    else:
        assert _shapes(got) == want


def test_normalise_item_keeps_the_values():
    x, f = torch.arange(3.0 * H * W).reshape(3, H, W), torch.arange(2.0 * H * W).reshape(2, H, W)
    xi, ai, _, _ = _normalise_item([x, f])
    assert torch.equal(xi[0], x) and torch.equal(ai[0][0], f)
    assert xi.data_ptr() == x.data_ptr() and ai[0].data_ptr() == f.data_ptr()          # views, no copies
    rows, xy = torch.arange(N * 3.0).reshape(1, N, 3), torch.arange(N * 2.0).reshape(1, N, 2)
    xi, ai, _, _ = _normalise_item([rows, xy], "pixel", "xy_c_preattached")
    assert torch.equal(xi, rows[0]) and torch.equal(ai[0], xy[0])
    assert xi.data_ptr() == rows.data_ptr() and ai[0].data_ptr() == xy.data_ptr()


@pytest.mark.parametrize("module", ["fcseg", "cnnseg"])
def test_assign_grads_views_the_flat_buffer_in_parameters_order(module):
    import importlib
    from awesome_amd.model import CNNNet, FCNet
    M = importlib.import_module(f"awesome_amd.{module}")
    net = (FCNet(in_chn=5, out_chn=1, width=16, depth=3, in_type="rgbxy") if module == "fcseg"
           else CNNNet(in_chn=5, out_chn=1, kernel_size=3, width=16, depth=2, in_type="rgbxy"))
    params = list(net.parameters())
    P = sum(p.numel() for p in params)
    flat = torch.arange(float(P))
    M.assign_grads(net, flat)
    off = 0
    for p in params:
        assert p.grad.shape == p.shape
        assert p.grad.data_ptr() == flat.data_ptr() + 4 * off                          # a view at its offset, not a copy
        assert torch.equal(p.grad.reshape(-1), flat[off:off + p.numel()])
        off += p.numel()
    assert off == P == flat.numel()
    flat[0] = -1.0
    assert float(params[0].grad.reshape(-1)[0]) == -1.0
    with pytest.raises(AssertionError):
        M.assign_grads(net, torch.zeros(P + 1))
    with pytest.raises((AssertionError, RuntimeError)):          # (too short: the last parameter's view already fails)
        M.assign_grads(net, torch.zeros(P - 1))
