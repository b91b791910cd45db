"""Cases and float64 references for tests/test_gpu_step_l0_under_dw.py (the L = 1 step kernel's layer-0 mask and layer-0 gradient; the
CPU side of it: tests/test_step_l0_cases_host.py).  Nothing here touches the GPU or the HIP library.  The conditioning of the inputs,
the references and the bars are those of tests/step2_cases.py (its docstring), for one hidden layer.

Launches (slab base, N, workgroups); chunk c (64 points) goes to workgroup c % workgroups:

    two_and_one    base 8, N = 64 * 10 + 17   11 chunks on 8 workgroups: 0-2 take two, 3-7 one; the last chunk is ragged
    three_each     base 2, N = 64 * 5 + 1     two workgroups, three chunks each; the last chunk holds one point
    one_each       base 8, N = 192            three workgroups with one chunk each (the control: no stage is ever overwritten)
    TWO_IMAGES     base 4, N = 321, two images in one launch: two workgroups of three chunks per image

Shapes (h, C), chosen for the edges of the lane-group x tile transpose in front of the layer-0 sums (tile quads of four 16-unit tiles,
h % 16 leftover units on the VALU).  A width the library has no kernel for runs zero-padded on the next compiled one (130 or 64),
so its padded units carry exact zeros through the mask, the transpose and the sums; wider than 130 runs layer by layer:

    (130, 2), (130, 3)   two full quads, two leftover units
    (64, 2)              one quad, no leftover units
    (48, 2)              three tiles in use, the quad's fourth all padding (64 kernel)
    (100, 2)             six tiles and four units in use: the second quad half empty, a partly used tile (130 kernel)
    (132, 2)             above every compiled width: the layer-by-layer path at the same launches (the control for the route itself)"""
import torch

from tests import step2_cases as S

LAUNCHES = {"two_and_one": (8, 64 * 10 + 17, 8), "three_each": (2, 64 * 5 + 1, 2), "one_each": (8, 192, 3)}   # slab base, N, workgroups
TWO_IMAGES = (4, 321, 2)
SHAPES = [(130, 2), (130, 3), (64, 2), (48, 2), (100, 2), (132, 2)]
MULTI_CHUNK = ["two_and_one", "three_each"]

_CASES = {}


def _spec(h, C):
    from awesome_amd.icnn import IcnnSpec
    return IcnnSpec(n_hidden=h, in_features=C, n_layers=1)


def build_case(h, C, name, image=0):
    """A fresh (uncached) case: parameters (non-zero everywhere), explicit coordinates (conditioned: no ReLU pre-activation within
    4 x the float32 forward error bound of zero), soft and hard targets, an external dL/dlogits."""
    n = TWO_IMAGES[1] if name == "two_images" else LAUNCHES[name][1]
    g = torch.Generator().manual_seed(3_000_000 + 100_000 * image + 50_000 * (name == "two_images") + 1000 * h + 10 * C + n)
    spec = _spec(h, C)
    p = {k: (torch.rand(shp, generator=g) - 0.45) * 0.3 for k, shp in spec.keys_shapes()}
    coords = torch.rand(C, n, generator=g)
    un = torch.rand(n, generator=g)
    dlog = torch.randn(n, generator=g)
    p64 = S.f64(p)
    rounds, redrawn = S.redraw(lambda c: S.conditioning(p64, c.double().t())[0], coords, lambda m: torch.rand(C, m, generator=g))
    return dict(spec=spec, p=p, coords=coords, un=un, hard=(un > 0.6).float(), dlog=dlog, rounds=rounds, redrawn=redrawn, refs={},
                act0="relu", omega=1.0)


def case(h, C, name, image=0):
    """build_case, built once per key and shared: callers must not change what it returns."""
    key = (h, C, name, image)
    if key not in _CASES:
        _CASES[key] = build_case(h, C, name, image)
    return _CASES[key]


def sine_case():
    """SineLayerNet (sin layer 0, h = 130, one hidden layer) at two_and_one, built as tests/test_gpu_step_dw_first.py builds it: centred
    coordinates, the skip weights constants of the model family.  The kernel keeps its MFMA recompute of the pre-activation here."""
    key = ("sine",)
    if key in _CASES:
        return _CASES[key]
    from awesome_amd.icnn import unpack_params
    from awesome_amd.model import SineLayerNet
    n = LAUNCHES["two_and_one"][1]
    with torch.random.fork_rng():
        torch.manual_seed(62)
        m = SineLayerNet(in_features=2, n_hidden=130, n_hidden_layers=1)
    g = torch.Generator().manual_seed(3_062_001)
    flat = m.flat_parameters().cpu()
    p = unpack_params(m.spec, flat)
    coords = torch.rand(2, n, generator=g) - 0.5
    un = torch.rand(n, generator=g)
    p64 = S.f64(p)
    rounds, redrawn = S.redraw(lambda c: S.conditioning(p64, c.double().t(), m.spec.act0, m.spec.omega)[0], coords,
                               lambda k: torch.rand(2, k, generator=g) - 0.5)
    _CASES[key] = dict(spec=m.spec, p=p, flat=flat, coords=coords, un=un, hard=(un > 0.6).float(), rounds=rounds, redrawn=redrawn,
                       refs={}, act0=m.spec.act0, omega=m.spec.omega)
    return _CASES[key]
