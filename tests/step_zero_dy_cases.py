"""Cases and float64 references for tests/test_gpu_step_zero_dy.py (the L = 1 step kernel skips the backward block of a wave, and the dW
phase of a chunk, whose dL/dlogit are all exactly zero; the CPU side of it: tests/test_step_zero_dy_cases_host.py).  Nothing here
touches the GPU or the HIP library.  Launches, parameters, coordinates, conditioning, references and bars are those of
tests/step_l0_cases.py and tests/step2_cases.py; what is new is where dL/dlogit is zero.

Chunk c (64 points, four wave tiles of 16) goes to workgroup c % workgroups:

    three_each     N = 321, two workgroups: 0 takes chunks 0, 2, 4; 1 takes 1, 3, 5; chunk 5 holds one point
    two_and_one    N = 657, eight workgroups: 0-2 take two chunks (c, c + 8), 3-7 one; chunk 10 holds 17 points

Exact zero patterns (PATTERNS: launch, name): dL/dlogit is handed in (the vector-Jacobian product, INR_LOSS_EXTERNAL), the case's own
`dlog` with zeros written over the points `zero_mask` marks - so which points are zero depends on no exponential.

    all                          every point
    first / middle / last        one whole chunk, as the first, a middle and the last chunk of its workgroup
    two_consecutive[_late]       two chunks in a row on one workgroup (the flag words' double buffer), the second pair ending the loop
    alternating                  zero, live, zero on workgroup 0 and live, zero, live on workgroup 1
    one_live_w0 .. w3            a zero chunk but for ONE point, in each of the four wave tiles in turn (the chunk is live, three waves skip)
    tile_w0 .. w3                one wave tile zero inside a live chunk (that wave stages zeros, the block runs the dW phase)
    neg_zero                     -0.0 instead of +0.0: two chunks and one wave tile
    ragged                       the valid points of the ragged last chunk
    (two_and_one) first / second: the first, the second chunk of the workgroups that take two

Natural saturation (sat_case): the output layer's skip weight on x_0 is 60 and its bias centres the live logits, x_0 is in [0, 0.05) on
the live points and in [1, 1.05) on the saturated ones: logits >= 40 there (float32 and float64 sigmoid are exactly 1, both data
terms' dL/dlogit exactly 0) and |logit| <= 5 on the live points.  BCE takes target 1 on the saturated points (a confident fit that
is also right: with any other target the clamped log(0) = -100 of those points would be all there is to the loss, and its bar would
see nothing else).
The trajectory case starts 2.3 under the float32 threshold (logit 16.64) on three chunks and crosses it."""
import torch

from oracle import inr_oracle as O  # noqa: E402  (checker only)
from tests import step2_cases as S
from tests import step_l0_cases as Z

SHAPES = [(130, 2), (130, 3), (64, 2), (100, 2)]
SP, TILE = 64, 16


def _chunks(n, which):
    m = torch.zeros(n, dtype=torch.bool)
    for c in which:
        m[SP * c:SP * (c + 1)] = True
    return m


def _tile(n, chunk, wave):
    m = torch.zeros(n, dtype=torch.bool)
    m[SP * chunk + TILE * wave:SP * chunk + TILE * (wave + 1)] = True
    return m


def zero_mask(launch, pattern):
    """-> (N,) bool: the points whose dL/dlogit the pattern sets to zero"""
    n = Z.LAUNCHES[launch][1]
    if pattern == "all":
        return torch.ones(n, dtype=torch.bool)
    if launch == "two_and_one":
        return {"first": _chunks(n, [0, 1, 2]), "second": _chunks(n, [8, 9]), "ragged": _chunks(n, [10])}[pattern]
    if pattern.startswith("one_live_w"):
        m = _chunks(n, [2])
        m[SP * 2 + TILE * int(pattern[-1]) + 5] = False
        return m
    if pattern.startswith("tile_w"):
        return _tile(n, 2, int(pattern[-1]))
    return {"first": _chunks(n, [0]), "middle": _chunks(n, [2]), "last": _chunks(n, [4]), "two_consecutive": _chunks(n, [0, 2]),
            "two_consecutive_late": _chunks(n, [3, 5]), "alternating": _chunks(n, [0, 4, 3]),
            "neg_zero": _chunks(n, [0, 3]) | _tile(n, 2, 1), "ragged": _chunks(n, [5])}[pattern]


PATTERNS = [("three_each", p) for p in ["all", "first", "middle", "last", "two_consecutive", "two_consecutive_late", "alternating"]
            + [f"one_live_w{w}" for w in range(4)] + [f"tile_w{w}" for w in range(4)] + ["neg_zero", "ragged"]] \
    + [("two_and_one", p) for p in ["all", "first", "second", "ragged"]]

_CASES = {}


def pattern_case(h, C, launch, pattern, image=0):
    """The case of tests/step_l0_cases.py with the pattern's zeros in `dlog` (its own reference cache); shared, not to be changed."""
    key = ("pattern", h, C, launch, pattern, image)
    if key not in _CASES:
        c = Z.case(h, C, launch, image)
        m = zero_mask("three_each" if launch == "two_images" else launch, pattern)
        dlog = c["dlog"].clone()
        dlog[m] = -0.0 if pattern == "neg_zero" else 0.0
        _CASES[key] = dict(c, dlog=dlog, zero=m, refs={})
    return _CASES[key]


def sine_pattern_case():
    """the sine encode net of tests/step_l0_cases.py at two_and_one with the pattern `second` and wave tile 2 of chunk 1 zero"""
    key = ("sine",)
    if key not in _CASES:
        c = Z.sine_case()
        n = c["coords"].shape[1]
        m = zero_mask("two_and_one", "second") | _tile(n, 1, 2)
        dlog = torch.randn(n, generator=torch.Generator().manual_seed(4_062_001))
        dlog[m] = 0.0
        _CASES[key] = dict(c, dlog=dlog, zero=m, refs={})
    return _CASES[key]


def encode_vjp(c, dtype=torch.float64):
    """d (dlog . logits) / d parameters of an encode net, everything but the skip weights (constants of the model family)"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in c["p"].items()}
    y = O.icnn_forward(p, c["coords"].to(dtype).t(), c["act0"], c["omega"])[:, 0]
    (y * c["dlog"].to(dtype)).sum().backward()
    return {k: v.grad for k, v in p.items() if not k.endswith("skp.weight")}


# ---- natural saturation -----------------------------------------------------------------------------------------------------------
SAT_SLOPE, SAT_MIN, LIVE_MAX = 60.0, 40.0, 5.0
SAT_LAUNCHES = ["three_each", "two_and_one"]


def sat_mask(launch):
    n = Z.LAUNCHES[launch][1]
    if launch == "three_each":
        return _chunks(n, [0, 3, 5]) | _tile(n, 2, 1)      # a first and a middle chunk, the ragged last one, one wave tile of a live chunk
    return _chunks(n, [1, 8, 10]) | _tile(n, 9, 3)


def _recondition(p64, coords, draw):
    """redraw (draw(bad) -> new columns, each in its own group's range of x_0) the points that are ill-conditioned -> rounds"""
    for r in range(S.MAX_ROUNDS):
        bad = S.conditioning(p64, coords.double().t())[0]
        if not bool(bad.any()):
            return r
        coords[:, bad] = draw(bad)
    raise AssertionError("still ill-conditioned")


def sat_case(h, C, launch):
    """-> the case (parameters of tests/step_l0_cases.py but for the output layer's bias and skip weight on x_0; coordinates drawn
    anew, conditioned) with `sat` (N,) bool, `un` (soft targets) and `un_bce` (1 on the saturated points)."""
    key = ("sat", h, C, launch)
    if key in _CASES:
        return _CASES[key]
    base = Z.case(h, C, launch)
    n = base["coords"].shape[1]
    g = torch.Generator().manual_seed(5_000_000 + 1000 * h + 10 * C + n)
    sat = sat_mask(launch)
    p = {k: v.clone() for k, v in base["p"].items()}
    p["out.skp.weight"][0, 0] = SAT_SLOPE
    p["out.ln.bias"][0] = 0.0

    def draw(sel):
        x = torch.rand(C, int(sel.sum()), generator=g)
        x[0] = 0.05 * x[0] + sat[sel].float()
        return x

    coords = draw(torch.ones(n, dtype=torch.bool))
    rounds = _recondition(S.f64(p), coords, draw)
    with torch.no_grad():
        y = O.icnn_forward(S.f64(p), coords.double().t())[:, 0]
    live = y[~sat]
    p["out.ln.bias"][0] = float(-(live.max() + live.min()) / 2)     # centre the live logits
    assert float(p["out.ln.bias"][0]) != 0.0
    un = base["un"].clone()
    un_bce = un.clone()
    un_bce[sat] = 1.0
    c = dict(base, p=p, coords=coords, sat=sat, un=un, un_bce=un_bce, hard=(un > 0.6).float(), rounds=rounds, refs={})
    _CASES[key] = c
    return c


def sat_loss_and_grads(c, kind, dtype=torch.float64):
    tgt = (c["un_bce"] if kind == "bce" else c["un"]).to(dtype).reshape(1, 1, 1, -1)
    return O.loss_and_grads({k: v.to(dtype) for k, v in c["p"].items()}, S.image(c, dtype), tgt, kind, "none")


def dl_dlogit(c, kind, dtype=torch.float32):
    """dL/dlogit (N,) of the data term by torch's autograd in `dtype`, and the logits"""
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    with torch.no_grad():
        y = O.icnn_forward(p, c["coords"].to(dtype).t())[:, 0]
    y = y.clone().requires_grad_(True)
    tgt = (c["un_bce"] if kind == "bce" else c["un"]).to(dtype)
    O.weighted_loss(torch.sigmoid(y), tgt, kind, "none").backward()
    return y.grad, y.detach()


def nan_case():
    """sat_case(130, 2, three_each) with a NaN coordinate on one point of chunk 0, whose other 63 points are saturated: the chunk's
    only non-zero dL/dlogit is a NaN"""
    key = ("nan",)
    if key not in _CASES:
        c = sat_case(130, 2, "three_each")
        coords = c["coords"].clone()
        coords[:, 37] = float("nan")
        _CASES[key] = dict(c, coords=coords, refs={})
    return _CASES[key]


# ---- a trajectory that crosses the float32 threshold ----------------------------------------------------------------------------------
THRESHOLD = 16.64      # 1 + exp(-y) rounds to 1 in float32 from about here
TRAJ_STEPS = 25


def traj_case():
    """three_each, h = 130: chunks 0 and 3 and the one point of chunk 5 start with logits in [THRESHOLD - 2.3, THRESHOLD - 2.2] and
    target 1, the live points (x_0 in [0, 0.05), logits centred) have target 1 on nine points in ten: every Adam step raises the
    logits there (by about 2 in the first step, then by about 0.15 per step up to step 15): the three chunks are live for the first
    steps, saturated from about step 5 on and back at the threshold at the end."""
    key = ("traj",)
    if key in _CASES:
        return _CASES[key]
    base = Z.case(130, 2, "three_each")
    n, C = base["coords"].shape[1], 2
    g = torch.Generator().manual_seed(6_130_321)
    near = _chunks(n, [0, 3, 5])
    p = {k: v.clone() for k, v in base["p"].items()}
    p["out.skp.weight"][0, 0] = SAT_SLOPE
    p["out.ln.bias"][0] = 0.0
    p64 = S.f64(p)
    want = THRESHOLD - 2.3 + 0.1 * torch.rand(n, generator=g).double()

    def solve(x):      # x_0 of the `near` columns such that the float64 logit is `want` (the hidden layers hardly see x_0's change)
        sel = near_of[0]
        for _ in range(6):
            with torch.no_grad():
                y = O.icnn_forward(p64, x.double().t())[:, 0]
            x[0] = torch.where(sel, (x[0].double() + (want_of[0] - y) / SAT_SLOPE).float(), x[0])
        return x

    near_of, want_of = [near], [want]
    coords = torch.rand(C, n, generator=g)
    coords[0] = 0.05 * coords[0]
    with torch.no_grad():
        live = O.icnn_forward(p64, coords.double().t())[:, 0][~near]
    p["out.ln.bias"][0] = float(-(live.max() + live.min()) / 2)
    p64 = S.f64(p)
    coords = solve(coords)
    for r in range(S.MAX_ROUNDS):
        bad = S.conditioning(p64, coords.double().t())[0]
        if not bool(bad.any()):
            break
        coords[1, bad] = torch.rand(int(bad.sum()), generator=g)
        coords = solve(coords)
    else:
        raise AssertionError("still ill-conditioned")
    hard = (torch.rand(n, generator=g) < 0.9).float()
    hard[near] = 1.0
    c = dict(base, p=p, coords=coords, near=near, hard=hard, un=hard, un_bce=hard, rounds=r, refs={})
    _CASES[key] = c
    return c


def trajectory(c, steps=TRAJ_STEPS, dtype=torch.float64):
    """`steps` Adam + clamp steps (se, lr 2e-3) on the case's hard targets -> (parameters, losses, final logits (N,))"""
    pf, losses, logits = O.fit_icnn({k: v.to(dtype) for k, v in c["p"].items()}, S.image(c, dtype),
                                    c["hard"].to(dtype).reshape(1, 1, 1, -1), steps, lr=2e-3)
    return pf, losses, logits.reshape(-1)


def dead_chunks(dy):
    """-> the chunks (of 64 points, the last one ragged) whose dL/dlogit are all zero"""
    n = dy.numel()
    return [c for c in range((n + SP - 1) // SP) if bool((dy[SP * c:SP * (c + 1)] == 0).all())]
