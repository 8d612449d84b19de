"""Inputs, references and the two bound rules shared by test_spline_sharp_cpu.py and
test_gpu_spline_sharp.py: the TRAINING spline (csrc/spline_autograd.hip: build_knots, find_bin,
rqs_bin_theta, rqs_bin, rqs_bin_bwd, knots_backward) on SHARP bins, values and gradients, against
float64.

Every other test of that arithmetic either runs on near-uniform bins (logits of std 0.7) against
float32, or compares the fused kernels with torch ops that call the same HIP spline.  Here a
quarter of the elements keep that mild regime and the others have logits of std 3, or planted
extremes: K - 1 bins at the minimum width next to one that takes the rest, bin slopes of 1e-3 and
1e3, derivative logits beyond the softplus threshold and derivatives at the minimum.

The reference is a plain float64 restatement of the circular rational-quadratic spline (rqs64
below), differentiated by autograd.  A sharp bin amplifies float32 rounding by its slope, so no
fixed tolerance holds.  Two rules:

  rule 1 (out, lad, g_x, g_ud):  |got - exact| <= base + C_ENV_S * env   per element, where env is
          how far the float64 value itself moves when x, the interior knots and the derivatives
          move by one float32 rounding (8 seeded sign patterns);
  rule 2 (g_uw, g_uh):  no input-perturbation envelope bounds the float32 error of the logit
          gradients (softmax's backward p_k (g_k - sum_j p_j g_j) cancels where one p_k is ~1), so
          the yardstick is the float32 torch restatement itself, per class of elements: the
          largest and the 90th percentile of the row error may be 4 x the yardstick's.

Everything here runs on the CPU and is computed once per case."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from flowstate.normflows import autograd_flow as AF

EPS32 = 2.0 ** -23
B = 3.0
assert float(np.float32(B)) == B     # the planted +-fl32(B) elements sit ON the bound
STEP = B * EPS32                     # one float32 ulp of B
M = 800                              # three full 256-thread blocks and a ragged one
CLASS_N = 192
CLASSES = ("wide0", "steep0", "sharp", "mild")
N_PLANTED = M - CLASS_N * len(CLASSES)     # 32
N_FIXED = 8                                # planted elements that are no knot pairs
MIN = 1e-3                                 # minimum bin width, bin height and derivative
N_PERTURB = 8
MARGIN_ULPS = 64      # |x| within 64 ulp(B) of B: the inside test itself depends on rounding
ROOT_MARGIN = 1e-6    # inverse: float64 root within 1e-6 of 0 or 1 (the pinned root's kink)
# An element this close to an interior knot of the side its bin is searched on may land in the
# neighbouring bin in float32: out and lad are continuous across a knot and keep their bounds,
# the gradients are another function on the other side and are held to finiteness.  16 ulp(B) is
# the worst float32 rounding of a knot: a cumulative sum of K <= 32 terms below 1 (32 x 2^-25)
# times 2 B.  The planted knot pairs are such elements by construction.
FLIP_ULPS = 16
MAX_EXCLUDED = 0.05   # share of the elements of a case that may be left out of the bounds
RATIO_CAP = 16.0      # admissible seed: the yardstick's (err - base) / env at most this
Y_FLOOR = 2e-5        # floor of each rule-2 yardstick value

FIXED_K = (5, 8, 15, 32)   # bin counts the spline kernels are instantiated for
ANY_K = (7, 10, 1)         # bin counts only the runtime-K kernels accept
CASES = [(K, inv) for K in FIXED_K + ANY_K for inv in (False, True)]
RULE1 = ("out", "lad", "g_x", "g_ud")
RULE2 = ("g_uw", "g_uh")
NAMES = ("out", "lad", "g_x", "g_uw", "g_uh", "g_ud")

# Input seed per case: the first seed (1, 2, ...) that is ADMISSIBLE, measured on the float64
# reference and the float32 torch restatement alone (test_spline_sharp_cpu.py re-checks every
# condition on the seed kept here):
#   * at most MAX_EXCLUDED of the elements left out of the bounds, and as few near a knot;
#   * the float32 restatement finite on every element inside the interval;
#   * the float32 restatement's (err - base) / env at most RATIO_CAP on every checked element.
# Seed 1 is rejected three times, each for one planted knot element of the inverse direction
# whose root lies within 1e-4 of its bin's end (ratios: K = 5 out 403, in a bin of slope 1e-3
# whose discriminant bb^2 - 4 a c cancels to 4 % of bb^2; K = 8 lad 53; K = 15 lad 19.9).
SEEDS = {(5, False): 1, (5, True): 2, (8, False): 1, (8, True): 2, (15, False): 1, (15, True): 2,
         (32, False): 1, (32, True): 1, (7, False): 1, (7, True): 1, (10, False): 1, (10, True): 1,
         (1, False): 1, (1, True): 1}

# C_ENV_S: 4 x the largest (err - base) / env that the float32 torch restatement
# (autograd_flow.circular_rqs_torch on CPU tensors, with the stable pinned root) shows on checked
# elements over all cases, rounded up to a power of two.  The factor 4 is what
# flow_sharp_cases.py leaves the kernels for their other operation order (here: knots summed in
# double, expf / logf of the device library, the hand-written adjoint).  Measured per case
# (test_spline_sharp_cpu.py::test_c_env_s_is_the_measured_one prints and re-derives them):
C_ENV_RATIOS = {   # (K, inverse): (out, lad, g_x, g_ud); 0: the restatement within base everywhere
    (5, False): (1.38, 1.72, 0.63, 0.0), (5, True): (0.52, 1.55, 0.0, 0.0),
    (8, False): (2.06, 14.19, 1.2, 2.76), (8, True): (1.52, 3.1, 0.0, 0.0),
    (15, False): (3.94, 6.81, 4.63, 0.3), (15, True): (0.37, 5.92, 6.93, 6.33),
    (32, False): (0.09, 0.13, 0.45, 0.16), (32, True): (0.0, 0.33, 0.47, 0.0),
    (7, False): (1.89, 3.39, 2.34, 2.95), (7, True): (1.52, 2.87, 0.0, 0.0),
    (10, False): (2.88, 11.75, 3.08, 1.04), (10, True): (1.95, 6.96, 1.45, 6.22),
    (1, False): (0.0, 0.0, 0.0, 0.0), (1, True): (0.0, 0.0, 0.0, 0.0)}
C_ENV_S = 64.0      # 4 x 14.19 = 56.8, rounded up to a power of two


# --- the float64 reference ------------------------------------------------------------------------
def _knots(u, pert):
    """(..., K + 1) knots on [-B, B] and the K bin sizes: softmax, minimum-size affine, cumsum,
    pinned ends.  pert (..., K + 1) is added after the cumsum; the ends stay pinned."""
    K = u.shape[-1]
    s = MIN + (1 - MIN * K) * F.softmax(u, dim=-1)
    c = 2 * B * F.pad(torch.cumsum(s, dim=-1), pad=(1, 0)) - B
    if pert is not None:
        c = c + pert
    c = torch.cat([torch.full_like(c[..., :1], -B), c[..., 1:-1], torch.full_like(c[..., :1], B)], dim=-1)
    return c, c[..., 1:] - c[..., :-1]


def rqs64(x, uw, uh, ud, inverse, pw=None, ph=None, pd=None):
    """The circular rational-quadratic spline on [-B, B], identity outside.  pw / ph move the
    interior width / height knots, pd scales the derivatives (the envelope's hooks).  Returns
    (out, lad, bin, theta); the inverse root in its cancellation-free form, not pinned."""
    inside = (x >= -B) & (x <= B)
    xi = torch.where(inside, x, torch.zeros_like(x))
    K = uw.shape[-1]
    cw, w = _knots(uw, pw)
    ch, h = _knots(uh, ph)
    d = MIN + F.softplus(ud)
    if pd is not None:
        d = d * pd
    kn = (ch if inverse else cw).detach().clone()
    kn[..., -1] += 1e-6
    b = (torch.sum(xi[..., None] >= kn, dim=-1) - 1).clamp(0, K - 1)[..., None]
    g = lambda t: t.gather(-1, b)[..., 0]   # noqa: E731
    icw, ibw, ich, ih, d0, d1 = g(cw), g(w), g(ch), g(h), g(d), g(d[..., 1:])
    s = ih / ibw
    sdd = d0 + d1 - 2 * s
    if inverse:
        a = (xi - ich) * sdd + ih * (s - d0)
        bb = ih * d0 - (xi - ich) * sdd
        c = -s * (xi - ich)
        sq = torch.sqrt(torch.abs(bb * bb - 4 * a * c))
        pos = bb >= 0
        th = torch.where(pos, 2 * c, sq - bb) / torch.where(pos, -bb - sq, 2 * a)
        o = th * ibw + icw
    else:
        th = (xi - icw) / ibw
    t = th * (1 - th)
    den = s + sdd * t
    lad = torch.log(s * s * (d1 * th * th + 2 * s * t + d0 * (1 - th) * (1 - th))) - 2 * torch.log(den)
    if inverse:
        lad = -lad
    else:
        o = ich + ih * (s * th * th + d0 * t) / den
    return (torch.where(inside, o, x), torch.where(inside, lad, torch.zeros_like(lad)), b[..., 0], th.detach())


def values_and_grads(fn, x, uw, uh, ud, wo, wl, dtype=torch.float64, device="cpu"):
    """{name: float64 numpy array} of out, lad and the gradients of sum(wo out) + sum(wl lad):
    fn(x, uw, uh, ud) -> (out, lad, ...) on leaves of the given dtype and device."""
    ts = [t.to(device=device, dtype=dtype).clone().requires_grad_(True) for t in (x, uw, uh, ud)]
    res = fn(*ts)
    out, lad = res[0], res[1]
    loss = (out * wo.to(device=device, dtype=dtype)).sum() + (lad * wl.to(device=device, dtype=dtype)).sum()
    grads = torch.autograd.grad(loss, ts)
    vals = [out.detach(), lad.detach()] + list(grads)
    return {n: v.double().cpu().numpy() for n, v in zip(NAMES, vals)}


def restatement32(inverse):
    """The yardstick: the float32 torch restatement the CPU path runs."""
    return lambda *ts: AF.circular_rqs_torch(*ts, B, inverse)


# --- inputs ---------------------------------------------------------------------------------------
def _plant(uw, uh, ud, rows, K, wide):
    """wide0 (wide): width bin 0 and height bin K - 1 take everything, the other bins sit at the
    minimum: bin 0 has slope ~1e-3, bin K - 1 slope ~1e3.  steep0: the mirror image.  Derivative
    logits: +25 (beyond the softplus threshold), -25 (the derivative is the minimum) and 3 at the
    end (its own parameter: the circular tails tie nothing)."""
    uw[rows] = 0.0
    uh[rows] = 0.0
    uw[rows, 0 if wide else K - 1] = 12.0
    uh[rows, K - 1 if wide else 0] = 12.0
    ud[rows, 0] = 25.0
    ud[rows, 1] = -25.0
    ud[rows, K] = 3.0


def _other_side(v32, exact):
    """The float32 neighbour of v32 on the other side of exact (v32 itself if it is exact)."""
    if float(v32) == exact:
        return v32
    return np.nextafter(v32, np.float32(np.inf if float(v32) < exact else -np.inf))


def make_inputs(K, inverse, seed):
    """x (M,), uw, uh (M, K), ud (M, K + 1), the loss weights wo, wl (M,), all float32, and info:
    info["classes"][name] -> slice; info["planted"][name] -> index; info["knot_pairs"] -> slice
    (pairs of neighbouring floats around one interior knot of the searched side: width knots in
    the forward direction, height knots in the inverse; empty knots at K = 1, where those
    elements stay uniform).  The planted elements fill the last N_PLANTED slots; their logits are
    std-3 draws, except the bin middles (wide0 logits) and the knot pairs (pair q: class q % 4)."""
    g = torch.Generator().manual_seed(int(seed))
    uw = torch.randn(M, K, generator=g) * 3.0
    uh = torch.randn(M, K, generator=g) * 3.0
    ud = torch.randn(M, K + 1, generator=g) * 3.0
    x = ((torch.rand(M, generator=g, dtype=torch.float64) * 2 - 1) * B).float().clamp_(-B, B)
    wo = torch.randn(M, generator=g)
    wl = torch.randn(M, generator=g)
    classes = {n: slice(i * CLASS_N, (i + 1) * CLASS_N) for i, n in enumerate(CLASSES)}
    _plant(uw, uh, ud, classes["wide0"], K, True)
    _plant(uw, uh, ud, classes["steep0"], K, False)
    for t in (uw, uh, ud):
        t[classes["mild"]] *= 0.7 / 3.0
    p0 = CLASS_N * len(CLASSES)
    names = ("plusB", "minusB", "zero", "negzero", "just_outside", "far_outside", "firstbin_mid", "lastbin_mid")
    planted = {n: p0 + i for i, n in enumerate(names)}
    x[planted["plusB"]] = B
    x[planted["minusB"]] = -B
    x[planted["zero"]] = 0.0
    x[planted["negzero"]] = -0.0
    for t in (uw, uh, ud, wo, wl):   # the same spline and weights at 0.0 and at -0.0
        t[planted["negzero"]] = t[planted["zero"]]
    x[planted["just_outside"]] = float(np.nextafter(np.float32(B), np.float32(np.inf)))
    x[planted["far_outside"]] = 1.2 * B
    side = uh if inverse else uw
    for name, lo in (("firstbin_mid", 0), ("lastbin_mid", K - 1)):
        r = planted[name]
        _plant(uw, uh, ud, [r], K, True)
        kn = _knots(side[r].double(), None)[0]
        x[r] = float(np.float32(0.5 * (kn[lo].item() + kn[lo + 1].item())))
    pairs = slice(p0 + N_FIXED, M)
    if K > 1:
        for q in range((M - pairs.start) // 2):
            r = pairs.start + 2 * q
            if q % 4 < 2:
                _plant(uw, uh, ud, [r], K, q % 4 == 0)
            elif q % 4 == 3:
                for t in (uw, uh, ud):
                    t[r] *= 0.7 / 3.0
            for t in (uw, uh, ud):
                t[r + 1] = t[r]
            exact = _knots(side[r].double(), None)[0][1 + q % (K - 1)].item()
            v = np.float32(exact)
            x[r] = float(v)
            x[r + 1] = float(_other_side(v, exact))
    return x, uw, uh, ud, wo, wl, dict(classes=classes, planted=planted, knot_pairs=pairs)


# --- one case -------------------------------------------------------------------------------------
def _absdiff(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    return np.where(np.isfinite(d), d, np.inf)


def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


class Case:
    """Inputs, float64 values (exact), envelope (env), the float32 restatement's values (yard)
    and the masks of one (K, inverse, seed)."""


@functools.lru_cache(maxsize=None)
def case(K, inverse, seed=None):
    c = Case()
    c.K, c.inverse = K, inverse
    c.seed = SEEDS[(K, inverse)] if seed is None else seed
    c.x, c.uw, c.uh, c.ud, c.wo, c.wl, c.info = make_inputs(K, inverse, c.seed)
    args = (c.x, c.uw, c.uh, c.ud, c.wo, c.wl)
    c.exact = values_and_grads(lambda *ts: rqs64(*ts, inverse), *args)
    with torch.no_grad():
        x64 = c.x.double()
        _, _, b, th = rqs64(x64, c.uw.double(), c.uh.double(), c.ud.double(), inverse)
        kn = _knots((c.uh if inverse else c.uw).double(), None)[0][:, 1:-1]
        gap = (x64[:, None] - kn).abs().min(dim=1).values.numpy() if K > 1 else np.full(M, np.inf)
    c.bin, c.theta = b.numpy(), th.numpy()
    # the envelope
    c.outside = ~((c.x >= -B) & (c.x <= B)).numpy()
    g = torch.Generator().manual_seed(1000 + c.seed)
    c.env = {n: np.zeros_like(v) for n, v in c.exact.items()}
    out_t = torch.from_numpy(c.outside)
    for _ in range(N_PERTURB):
        pw, ph = STEP * _signs((M, K + 1), g), STEP * _signs((M, K + 1), g)
        pd = 1 + EPS32 * _signs((M, K + 1), g)
        xp = torch.where(out_t, x64, (x64 + STEP * _signs((M,), g)).clamp(-B, B))
        moved = values_and_grads(lambda *ts: rqs64(*ts, inverse, pw, ph, pd), xp, *args[1:])
        for n in NAMES:
            c.env[n] = np.maximum(c.env[n], _absdiff(moved[n], c.exact[n]))
    env_inf = np.zeros(M, bool)
    for n in NAMES:
        env_inf |= ~np.isfinite(c.env[n]).reshape(M, -1).all(axis=1)
    c.boundary = (B - np.abs(c.x.double().numpy()) <= MARGIN_ULPS * STEP) & ~c.outside
    root_edge = np.minimum(c.theta, 1 - c.theta) < ROOT_MARGIN if inverse else np.zeros(M, bool)
    c.flip = ~c.outside & (gap <= FLIP_ULPS * STEP)
    # A root at a bin's end that is on a knot (the planted knot pairs in a tall bin) keeps its out
    # and lad bounds like every knot element; any other one is left out altogether.
    c.excluded = ~c.outside & (c.boundary | env_inf | (root_edge & ~c.flip))
    c.checked = ~c.outside & ~c.excluded            # out, lad
    c.grad_checked = c.checked & ~c.flip            # every gradient
    # the yardstick
    c.yard = values_and_grads(restatement32(inverse), *args, dtype=torch.float32)
    AF.check_nan_flags()
    return c


# --- rule 1 ---------------------------------------------------------------------------------------
def base_of(name, exact):
    """The project's existing bound of each quantity (tests/test_gpu_spline_grad.py)."""
    if name == "out":
        return np.full_like(exact, 1e-5 * B)
    if name == "lad":
        return 1e-4 * np.abs(exact) + 2e-4
    rowmax = np.abs(exact).reshape(len(exact), -1).max(axis=1)
    atol = 2e-5 * np.maximum(1.0, rowmax)
    return 2e-4 * np.abs(exact) + (atol[:, None] if exact.ndim == 2 else atol)


def mask_of(c, name):
    return c.checked if name in ("out", "lad") else c.grad_checked


def env_ratio(c, got, name):
    """max over the checked elements of (err - base) / env; +inf where got is not finite."""
    err = _absdiff(np.asarray(got[name], np.float64), c.exact[name])
    exc = err - base_of(name, c.exact[name])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(exc > 0, exc / c.env[name], 0.0)
    ratio = ratio.reshape(M, -1).max(axis=1)[mask_of(c, name)]
    return float(ratio.max()) if ratio.size else 0.0


def rule1_failures(c, got, c_env):
    msgs = []
    for name in RULE1:
        err = _absdiff(np.asarray(got[name], np.float64), c.exact[name])
        with np.errstate(invalid="ignore"):
            bound = base_of(name, c.exact[name]) + c_env * c.env[name]
        bad = (~(err <= bound)).reshape(M, -1).any(axis=1) & mask_of(c, name)
        if bad.any():
            rows = np.flatnonzero(bad)[:4]
            msgs.append(f"rule 1 {name}: {bad.sum()} elements; {rows.tolist()} x {c.x.numpy()[rows].tolist()} bin "
                        f"{c.bin[rows].tolist()} err {err.reshape(M, -1).max(axis=1)[rows].tolist()} ratio "
                        f"{env_ratio(c, got, name):.1f}")
    return msgs


# --- rule 2 ---------------------------------------------------------------------------------------
def row_error(c, got, name):
    """e_row = |got - exact|_inf / max(1, |exact|_inf) per element (row of logits)."""
    err = _absdiff(np.asarray(got[name], np.float64), c.exact[name]).reshape(M, -1).max(axis=1)
    return err / np.maximum(1.0, np.abs(c.exact[name]).reshape(M, -1).max(axis=1))


def rule2_classes(c):
    """{class: indices of its elements held to rule 2}: the four classes, and the planted
    elements that are checked and on no knot."""
    cl = {n: np.arange(s.start, s.stop) for n, s in c.info["classes"].items()}
    cl["planted"] = np.arange(CLASS_N * len(CLASSES), M)
    return {n: i[c.grad_checked[i]] for n, i in cl.items()}


def rule2_stats(c, got):
    """{(name, class): (max, 90th percentile) of e_row}"""
    st = {}
    for name in RULE2:
        e = row_error(c, got, name)
        for cls, idx in rule2_classes(c).items():
            if len(idx):
                st[(name, cls)] = (float(e[idx].max()), float(np.percentile(e[idx], 90)))
    return st


def rule2_failures(c, got, factor):
    msgs = []
    yard = rule2_stats(c, c.yard)
    for key, (mx, p90) in rule2_stats(c, got).items():
        ymx, yp90 = (max(v, Y_FLOOR) for v in yard[key])
        if not (mx <= factor * ymx and p90 <= factor * yp90):
            msgs.append(f"rule 2 {key}: max {mx:.3e} (yardstick {ymx:.3e}), p90 {p90:.3e} (yardstick {yp90:.3e})")
    return msgs


# --- the whole check ------------------------------------------------------------------------------
def failures(c, got, factor=4.0):
    """Every way `got` ({name: array}) breaks the rules of case c.  factor 4: the kernels;
    factor 1: the yardstick itself (rule 1 with C_ENV_S / 4)."""
    msgs = []
    got = {n: np.asarray(got[n], np.float64) for n in NAMES}
    ins, out = ~c.outside, c.outside
    x64 = c.x.double().numpy()
    for n in NAMES:   # finite wherever x is inside, excluded and knot elements included
        bad = ~np.isfinite(got[n]).reshape(M, -1).all(axis=1) & ins
        if bad.any():
            msgs.append(f"{n} not finite on elements {np.flatnonzero(bad)[:8].tolist()} x {x64[bad][:8].tolist()}")
    exact_out = (np.array_equal(got["out"][out], x64[out]) and (got["lad"][out] == 0).all()
                 and np.array_equal(got["g_x"][out], c.wo.double().numpy()[out])
                 and all((got[n][out] == 0).all() for n in ("g_uw", "g_uh", "g_ud")))
    if not exact_out:
        msgs.append("outside elements are not the exact identity")
    return msgs + rule1_failures(c, got, C_ENV_S * factor / 4) + rule2_failures(c, got, factor)


def admissible(c):
    """(ok, detail): the conditions on a seed, on the reference and the yardstick alone."""
    ratios = {n: env_ratio(c, c.yard, n) for n in RULE1}
    ins = ~c.outside
    finite = all(np.isfinite(c.yard[n]).reshape(M, -1).all(axis=1)[ins].all() for n in NAMES)
    detail = dict(ratios=ratios, excluded=c.excluded.mean(), flip=c.flip.mean(), finite=finite)
    ok = (finite and c.excluded.mean() <= MAX_EXCLUDED and c.flip.mean() <= MAX_EXCLUDED
          and max(ratios.values()) <= RATIO_CAP)
    return ok, detail
