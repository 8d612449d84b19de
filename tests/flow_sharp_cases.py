"""Weights, inputs, references and the row check shared by test_flow_sharp_cpu.py and
test_gpu_flow_sharp.py: the inference flow passes (csrc/flow_device.h: knots_from_logits,
rqs_eval, the bin search, softplus_t, the inside test) on SHARP splines and boundary inputs.

Every other flow test builds near-identity weights (oracle.flow.random_state_dict with
final_std <= 0.05, uncond_std = 0.3: bins of nearly equal width, derivatives near 1).  Here
the conditioner's logits are O(1) .. O(10), and layers 0 and L - 1 carry planted extremes:
K - 1 bins at the MIN_W / MIN_H floor, derivative logits beyond the softplus threshold and
derivatives at MIN_D, a circular end derivative far from 1.

The reference is the oracle evaluated in float64 on the float32 inputs and up-cast weights.
A sharp layer amplifies the float32 rounding of a latent by the bin slope (up to ~1e3), so
no fixed tolerance holds; the bound follows each row's conditioning:

    |got - exact| <= base + C_ENV * env

base: the project's existing bound for the quantity (tests/test_gpu_flow.py); env: how far
the float64 value itself moves when the input moves by one float32 ulp of B per coordinate
(8 seeded sign patterns).  C_ENV is measured on the float32 oracle, not on the kernels (see
C_ENV below).  Rows on which an input coordinate or a layer's output lies within 64 ulp(B) of
+-B are boundary rows: there the inside test of the next layer (and the base density's -inf)
legitimately depends on rounding.

Everything here runs on the CPU and is computed once per case."""
import functools

import numpy as np
import torch

from oracle import flow as OF

EPS32 = 2.0 ** -23
ROWS = 200            # three full 64-row groups and a ragged tail
KNOT_ROWS = 16        # eight straddling pairs on knots of the first unconditional spline of the pass
MARGIN_ULPS = 64      # interior: margin > MARGIN_ULPS * B * 2^-23
N_PERTURB = 8

# (N, L, H, nb, K): the smallest shape of each instantiated kernel family ...
SHAPES = [(3, 2, 32, 2, 5),
          (16, 3, 64, 2, 8),
          (15, 2, 128, 2, 15),    # odd N: the last feature pair holds one feature
          (4, 2, 256, 2, 32),
          (64, 2, 128, 2, 15)]
# ... and shapes only the general-shape kernels accept
GENERAL_ONLY = [(5, 2, 96, 1, 10), (3, 2, 24, 1, 7)]
ALL_SHAPES = SHAPES + GENERAL_ONLY

# Weight seed per shape: the first seed (1, 2, ...) that is ADMISSIBLE, all measured on the
# oracle alone (test_flow_sharp_cpu.py re-checks every condition on the seed kept here):
#   * at least 80 % of the rows interior, in both directions;
#   * the float32 oracle finite on every interior row;
#   * RATIO_CAP: the float32 oracle's own (err - base) / env at most 8 on every interior row.
# The last one keeps out weights on which the float32 oracle is no yardstick: where its
# (err - base) / env is 35 .. 11000, no constant turns the envelope into a bound with teeth.
# Nearly all of those are the sampling log det, and the cause is the reference's own inverse
# root, not the envelope (see "cases the reference's own float32 root cannot serve ..." at the
# end of this file, which also tests two of the rejected seeds).  The cap of 8 is a choice: 2 x
# the factor 4 that C_ENV leaves the kernels; with it C_ENV cannot exceed 32.
RATIO_CAP = 8.0
SD_SEEDS = {(3, 2, 32, 2, 5): 1, (16, 3, 64, 2, 8): 7, (15, 2, 128, 2, 15): 1, (4, 2, 256, 2, 32): 2,
            (64, 2, 128, 2, 15): 32, (5, 2, 96, 1, 10): 1, (3, 2, 24, 1, 7): 2}

# C_ENV: 4 x the largest (err_ref32 - base) / env the float32 ORACLE shows on interior rows
# over all cases, both directions and every checked quantity, rounded up to a power of two.
# The factor 4: the kernels' operation order differs from the oracle's (knots in double,
# exp2, MFMA accumulation), and 8 perturbations sample the sensitivity without bounding it.
# Measured per case (log q, density log det, latents z, samples x, sampling log det;
# test_flow_sharp_cpu.py::test_c_env_is_the_measured_one prints and re-derives them):
C_ENV_RATIOS = {   # shape: (lq, ldd, z, x, ld); 0: the float32 oracle within base on every row
    (3, 2, 32, 2, 5): (3.72, 3.72, 1.06, 0.43, 1.04),
    (16, 3, 64, 2, 8): (1.76, 1.76, 0.00, 0.00, 1.95),
    (15, 2, 128, 2, 15): (6.38, 6.39, 4.73, 0.11, 4.57),
    (4, 2, 256, 2, 32): (1.68, 1.68, 0.00, 0.00, 0.48),
    (64, 2, 128, 2, 15): (2.25, 2.25, 2.17, 0.00, 0.81),
    (5, 2, 96, 1, 10): (5.12, 5.12, 3.25, 0.01, 1.29),
    (3, 2, 24, 1, 7): (6.27, 6.26, 2.97, 0.00, 0.50)}
C_ENV = 32.0        # 4 x 6.39 = 25.6, rounded up to a power of two

# base bounds (tests/test_gpu_flow.py): (rtol on |exact|, atol in units of 1, atol in units of B)
BASE = {"lq": (1e-5, 1e-4, 0.0),      # log q, and the density direction's log det
        "z": (0.0, 0.0, 2e-4),        # latents of the density direction
        "x": (0.0, 0.0, 5e-4),        # samples
        "ld": (1e-4, 1e-3, 0.0)}      # the sampling direction's log det


def dims_of(shape):
    N, L, H, nb, K = shape
    return OF.FlowDims(N=N, L=L, H=H, nb=nb, K=K, B=OF.half_box(N))


def _up(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


# --- weights ------------------------------------------------------------------------------------
def sharp_state_dict(dims, seed):
    """random_state_dict at final_std = 0.3, uncond_std = 3.0, with extremes planted on feature
    0 of the unconditional and of the conditional transform of layers 0 and L - 1:
      * width logit 0 at +12 over the others: bins 1 .. K - 1 at the MIN_W floor;
      * height logit K - 1 at +12 over the others: bins 0 .. K - 2 at the MIN_H floor
        (so bin 0 has slope ~1e-3 and bin K - 1 slope ~1e3);
      * derivative logits +25 (slot 0: beyond the softplus threshold), -25 (slot 1: the
        derivative is MIN_D) and 3 (slot K, the end derivative: neither ~1 nor d[0].  The
        reference's circular pad ties nothing: its derivative rows have K + 1 columns, the pad
        writes column K + 1, which no bin reads, oracle.flow.rqs; so d[K] is a parameter of
        its own, and a kernel that copied d[0] into it would be wrong).
    The conditional ones go through final_layer.bias (widths and heights are divided by
    sqrt(H) after the layer, so they are planted times sqrt(H))."""
    K, H = dims.K, dims.H
    sd = OF.random_state_dict(dims, seed, final_std=0.3, uncond_std=3.0)
    rH = float(np.sqrt(H))
    for i in sorted({0, dims.L - 1}):
        p = f"flows.{i}.prqct."
        uw = sd[p + "unconditional_transform.unnormalized_widths"]
        uh = sd[p + "unconditional_transform.unnormalized_heights"]
        ud = sd[p + "unconditional_transform.unnormalized_derivatives"]
        uw[0, :] = 0.0
        uw[0, 0] = 12.0
        uh[0, :] = 0.0
        uh[0, K - 1] = 12.0
        ud[0, 0] = 25.0
        ud[0, 1] = -25.0
        ud[0, K] = 3.0
        b = sd[p + "transform_net.final_layer.bias"]   # feature 0: [0, 3K + 1)
        b[0:2 * K] = 0.0
        b[0] = 12.0 * rH
        b[2 * K - 1] = 12.0 * rH
        b[2 * K] = 25.0
        b[2 * K + 1] = -25.0
        b[3 * K] = 3.0
    return sd


def _knots64(u, B):
    """(..., K + 1) float64 knots from logits, by rqs_core's own formulas (MIN_W == MIN_H)."""
    K = u.shape[-1]
    w = OF.MIN_W + (1 - OF.MIN_W * K) * torch.softmax(u.double(), dim=-1)
    c = torch.nn.functional.pad(torch.cumsum(w, dim=-1), pad=(1, 0), mode="constant", value=0.0)
    c = 2 * B * c - B
    c[..., 0] = -B
    c[..., -1] = B
    return c


def uncond_knots(sd, layer, dims, inverse):
    """(N, K + 1) float64 knots of a layer's unconditional spline on the side its input is
    searched on (widths in the density direction, heights in the sampling direction)."""
    p = f"flows.{layer}.prqct.unconditional_transform."
    return _knots64(sd[p + ("unnormalized_heights" if inverse else "unnormalized_widths")], dims.B)


# --- inputs -------------------------------------------------------------------------------------
PLANTED = ("plusB", "minusB", "zero", "negzero", "outside", "insideB", "lastbin_mid", "firstbin_mid")


def _other_side(v32, exact):
    """The float32 neighbour of v32 on the other side of exact (v32 itself if it is exact)."""
    if float(v32) == exact:
        return v32
    return np.nextafter(v32, np.float32(np.inf if float(v32) < exact else -np.inf))


def sharp_inputs(dims, rows, seed, sd=None, direction="density"):
    """(rows, D) float32: uniform rows in [-B, B], then KNOT_ROWS knot rows, then the PLANTED
    rows (the last len(PLANTED) rows):
      plusB / minusB   every coordinate fl32(B) / -fl32(B)
      zero / negzero   every coordinate 0.0 / -0.0
      outside          a uniform row with one coordinate nextafter(fl32(B), +inf)
      insideB          every coordinate nextafter(fl32(B), 0)
      lastbin_mid / firstbin_mid   a uniform row with the planted spline's (identity feature
                       0 of the layer named below) coordinate in the middle of its last / first bin
    The knot rows come in pairs: the identity-feature coordinates of the first are float32
    roundings of interior knots of the unconditional spline of the first layer the pass
    applies (layer L - 1, widths, in the density direction; layer 0, heights, behind the half
    rotation, in the sampling direction; float64 knots by rqs_core's formulas), those of the
    second the float32 neighbours on the other side of the same knots, so every planted knot
    is straddled.  Pair q puts feature f on knot 1 + (q + f - 1) % (K - 1): pair 0 has
    feature 0 (the planted spline) on the last interior knot.

    Returns (x, info): info["planted"][name] -> row index, info["knot_rows"] -> slice,
    info["outside_coord"] -> the coordinate of the "outside" row that is beyond +B."""
    D, N, K = dims.D, dims.N, dims.K
    B32 = np.float32(dims.B)
    g = torch.Generator().manual_seed(int(seed))
    x = ((torch.rand((rows, D), generator=g, dtype=torch.float64) * 2 - 1) * dims.B).float()
    x.clamp_(-float(B32), float(B32))
    first_pl = rows - len(PLANTED)
    planted = {name: first_pl + i for i, name in enumerate(PLANTED)}
    x[planted["plusB"]] = float(B32)
    x[planted["minusB"]] = -float(B32)
    x[planted["zero"]] = 0.0
    x[planted["negzero"]] = -0.0
    oc = 3 % D
    x[planted["outside"], oc] = float(np.nextafter(B32, np.float32(np.inf)))
    x[planted["insideB"]] = float(np.nextafter(B32, np.float32(0)))
    knot_rows = slice(first_pl - KNOT_ROWS, first_pl)
    if sd is not None:
        inverse = direction == "sample"
        kn = uncond_knots(sd, 0 if inverse else dims.L - 1, dims, inverse)   # (N, K + 1)
        for f in range(N):
            # identity feature f reads coordinate 2 f (in the sampling direction behind the
            # half rotation: rolled[j] = z[(j + N) % D])
            pos = (2 * f + N) % D if inverse else 2 * f
            for j, r in enumerate(range(knot_rows.start, knot_rows.stop)):
                exact = kn[f, 1 + (j // 2 + f - 1) % (K - 1)].item()
                v = np.float32(exact)
                x[r, pos] = float(_other_side(v, exact) if j % 2 else v)
            if f == 0:   # the planted spline; the row's other coordinates stay uniform
                x[planted["lastbin_mid"], pos] = float(np.float32(0.5 * (kn[f, K - 1].item() + kn[f, K].item())))
                x[planted["firstbin_mid"], pos] = float(np.float32(0.5 * (kn[f, 0].item() + kn[f, 1].item())))
    return x, dict(planted=planted, knot_rows=knot_rows, outside_coord=oc)


def final_position(p, dims):
    """Where a coordinate that passes through every layer untouched ends up: each layer, in
    either direction, rotates the coordinates by half (new[j] = old[(j + N) % D])."""
    return (p - dims.L * dims.N) % dims.D


# --- references ---------------------------------------------------------------------------------
def _sample_trace(sd, z, dims):
    lps = [OF.layer_params(sd, i) for i in range(dims.L)]
    ld_tot = torch.zeros(len(z), dtype=z.dtype)
    trace = []
    for i in range(dims.L):
        z, ld = OF.coupling_sample(lps[i], z, dims)
        ld_tot += ld.view(-1)
        trace.append(z.clone())
    return z, ld_tot, trace


def _margin(first, trace, B):
    m = (B - first.abs()).min(dim=1).values
    for t in trace:
        m = torch.minimum(m, (B - t.abs()).min(dim=1).values)
    return m.numpy()


def _signs(shape, seed):
    g = torch.Generator().manual_seed(int(seed))
    return [(torch.randint(0, 2, shape, generator=g).double() * 2 - 1) for _ in range(N_PERTURB)]


def _absdiff(a, b):
    """|a - b|, with non-finite differences (a perturbed row leaving the box) as +inf."""
    d = (a - b).abs()
    return torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))


class Ref:
    """One case: the float64 and float32 oracle values of both directions, each row's margin
    and sensitivity envelope."""


@torch.no_grad()
def reference(sd, x, dims, z0=None, seed=0):
    """Float64 oracle values (log_prob with per_layer=True on x; sample_from with its log det
    on z0), the float32 oracle's, and per row: margin (smallest distance to +-B of any input
    coordinate and any layer's float64 output) and env (largest |change| of the float64 value
    over N_PERTURB copies of the input moved by +-B 2^-23 per coordinate, clamped to the box).

    The float64 oracle reads x.double() with coordinates that are inside the float32 box
    (|x| <= fl32(B)) clamped to [-B, B]: fl32(B) may exceed B by half an ulp, and the planted
    +-B rows are meant to sit ON the bound, not outside it."""
    B = dims.B
    B32 = float(np.float32(B))
    sd64 = _up(sd)
    r = Ref()
    r.dims, r.x, r.z0 = dims, x, z0
    step = B * EPS32

    def to64(v):
        v64 = v.double()
        return torch.where(v.abs() <= B32, v64.clamp(-B, B), v64)

    # density direction
    x64 = to64(x)
    r.outside = (x.abs() > B32).any(dim=1).numpy()
    lq, z, trace = OF.log_prob(sd64, x64.clone(), dims, per_layer=True)
    r.lq64, r.z64 = lq.numpy(), z.numpy()
    r.ldd64 = sum(t[1] for t in trace).numpy()            # the log det without the base term
    r.margin = _margin(x64, [t[0] for t in trace], B)
    r.interior = (r.margin > MARGIN_ULPS * step) & ~r.outside
    lq32, z32, tr32 = OF.log_prob(sd, x.clone(), dims, per_layer=True)
    r.lq32, r.z32 = lq32.double().numpy(), z32.double().numpy()
    r.ldd32 = sum(t[1] for t in tr32).double().numpy()
    env = torch.zeros(len(x), dtype=torch.float64)
    env_z = torch.zeros(len(x), dtype=torch.float64)
    for s in _signs(x.shape, 1000 + seed):
        xp = (x64 + step * s).clamp(-B, B)
        lqp, zp, _ = OF.log_prob(sd64, xp, dims, per_layer=True)
        env = torch.maximum(env, _absdiff(lqp, lq))
        env_z = torch.maximum(env_z, _absdiff(zp, z).max(dim=1).values)
    r.env, r.env_z = env.numpy(), env_z.numpy()
    if z0 is None:
        return r
    # sampling direction
    z064 = to64(z0)
    r.outside_s = (z0.abs() > B32).any(dim=1).numpy()
    xs, ld, trace = _sample_trace(sd64, z064.clone(), dims)
    r.xs64, r.ld64 = xs.numpy(), ld.numpy()
    r.margin_s = _margin(z064, trace, B)
    r.interior_s = (r.margin_s > MARGIN_ULPS * step) & ~r.outside_s
    xs32, ld32 = OF.sample_from(sd, z0.clone(), dims, with_logdet=True)
    r.xs32, r.ld32 = xs32.double().numpy(), ld32.double().numpy()
    env_x = torch.zeros(len(z0), dtype=torch.float64)
    env_ld = torch.zeros(len(z0), dtype=torch.float64)
    for s in _signs(z0.shape, 2000 + seed):
        zp = (z064 + step * s).clamp(-B, B)
        xp, lp, _ = _sample_trace(sd64, zp, dims)
        env_x = torch.maximum(env_x, _absdiff(xp, xs).max(dim=1).values)
        env_ld = torch.maximum(env_ld, _absdiff(lp, ld))
    r.env_x, r.env_ld = env_x.numpy(), env_ld.numpy()
    # the way back from the exact samples (round trip): the density direction's sensitivity there
    env_rt = torch.zeros(len(z0), dtype=torch.float64)
    for s in _signs(z0.shape, 3000 + seed):
        xp = (xs + step * s).clamp(-B, B)
        zp = OF.log_prob(sd64, xp, dims, per_layer=True)[1]
        env_rt = torch.maximum(env_rt, _absdiff(zp, z064).max(dim=1).values)
    r.env_rt = env_rt.numpy()
    return r


def round_trip_bound(ref, c_env=None):
    """Per row: the samples' bound plus the latents' bound at the samples (the sum of the two)."""
    c_env = C_ENV if c_env is None else c_env
    B = ref.dims.B
    with np.errstate(invalid="ignore"):
        return (BASE["x"][2] * B + c_env * ref.env_x) + (BASE["z"][2] * B + c_env * ref.env_rt)


# what check_rows reads per kind: exact, float32 oracle, envelope, interior mask, outside mask
_KIND = {"lq": ("lq64", "lq32", "env", "interior", "outside", "lq"),
         "ldd": ("ldd64", "ldd32", "env", "interior", "outside", "lq"),
         "z": ("z64", "z32", "env_z", "interior", "outside", "z"),
         "x": ("xs64", "xs32", "env_x", "interior_s", "outside_s", "x"),
         "ld": ("ld64", "ld32", "env_ld", "interior_s", "outside_s", "ld")}


def fields(ref, kind):
    e, r32, env, inter, out, base = _KIND[kind]
    return (getattr(ref, e), getattr(ref, r32), getattr(ref, env), getattr(ref, inter), getattr(ref, out), BASE[base])


def bound_of(ref, kind, c_env=None):
    """Per row (per element for the vector kinds): base + c_env * env."""
    c_env = C_ENV if c_env is None else c_env
    exact, _, env, _, _, (rtol, atol, atol_b) = fields(ref, kind)
    if kind == "ldd":   # log q without its constant: the bound is log q's
        exact = exact - ref.dims.D * np.log(2 * ref.dims.B)
    with np.errstate(invalid="ignore"):
        base = rtol * np.abs(exact) + atol + atol_b * ref.dims.B
        e = c_env * env
    return base + (e[:, None] if exact.ndim == 2 else e)


def row_errors(got, ref, kind):
    """|got - exact| per row (per element for the vector kinds), non-finite differences as +inf."""
    exact = fields(ref, kind)[0]
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - exact)
    return np.where(np.isfinite(err), err, np.inf)


def escaped_rows(vec, ref):
    """Rows of a pass's vector output (latents z or samples x) with a coordinate beyond
    +-fl32(B): the pass itself shows that it passed a coordinate through (a coordinate that
    leaves the box at some layer is the identity in every later one, so it is still outside at
    the end; inside the box no spline puts one out except by rounding at the very edge)."""
    return (np.abs(np.asarray(vec, np.float64)) > float(np.float32(ref.dims.B))).any(axis=1)


def failing_rows(got, ref, kind, c_env=None, escaped=None):
    """Boolean per row: the row breaks check_rows' rule for its class.
      interior: got finite and every element within base + c_env * env of the exact value;
      boundary: the same, unless the row demonstrably took a pass-through: log q is -inf, or
                (other kinds) the same pass's vector output has a coordinate beyond +-fl32(B)
                (`escaped`, from escaped_rows; for the vector kinds it is read off `got`).
                What follows a pass-through is another function, so only finiteness is left to
                check there; never NaN, never +inf;
      outside (an input coordinate beyond +-fl32(B)): log q exactly -inf, the rest finite.  (That
                the untouched coordinate comes out bit-equal is checked by the caller.)"""
    exact, _, _, interior, outside, _ = fields(ref, kind)
    got = np.asarray(got, np.float64)
    vec = exact.ndim == 2
    err = row_errors(got, ref, kind)
    with np.errstate(invalid="ignore"):
        within = err <= bound_of(ref, kind, c_env)
    fin_row = np.isfinite(got)
    if vec:
        within, fin_row = within.all(axis=1), fin_row.all(axis=1)
        escaped = escaped_rows(got, ref) if escaped is None else escaped
        bad_value = ~fin_row
    elif kind == "lq":
        escaped = np.isneginf(got)
        bad_value = np.isnan(got) | np.isposinf(got)
    else:
        escaped = np.zeros(len(got), bool) if escaped is None else escaped
        bad_value = ~fin_row
    ok = within & fin_row
    fail = np.where(interior, ~ok, ~(ok | escaped)) | bad_value
    if kind == "lq":
        return np.where(outside, ~np.isneginf(got), fail)
    return np.where(outside, bad_value, fail)


def check_rows(got, ref, kind, c_env=None, label="", escaped=None):
    fail = failing_rows(got, ref, kind, c_env, escaped)
    if fail.any():
        err = row_errors(got, ref, kind)
        bnd = bound_of(ref, kind, c_env)
        if err.ndim == 2:
            err, bnd = err.max(axis=1), bnd.min(axis=1)
        inter = fields(ref, kind)[3]
        rows = np.flatnonzero(fail)[:8]
        raise AssertionError(
            f"{label} {kind}: {fail.sum()} / {fail.size} rows fail; rows {rows.tolist()} interior "
            f"{inter[rows].tolist()} err {err[rows].tolist()} bound {bnd[rows].tolist()} "
            f"got {np.asarray(got)[rows].tolist() if np.ndim(got) == 1 else ''}")


def env_ratio(ref, kind):
    """max over interior rows of (err_ref32 - base) / env: what C_ENV is measured from."""
    exact, r32, env, interior, _, _ = fields(ref, kind)
    err = row_errors(r32, ref, kind)
    base = bound_of(ref, kind, 0.0)
    exc = err - base
    if exc.ndim == 2:
        exc = exc.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(exc > 0, exc / env, 0.0)
    return float(ratio[interior].max())


def median_error(got, ref, kind):
    """Median over interior rows of |got - exact| (per row: the largest element)."""
    err = row_errors(got, ref, kind)
    if err.ndim == 2:
        err = err.max(axis=1)
    return float(np.median(err[fields(ref, kind)[3]]))


# --- the regime the cases claim -------------------------------------------------------------------
@torch.no_grad()
def regime(sd, x, dims, direction="density"):
    """What the float64 trace of a pass evaluates, over every layer, spline and row inside the
    box: the smallest evaluated bin width and height (in units of the floor, 2 B MIN_W), the
    largest derivative logit, the smallest evaluated derivative (in units of MIN_D) and how
    many evaluations land on the first and on the last bin."""
    sd64 = _up(sd)
    B, K, H = dims.B, dims.K, dims.H
    inverse = direction == "sample"
    out = dict(min_w=np.inf, min_h=np.inf, max_ud=-np.inf, min_d=np.inf, first_bin=0, last_bin=0)

    def note(v, uw, uh, ud):
        _, _, bins = OF.rqs(v, uw, uh, ud, B, inverse, return_bins=True)
        ok = bins >= 0
        b = bins.clamp(min=0)[..., None]
        cw, ch = _knots64(uw, B), _knots64(uh, B)
        w = (cw[..., 1:] - cw[..., :-1]).gather(-1, b)[..., 0][ok]
        h = (ch[..., 1:] - ch[..., :-1]).gather(-1, b)[..., 0][ok]
        d = OF.MIN_D + torch.nn.functional.softplus(ud)   # K + 1 columns: d[K] is its own
        dd = torch.minimum(d.gather(-1, b)[..., 0], d.gather(-1, b + 1)[..., 0])[ok]
        out["min_w"] = min(out["min_w"], float(w.min()) / (2 * B * OF.MIN_W))
        out["min_h"] = min(out["min_h"], float(h.min()) / (2 * B * OF.MIN_H))
        out["max_ud"] = max(out["max_ud"], float(ud.max()))
        out["min_d"] = min(out["min_d"], float(dd.min()) / OF.MIN_D)
        out["first_bin"] += int((bins == 0).sum())
        out["last_bin"] += int((bins == K - 1).sum())

    v = x.double().clamp(-B, B)
    order = range(dims.L) if inverse else range(dims.L - 1, -1, -1)
    for i in order:
        lp = OF.layer_params(sd64, i)
        u = torch.cat([v[:, dims.N:], v[:, :dims.N]], dim=1) if inverse else v
        ident, trans = u[:, lp["idf"]], u[:, lp["trf"]]
        n = len(u)
        ex = lambda t: t[None, ...].expand(n, *t.shape)   # noqa: E731
        note(ident, ex(lp["uw"]), ex(lp["uh"]), ex(lp["ud"]))
        cond_in = OF.rqs(ident, ex(lp["uw"]), ex(lp["uh"]), ex(lp["ud"]), B, True)[0] if inverse else ident
        p = OF.conditioner(lp, cond_in, B).reshape(n, dims.N, -1)
        note(trans, p[..., :K] / np.sqrt(H), p[..., K:2 * K] / np.sqrt(H), p[..., 2 * K:])
        v = OF.coupling_sample(lp, v, dims)[0] if inverse else OF.coupling_density(lp, v, dims)[0]
    return out


# --- cases --------------------------------------------------------------------------------------
X_SEED, Z_SEED = 17, 29


@functools.lru_cache(maxsize=None)
def case(shape, rows=ROWS, sd_seed=None):
    """(dims, sd, ref, info_x, info_z) of one shape, computed once and read only."""
    dims = dims_of(shape)
    sd = sharp_state_dict(dims, SD_SEEDS[shape] if sd_seed is None else sd_seed)
    x, info_x = sharp_inputs(dims, rows, X_SEED, sd, "density")
    z0, info_z = sharp_inputs(dims, rows, Z_SEED, sd, "sample")
    ref = reference(sd, x, dims, z0)
    return dims, sd, ref, info_x, info_z


# --- cases the reference's own float32 root cannot serve as a yardstick for --------------------------
# Two defects of the reference's inverse (sampling direction), both fixed in rqs_eval, both the
# reason most seeds fail the admission rule above (the float32 ORACLE's sampling log det):
#   * unstable root: 2 c / (-b - sqrt(disc)) with b < 0 (a flat bin between larger end
#     derivatives, towards its top) subtracts two nearly equal numbers; the root is off by ~1e-5,
#     the log det by 0.05 .. 0.3.  Float32 oracle (err - base) / env at the seeds below: log det
#     8314 and 11455 at (16, 3, 64, 2, 8) seeds 1 and 5, 2943 at N = 64 seed 7; with the root in
#     its other form, (-b + sqrt(disc)) / (2 a), for b < 0: 0.99, 0.74, 0.74.
#   * root > 1: in a steep bin b^2 - 4 a c cancels towards the bin's top, the root passes 1 by
#     ~1e-4 and the log det is the logarithm of a negative number (N = 64 seed 4: NaN on an
#     interior row; 10 of the first 32 seeds at N = 64).
# Admission counts (first admissible seed last): (16, 3, 64, 2, 8) rejects 6 of the first 7 seeds,
# (64, 2, 128, 2, 15) 31 of the first 32 (8 for fewer than 80 % interior rows in the density
# direction, the others for the sampling log det; a few also for a density ratio above the cap).
# The extra cases below are such rejected seeds, for the sampling direction only: the first seed
# at N = 64 with a NaN, and the first seed at (16, 3, 64, 2, 8) with an unstable root.  Their
# float32 yardstick is the oracle with the kernels' root (stable form, pinned), held to the same
# RATIO_CAP, so C_ENV stands.
EXTRA_CASES = {"nan-root": ((64, 2, 128, 2, 15), 4), "unstable-root": ((16, 3, 64, 2, 8), 1)}


def _rqs_core_kernel_root(x, uw, uh, ud, left, right, bottom, top, inverse):
    """oracle.flow.rqs_core with the inverse's root as the kernels take it (flow_device.h
    rqs_eval): the cancellation-free form of the same root for b < 0, pinned to [0, 1].  The
    forward map is the oracle's own."""
    if not inverse:
        return _RQS_CORE(x, uw, uh, ud, left, right, bottom, top, inverse)
    F = torch.nn.functional
    K = uw.shape[-1]

    def knots(u, lo, hi, minb):
        w = minb + (1 - minb * K) * F.softmax(u, dim=-1)
        c = F.pad(torch.cumsum(w, dim=-1), pad=(1, 0), mode="constant", value=0.0)
        c = (hi - lo) * c + lo
        c[..., 0] = lo
        c[..., -1] = hi
        return c, c[..., 1:] - c[..., :-1]

    cw, w = knots(uw, left, right, OF.MIN_W)
    ch, h = knots(uh, bottom, top, OF.MIN_H)
    d = OF.MIN_D + F.softplus(ud)
    ch[..., -1] += 1e-6
    b = (torch.sum(x[..., None] >= ch, dim=-1) - 1)[..., None]
    g = lambda t: t.gather(-1, b)[..., 0]   # noqa: E731
    icw, ibw, ich, idl, id0, id1, ih = g(cw), g(w), g(ch), g(h / w), g(d), g(d[..., 1:]), g(h)
    s = id0 + id1 - 2 * idl
    a = (x - ich) * s + ih * (idl - id0)
    bb = ih * id0 - (x - ich) * s
    c = -idl * (x - ich)
    disc = abs(bb.pow(2) - 4 * a * c)
    sq = torch.sqrt(disc)
    root = torch.where(bb >= 0, (2 * c) / (-bb - sq), (sq - bb) / (2 * a)).clamp(0, 1)
    out = root * ibw + icw
    tomt = root * (1 - root)
    den = idl + s * tomt
    dnum = idl.pow(2) * (id1 * root.pow(2) + 2 * idl * tomt + id0 * (1 - root).pow(2))
    return out, -(torch.log(dnum) - 2 * torch.log(den)), b[..., 0]


_RQS_CORE = OF.rqs_core


@functools.lru_cache(maxsize=None)
def extra_case(name):
    """(dims, sd, ref, bad_rows) of an extra case (sampling direction).  ref.xs32 / ref.ld32 are
    the float32 oracle's with the kernels' root; ref.xs32_ref / ref.ld32_ref the oracle's own;
    bad_rows: interior rows where the oracle's own log det is NaN or beyond base + C_ENV * env."""
    shape, seed = EXTRA_CASES[name]
    dims = dims_of(shape)
    sd = sharp_state_dict(dims, seed)
    x, _ = sharp_inputs(dims, ROWS, X_SEED, sd, "density")
    z0, _ = sharp_inputs(dims, ROWS, Z_SEED, sd, "sample")
    ref = reference(sd, x, dims, z0)
    bad = failing_rows(ref.ld32, ref, "ld", escaped=escaped_rows(ref.xs32, ref)) & ref.interior_s
    ref.xs32_ref, ref.ld32_ref = ref.xs32, ref.ld32
    OF.rqs_core = _rqs_core_kernel_root
    try:
        xs32, ld32 = OF.sample_from(sd, z0.clone(), dims, with_logdet=True)
    finally:
        OF.rqs_core = _RQS_CORE
    ref.xs32, ref.ld32 = xs32.double().numpy(), ld32.double().numpy()
    return dims, sd, ref, bad
