"""The sharp-spline flow cases (tests/flow_sharp_cases.py) proved on the oracle alone, no GPU:
the fixtures reach the regime they claim, the float32 oracle passes the row check with a
quarter of C_ENV, C_ENV is the measured constant, and the check has teeth: a float32 oracle
with a wrong MIN_D, MIN_W or MIN_H, or with the end derivative tied to d[0], fails it."""
import math

import numpy as np
import pytest
import torch

import flow_sharp_cases as FC
from oracle import flow as OF

KINDS = ("lq", "ldd", "z", "x", "ld")


@pytest.mark.parametrize("shape", FC.ALL_SHAPES, ids=str)
def test_fixture_conditions(shape):
    dims, sd, ref, info_x, info_z = FC.case(shape)
    # at least 80 % of the rows interior, and the float32 oracle finite on each of them
    for inter, vals in ((ref.interior, (ref.lq32, ref.z32)), (ref.interior_s, (ref.xs32, ref.ld32))):
        assert inter.sum() >= 0.8 * FC.ROWS, inter.sum()
        for v in vals:
            assert np.isfinite(v[inter]).all()
    # the planted rows are what they are named
    pl = info_x["planted"]
    assert np.isneginf(ref.lq64[pl["outside"]]) and ref.outside[pl["outside"]] and ref.outside.sum() == 1
    assert ref.lq64[pl["zero"]] == ref.lq64[pl["negzero"]] and ref.interior[pl["zero"]]
    assert torch.signbit(ref.x[pl["negzero"]]).all() and not torch.signbit(ref.x[pl["zero"]]).any()
    for name in ("plusB", "minusB", "insideB"):
        assert not ref.interior[pl[name]] and not ref.outside[pl[name]]
    assert ref.interior[pl["lastbin_mid"]] and ref.interior[pl["firstbin_mid"]]
    for r, info in ((ref.interior, info_x), (ref.interior_s, info_z)):
        assert r[info["knot_rows"]].sum() >= 8
    # the regime, on the float64 trace of each direction
    for direction, v in (("density", ref.x), ("sample", ref.z0)):
        got = FC.regime(sd, v[~(ref.outside if direction == "density" else ref.outside_s)], dims, direction)
        print(shape, direction, got)
        assert got["min_w"] <= 1.05 and got["min_h"] <= 1.05, got
        assert got["max_ud"] > 20 and got["min_d"] < 1.01, got
        assert got["first_bin"] >= 1 and got["last_bin"] >= 1, got


@pytest.mark.parametrize("shape", FC.ALL_SHAPES, ids=str)
def test_knot_rows_straddle_their_knots(shape):
    """Each pair of knot rows has the planted spline's (feature 0) coordinate on both sides of
    (or on) its float64 knot, one float32 apart."""
    dims, sd, ref, info_x, info_z = FC.case(shape)
    for v, info, inverse, pos in ((ref.x, info_x, False, 0), (ref.z0, info_z, True, dims.N % dims.D)):
        kn = FC.uncond_knots(sd, 0 if inverse else dims.L - 1, dims, inverse)[0]
        rows = range(info["knot_rows"].start, info["knot_rows"].stop, 2)
        for q, r in enumerate(rows):
            k = kn[1 + (q - 1) % (dims.K - 1)].item()
            a, b = float(v[r, pos]), float(v[r + 1, pos])
            assert min(a, b) <= k <= max(a, b)
            assert a == b == k or abs(np.float32(a) - np.float32(b)) == np.spacing(np.float32(min(abs(a), abs(b))))


def test_c_env_is_the_measured_one():
    """C_ENV = 4 x the float32 oracle's largest (err - base) / env over interior rows, every
    case, both directions, rounded up to a power of two; each case within RATIO_CAP."""
    worst = 0.0
    for shape in FC.ALL_SHAPES:
        ref = FC.case(shape)[2]
        ratios = {k: FC.env_ratio(ref, k) for k in KINDS}
        print(shape, {k: round(v, 2) for k, v in ratios.items()})
        assert max(ratios.values()) <= FC.RATIO_CAP, (shape, ratios)
        worst = max(worst, max(ratios.values()))
    assert FC.C_ENV == 2.0 ** math.ceil(math.log2(4 * worst)), worst


def _oracle_failures(ref, c_env):
    esc = {"ldd": FC.escaped_rows(ref.z32, ref), "ld": FC.escaped_rows(ref.xs32, ref)}
    return {k: FC.failing_rows(FC.fields(ref, k)[1], ref, k, c_env, esc.get(k)) for k in KINDS}


@pytest.mark.parametrize("shape", FC.ALL_SHAPES, ids=str)
def test_float32_oracle_passes_with_a_quarter_of_c_env(shape):
    """Every interior row of the float32 oracle is within base + C_ENV / 4 * env, and so is
    its round trip.  On boundary rows the float32 oracle itself may break the rule the kernels
    are held to (never NaN): with every coordinate at +B its sampling direction solves a root
    of 1 + a few ulp in a steep bin and takes the logarithm of a negative number (N = 64: log
    det NaN, x three ulp beyond +B).  Only such a NaN of its own on a boundary row is let
    through here."""
    dims, sd, ref, _, _ = FC.case(shape)
    for kind, fail in _oracle_failures(ref, FC.C_ENV / 4).items():
        inter = FC.fields(ref, kind)[3]
        assert not (fail & inter).any(), (kind, np.flatnonzero(fail & inter))
        r32 = FC.fields(ref, kind)[1]
        own_nan = np.isnan(r32).reshape(len(r32), -1).any(axis=1)
        assert not (fail & ~own_nan).any(), (kind, np.flatnonzero(fail & ~own_nan))
    xs32 = torch.from_numpy(ref.xs32).float()
    z = OF.log_prob(sd, xs32, dims, per_layer=True)[1].double().numpy()
    err = np.abs(z - ref.z0.double().numpy()).max(axis=1)
    i = ref.interior_s
    assert (err[i] <= FC.round_trip_bound(ref, FC.C_ENV / 4)[i]).all()


# --- the check has teeth ----------------------------------------------------------------------------
MUTANTS = {"MIN_D=0": ("MIN_D", 0.0), "MIN_W=0": ("MIN_W", 0.0), "MIN_H=2e-3": ("MIN_H", 2e-3)}


@pytest.mark.parametrize("mutant", MUTANTS, ids=str)
@pytest.mark.parametrize("shape", FC.ALL_SHAPES, ids=str)
def test_wrong_minimum_fails_the_check(shape, mutant, monkeypatch):
    """A float32 oracle with one spline minimum changed fails check_rows (full C_ENV) on more
    than 10 % of the interior rows, in the density direction (MIN_W = 0 makes the sampling
    direction's discriminant NaN, which raises)."""
    dims, sd, ref, _, _ = FC.case(shape)
    name, value = MUTANTS[mutant]
    monkeypatch.setattr(OF, name, value)
    lq = OF.log_prob(sd, ref.x.clone(), dims).double().numpy()
    fail = FC.failing_rows(lq, ref, "lq")
    frac = (fail & ref.interior).sum() / ref.interior.sum()
    print(shape, mutant, f"fails {frac:.2f} of the interior rows; median |err| "
          f"{np.median(np.abs(lq[ref.interior] - ref.lq64[ref.interior])):.2e}")
    assert frac > 0.10, frac
    with pytest.raises(AssertionError):
        FC.check_rows(lq, ref, "lq")


def _rqs_tied(x, uw, uh, ud, B, inverse, return_bins=False):
    """oracle.flow.rqs with the end derivative tied to the first one (d[K] = d[0]): what a
    kernel author who took "circular" at its word would write."""
    ud = ud.clone()
    ud[..., -1] = ud[..., 0]
    return _rqs(x, uw, uh, ud, B, inverse, return_bins)


def _rqs_unpadded(x, uw, uh, ud, B, inverse, return_bins=False):
    """oracle.flow.rqs without the copy into the pad column."""
    inside = (x >= -B) & (x <= B)
    out, lad = x.clone(), torch.zeros_like(x)
    ud_ = torch.nn.functional.pad(ud, pad=(0, 1))   # the pad column stays 0
    o, l, b = OF.rqs_core(x[inside], uw[inside, :], uh[inside, :], ud_[inside, :], -B, B, -B, B, inverse)
    out[inside], lad[inside] = o, l
    if return_bins:
        bins = torch.full_like(x, -1, dtype=torch.long)
        bins[inside] = b
        return out, lad, bins
    return out, lad


_rqs = OF.rqs


@pytest.mark.parametrize("shape", FC.ALL_SHAPES, ids=str)
def test_end_derivative_is_its_own_parameter(shape, monkeypatch):
    """The reference's circular pad ties nothing (its derivative rows have K + 1 columns; the
    pad writes column K + 1, which no bin reads): leaving the copy out changes no bit.  The
    mutant with teeth is the opposite one, d[K] = d[0]: it must fail on the planted row that
    sits in the middle of the last bin of the planted unconditional spline of the first layer
    (d[0] = 25, d[K] = 3), on every other interior row deep in that bin, and it moves the
    planted row with every coordinate one float inside +B (a boundary row) by more than 1."""
    dims, sd, ref, info_x, _ = FC.case(shape)
    monkeypatch.setattr(OF, "rqs", _rqs_unpadded)
    lq = OF.log_prob(sd, ref.x.clone(), dims).double().numpy()
    assert np.array_equal(lq, ref.lq32)
    monkeypatch.setattr(OF, "rqs", _rqs_tied)
    lq = OF.log_prob(sd, ref.x.clone(), dims).double().numpy()
    fail = FC.failing_rows(lq, ref, "lq")
    pl = info_x["planted"]
    bins = OF.rqs(ref.x[:, 0].double()[:, None], *[sd[f"flows.{dims.L - 1}.prqct.unconditional_transform." + n][None, :1].double()
                                                   .expand(len(ref.x), 1, -1) for n in
                                                   ("unnormalized_widths", "unnormalized_heights", "unnormalized_derivatives")],
                  dims.B, False, return_bins=True)[2][:, 0].numpy()
    assert bins[pl["lastbin_mid"]] == dims.K - 1
    # rows in the last bin of the planted spline, away from its left knot (there the slope is d[K - 1] alone)
    kn = FC.uncond_knots(sd, dims.L - 1, dims, False)[0]
    deep = (bins == dims.K - 1) & (ref.x[:, 0].double().numpy() > kn[dims.K - 1].item() + 0.05 * (dims.B - kn[dims.K - 1].item()))
    must = deep & ref.interior
    print(shape, "rows deep in the last bin and interior:", np.flatnonzero(must).tolist(), "failing:", int(fail[must].sum()))
    assert must[pl["lastbin_mid"]] and fail[must].all()
    assert abs(lq[pl["insideB"]] - ref.lq64[pl["insideB"]]) > 1.0


@pytest.mark.parametrize("name", FC.EXTRA_CASES, ids=str)
def test_extra_cases_need_the_kernels_root(name):
    """Rejected seeds (sampling direction): the float32 oracle's own log det is NaN or beyond
    the full envelope on interior rows; with the kernels' root (the stable form for b < 0,
    pinned to [0, 1]) it is finite on every interior row, within RATIO_CAP, and passes the row
    check with a quarter of C_ENV.  Measured: nan-root 1 bad row, ratios x 0 / log det 0.92;
    unstable-root ratios of the oracle's own x 204 / log det 8314, with the kernels' root
    0 / 0.99."""
    dims, sd, ref, bad = FC.extra_case(name)
    print(name, "bad rows of the oracle's own log det:", np.flatnonzero(bad).tolist())
    assert bad.sum() >= 1
    assert ref.interior_s.sum() >= 0.8 * FC.ROWS
    for kind in ("x", "ld"):
        assert np.isfinite(FC.fields(ref, kind)[1][ref.interior_s]).all()
        ratio = FC.env_ratio(ref, kind)
        print(name, kind, round(ratio, 2))
        assert ratio <= FC.RATIO_CAP and 4 * ratio <= FC.C_ENV
        fail = FC.failing_rows(FC.fields(ref, kind)[1], ref, kind, FC.C_ENV / 4, FC.escaped_rows(ref.xs32, ref))
        assert not (fail & ref.interior_s).any()
