"""The sharp-bin training-spline cases (tests/spline_sharp_cases.py) proved on the CPU alone: the
float64 reference is the restatement's float64, the fixtures reach the regime they claim and keep
their seeds' admission conditions, C_ENV_S is the measured constant, the float32 restatement
passes both rules with the kernels' factor 4 replaced by 1, and rule 1 has teeth: the restatement
with the reference's own inverse root fails it."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spline_sharp_cases as SC
from flowstate.normflows import autograd_flow as AF

IDS = [f"K{K}-{'inv' if inv else 'fwd'}" for K, inv in SC.CASES]


@pytest.mark.parametrize("K,inverse", SC.CASES, ids=IDS)
def test_reference_is_the_restatement_in_float64(K, inverse):
    c = SC.case(K, inverse)
    got = SC.values_and_grads(SC.restatement32(inverse), c.x, c.uw, c.uh, c.ud, c.wo, c.wl, dtype=torch.float64)
    AF.check_nan_flags()
    # (the restatement pins its root to [0, 1], the reference does not: on an excluded element,
    # y = +-B or a root within 1e-6 of the bin's end, a pinned root passes no gradient on)
    # Values on every element that is not left out (the restatement pins its root to [0, 1], the
    # reference does not); gradients on the elements whose bounds rest on them: on the planted knot pairs, a few
    # 1e-5 of a steep bin's width from its end, the two float64 gradients themselves differ by
    # up to 3e-8 (terms of ~1e8 cancel in the root's adjoint), and no bound uses them.
    for n in SC.NAMES:
        keep = ~c.excluded & ~(c.flip if n.startswith("g_") else False)
        np.testing.assert_allclose(got[n][keep], c.exact[n][keep], rtol=1e-9, atol=1e-9, err_msg=n)


@pytest.mark.parametrize("K,inverse", SC.CASES, ids=IDS)
def test_fixture_conditions(K, inverse):
    c = SC.case(K, inverse)
    ok, detail = SC.admissible(c)
    print(K, inverse, "seed", c.seed, detail)
    assert ok, detail
    # on the reference alone: what is left out of the bounds, and what sits on a knot
    assert c.excluded.sum() <= SC.MAX_EXCLUDED * SC.M and c.flip.sum() <= SC.MAX_EXCLUDED * SC.M
    pl, x = c.info["planted"], c.x.numpy()
    assert c.outside.sum() == 2 and c.outside[pl["just_outside"]] and c.outside[pl["far_outside"]]
    assert x[pl["plusB"]] == SC.B and x[pl["minusB"]] == -SC.B and c.boundary[pl["plusB"]] and c.boundary[pl["minusB"]]
    assert np.signbit(x[pl["negzero"]]) and not np.signbit(x[pl["zero"]]) and x[pl["negzero"]] == 0
    assert c.checked[pl["zero"]] and c.checked[pl["negzero"]]
    for n in SC.NAMES:
        assert np.array_equal(c.exact[n][pl["zero"]], c.exact[n][pl["negzero"]])
    assert c.bin[pl["firstbin_mid"]] == 0 and c.bin[pl["lastbin_mid"]] == K - 1
    assert c.grad_checked[pl["firstbin_mid"]] and c.grad_checked[pl["lastbin_mid"]]
    # the knot pairs straddle their knot, one float32 apart
    kp = c.info["knot_pairs"]
    if K > 1:
        assert c.flip[kp].all() and c.checked[kp].sum() >= 20
        kn = SC._knots((c.uh if inverse else c.uw).double(), None)[0].numpy()
        for q, r in enumerate(range(kp.start, kp.stop, 2)):
            k, a, b = kn[r, 1 + q % (K - 1)], x[r], x[r + 1]
            assert min(a, b) <= k <= max(a, b)
            assert a == b == k or abs(a - b) == np.spacing(np.float32(min(abs(a), abs(b))))
    # the regime: bins at the minimum size are evaluated, slopes of ~1e-3 and ~1e3, derivative
    # logits beyond the softplus threshold, derivatives at the minimum
    if K > 1:
        with torch.no_grad():
            w = SC._knots(c.uw.double(), None)[1].gather(1, torch.from_numpy(c.bin)[:, None])[:, 0].numpy()
            h = SC._knots(c.uh.double(), None)[1].gather(1, torch.from_numpy(c.bin)[:, None])[:, 0].numpy()
        ins = ~c.outside
        slope = (h / w)[ins]
        assert w[ins].min() <= 1.05 * 2 * SC.B * SC.MIN and h[ins].min() <= 1.05 * 2 * SC.B * SC.MIN
        assert slope.min() < 2e-3 and slope.max() > 5e2, (slope.min(), slope.max())
    ud_b = c.ud.numpy()[np.arange(SC.M), c.bin]
    assert ud_b.max() > 20
    assert (c.ud.numpy()[np.arange(SC.M), c.bin + 1] < -20).any() or K == 1
    # every class has nearly all its elements under rule 2
    for cls, idx in SC.rule2_classes(c).items():
        assert len(idx) >= (4 if cls == "planted" else 0.9 * SC.CLASS_N), (cls, len(idx))


def test_c_env_s_is_the_measured_one():
    """C_ENV_S = 4 x the float32 restatement's largest (err - base) / env over the checked
    elements of every case, rounded up to a power of two; each case within RATIO_CAP."""
    worst = 0.0
    for K, inverse in SC.CASES:
        c = SC.case(K, inverse)
        ratios = {n: SC.env_ratio(c, c.yard, n) for n in SC.RULE1}
        print(K, "inv" if inverse else "fwd", {n: round(v, 2) for n, v in ratios.items()},
              "table", SC.C_ENV_RATIOS[(K, inverse)])
        assert max(ratios.values()) <= SC.RATIO_CAP, (K, inverse, ratios)
        worst = max(worst, max(ratios.values()))
    assert SC.C_ENV_S == 2.0 ** math.ceil(math.log2(4 * worst)), worst
    assert SC.C_ENV_S <= 4 * SC.RATIO_CAP


@pytest.mark.parametrize("K,inverse", SC.CASES, ids=IDS)
def test_float32_restatement_passes_with_factor_1(K, inverse):
    """Rule 1 with C_ENV_S / 4; rule 2 against itself (trivially); finite inside, exact outside."""
    c = SC.case(K, inverse)
    print(K, inverse, {k: (f"{v[0]:.1e}", f"{v[1]:.1e}") for k, v in SC.rule2_stats(c, c.yard).items()})
    assert SC.failures(c, c.yard, factor=1.0) == []


def _restatement_reference_root(x, uw, uh, ud):
    """The inverse direction of the float32 restatement with the reference's root,
    2 c / (-b - sqrt(disc)) whatever the sign of b, not pinned."""
    cw, w = AF._knots(uw, SC.MIN, -SC.B, SC.B)
    ch, h = AF._knots(uh, SC.MIN, -SC.B, SC.B)
    d = SC.MIN + F.softplus(ud)
    kn = ch.detach().clone()
    kn[..., -1] += 1e-6
    b = (torch.sum(x[..., None] >= kn, dim=-1) - 1)[..., None]
    g = lambda t: t.gather(-1, b)[..., 0]   # noqa: E731
    icw, ibw, ich, ih, d0, d1 = g(cw), g(w), g(ch), g(h), g(d), g(d[..., 1:])
    s = ih / ibw
    sdd = d0 + d1 - 2 * s
    a = (x - ich) * sdd + ih * (s - d0)
    bb = ih * d0 - (x - ich) * sdd
    c = -s * (x - ich)
    root = (2 * c) / (-bb - torch.sqrt(torch.abs(bb.pow(2) - 4 * a * c)))
    t = root * (1 - root)
    dnum = s.pow(2) * (d1 * root.pow(2) + 2 * s * t + d0 * (1 - root).pow(2))
    return root * ibw + icw, -(torch.log(dnum) - 2 * torch.log(s + sdd * t))


def test_reference_root_fails_rule_1():
    """With the reference's root the float32 restatement breaks rule 1 at the kernels' full
    C_ENV_S on inverse cases (and is not finite on some elements inside the interval)."""
    failing = []
    for K, inverse in SC.CASES:
        if not inverse or K == 1:
            continue
        c = SC.case(K, inverse)
        ins = torch.from_numpy(~c.outside)

        def fn(x, uw, uh, ud):
            o, l = _restatement_reference_root(torch.where(ins, x, torch.zeros_like(x)), uw, uh, ud)
            return torch.where(ins, o, x), torch.where(ins, l, torch.zeros_like(l))

        got = SC.values_and_grads(fn, c.x, c.uw, c.uh, c.ud, c.wo, c.wl, dtype=torch.float32)
        msgs = SC.rule1_failures(c, got, SC.C_ENV_S)
        print(K, {n: round(SC.env_ratio(c, got, n), 1) for n in SC.RULE1}, len(msgs))
        if msgs:
            failing.append(K)
    assert len(failing) >= 1, failing
