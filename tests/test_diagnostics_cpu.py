"""Chain diagnostics (include/flowstate.h 'Chain diagnostics'), the part that needs no GPU:
the ABI's declarations and the float64 numpy restatement of the five definitions that
tests/test_gpu_diagnostics.py holds the kernels to.  The reference has no such feature; the
oracle is the restatement below (vectorised over chains, sequential in t and k exactly as the
header states them), checked here against brute force, closed forms and hand-written cases."""
import math
from fractions import Fraction

import numpy as np
import pytest

from flowstate import _lib
from oracle import analysis as OA
from test_host_cpu import header_symbols

U = 2.0 ** -53
NEW = ("fs_chain_observe", "fs_chain_autocov", "fs_chain_tau", "fs_chain_pool", "fs_chain_transitions")
CONSTANT, TRUNCATED, NONFINITE = 1, 2, 4


# ---------------------------------------------------------------- restatement
def observe_ref(state, is_f32, half_box, r0):
    """(avg_x f64, n_a, n_b u8) [C] of live states [C][N][2] float64: each chain classified
    and averaged in its own dtype, as fs_classify_wells does an array of that dtype."""
    state = np.asarray(state, np.float64)
    C = state.shape[0]
    avg_x, n_a, n_b = np.zeros(C), np.zeros(C, np.uint8), np.zeros(C, np.uint8)
    for dt, sel in ((np.float32, np.asarray(is_f32, bool)), (np.float64, ~np.asarray(is_f32, bool))):
        if sel.any():
            cls, _, ax = OA.classify(state[sel].astype(dt), half_box, r0)
            avg_x[sel], n_a[sel], n_b[sel] = ax.astype(np.float64), (cls == 0).sum(1), (cls == 1).sum(1)
    return avg_x, n_a, n_b


def autocov_ref(x, W):
    """(mean [C], acov [W+1][C]) of x [T][C] (float64, or uint8 widened exactly): s = x_0,
    s += x_t in order, mean = s / T; min == max (a NaN stays) makes the chain constant: mean =
    x_0, acov = +0; otherwise d = x - mean, a += d_t * d_{t+k} for t = 0..T-1-k in order with
    the product rounded first, acov[k] = a / T."""
    x = np.asarray(x).astype(np.float64)
    T, C = x.shape
    assert 0 <= W <= T - 1
    with np.errstate(invalid="ignore", over="ignore"):
        s, mn, mx = x[0].copy(), x[0].copy(), x[0].copy()
        for t in range(1, T):
            s = s + x[t]
            mn, mx = np.minimum(mn, x[t]), np.maximum(mx, x[t])  # both propagate a NaN
        const = mn == mx
        mean = np.where(const, x[0], s / T)
        d = x - mean
        a = np.zeros((W + 1, C))
        for t in range(T):  # every (lag, chain) accumulator takes its terms in order of t
            nk = min(W, T - 1 - t) + 1
            a[:nk] = a[:nk] + d[t] * d[t:t + nk]
        acov = np.where(const, 0.0, a / T)
    return mean, acov


def tau_ref(mean, acov, c=5.0):
    """(tau f64, window i32, flags u8) [C] by the header's rules, in their order."""
    mean, acov = np.asarray(mean, np.float64), np.asarray(acov, np.float64)
    W, C = acov.shape[0] - 1, acov.shape[1]
    tau, window, flags = np.zeros(C), np.zeros(C, np.int32), np.zeros(C, np.uint8)
    for j in range(C):
        v0 = acov[0, j]
        if not (math.isfinite(mean[j]) and math.isfinite(v0)):
            flags[j] = NONFINITE
        elif v0 == 0.0:
            flags[j] = CONSTANT
        else:
            t, window[j], flags[j] = np.float64(0.5), W, TRUNCATED
            for k in range(1, W + 1):
                t = t + acov[k, j] / v0
                if k >= c * t:
                    window[j], flags[j] = k, 0
                    break
            tau[j] = t
    return tau, window, flags


def pool_truth(mean, acov, T):
    """The pooled terms with every sum by math.fsum (the variance of the means in exact
    rational arithmetic), and the sums of absolute terms the bounds need:
    dict(used, n, pooled, pooled_abs, gm, gm_abs, var, var_s, mv, mv_abs)."""
    mean, acov = np.asarray(mean, np.float64), np.asarray(acov, np.float64)
    used = np.isfinite(mean) & np.isfinite(acov[0])
    n = int(used.sum())
    out = dict(used=used, n=n)
    m, a = mean[used], acov[:, used]
    out["pooled"] = np.array([math.fsum(r) / n if n else 0.0 for r in a])
    out["pooled_abs"] = np.array([math.fsum(np.abs(r)) for r in a])
    out["gm"], out["gm_abs"] = (math.fsum(m) / n if n else 0.0), math.fsum(np.abs(m))
    g = sum(Fraction(float(v)) for v in m) / n if n else Fraction(0)
    s = sum((Fraction(float(v)) - g) ** 2 for v in m)
    out["var_s"], out["var"] = float(s), (float(s / (n - 1)) if n >= 2 else 0.0)
    terms = a[0] * float(T) / float(T - 1) if T >= 2 else np.zeros(n)  # the kernel's two roundings per term
    out["mv"], out["mv_abs"] = (math.fsum(terms) / n if n and T >= 2 else 0.0), math.fsum(np.abs(terms))
    return out


def sum_bound(n, abs_sum):
    """|computed - exact| of a plain float64 sum of n terms in any order: (n + 16) u sum |term|
    (n u for the adds; the slack covers the division by the count that follows)."""
    return (n + 16) * U * abs_sum


def var_bound(n, var_s, gm_abs):
    """Bound on |scalars[1] - var| for n >= 2 chains, from sum_bound alone.  The kernel's grand
    mean g' is within eg = sum_bound(n, sum |m|) / n of the exact g.  Its terms are
    q_c = fl(fl(m_c - g')^2) = (m_c - g')^2 (1 + th), |th| <= 3u + O(u^2) <= 4u.  Because
    sum (m_c - g) = 0 exactly, sum (m_c - g')^2 = S + n (g - g')^2 <= S + n eg^2 =: S', with
    S = sum (m_c - g)^2 the exact numerator.  So |sum q_c - S| <= n eg^2 + 4u S'; the kernel's
    sum of the (non-negative) q_c adds sum_bound(n, S' (1 + 4u)) and the division by n - 1 one
    more rounding, both inside (n + 20) u S'.  Hence
        |var' - var| <= (n eg^2 + (n + 24) u S') / (n - 1)."""
    eg = sum_bound(n, gm_abs) / n
    sp = var_s + n * eg * eg
    return (n * eg * eg + (n + 24) * U * sp) / (n - 1)


def rhat_ref(var, mv, n, T):
    if mv == 0.0 or n < 2:
        return None
    return math.sqrt((T - 1) / T + var / mv)


def transitions_ref(n_a, n_b, N):
    """[C][6] int64 {steps_A, steps_B, steps_neither, hops_AB, hops_BA, last}."""
    n_a, n_b = np.asarray(n_a), np.asarray(n_b)
    T, C = n_a.shape
    out = np.zeros((C, 6), np.int64)
    last = np.zeros(C, np.int64)
    for t in range(T):
        s = np.where(n_a[t] == N, 1, np.where(n_b[t] == N, 2, 0))
        out[:, 0] += s == 1
        out[:, 1] += s == 2
        out[:, 2] += s == 0
        hop = (s != 0) & (last != 0) & (s != last)
        out[:, 3] += hop & (s == 2)
        out[:, 4] += hop & (s == 1)
        last = np.where(s != 0, s, last)
    out[:, 5] = last
    return out


def wells_of(states, N):
    """n_a, n_b [T][1] u8 of one chain from a string of 'A', 'B', '-' (neither)."""
    n_a = np.array([[N if ch == "A" else 1] for ch in states], np.uint8)
    n_b = np.array([[N if ch == "B" else 0] for ch in states], np.uint8)
    return n_a, n_b


EXCURSIONS = {  # states -> (steps_A, steps_B, steps_neither, hops_AB, hops_BA, last)
    "A-A": (2, 0, 1, 0, 0, 1),
    "A-B": (1, 1, 1, 1, 0, 2),
    "A--B-A": (2, 1, 3, 1, 1, 1),
    "---": (0, 0, 3, 0, 0, 0),
    "-B": (0, 1, 1, 0, 0, 2),
    "ABAB": (2, 2, 0, 2, 1, 2),
    "BBBA-AAB-": (3, 4, 2, 1, 1, 2),
    "A": (1, 0, 0, 0, 0, 1),
}


def ar1(phi, W):
    """Exact AR(1) autocovariance phi^k, k = 0..W, one chain."""
    return np.array([[phi ** k] for k in range(W + 1)])


def tau_closed(phi, M):
    return 0.5 + (phi * (1 - phi ** M) / (1 - phi) if phi else 0.0)


# ---------------------------------------------------------------- the ABI
def test_new_entry_points_are_declared_and_exported():
    L = _lib.load()
    syms = header_symbols()
    for s in NEW:
        assert s in syms, f"{s} not declared in include/flowstate.h"
        assert s in _lib.EXPORTED, f"{s} has no ctypes signature"
        assert hasattr(L, s), f"{s} not exported by the library"
    assert [k for k, _ in _lib.ChainSeries._fields_] == ["E", "W", "avg_x", "n_a", "n_b", "accept"]


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.load()
    one = 8  # never dereferenced: the checks come first
    bad = [
        L.fs_chain_autocov(one, 0, 600, 4, 4, 513, one, one, None),  # W > 512
        L.fs_chain_autocov(one, 0, 10, 4, 4, 10, one, one, None),    # W = T
        L.fs_chain_autocov(one, 2, 10, 4, 4, 3, one, one, None),     # dtype
        L.fs_chain_autocov(one, 0, 10, 4, 3, 3, one, one, None),     # ld < C
        L.fs_chain_autocov(one, 0, 0, 4, 4, 0, one, one, None),      # T = 0
        L.fs_chain_tau(one, one, 4, 3, 0.0, one, one, one, None),    # c_window
        L.fs_chain_pool(one, one, 4, 3, 0, one, one, None),          # T = 0
        L.fs_chain_transitions(one, one, 5, 4, 4, 256, one, None),   # N > 255
        L.fs_chain_observe(one, None, one, one, one, 4, 256, 5.0, 1.2, 0, 4, _lib.ChainSeries(), None),  # N > 255
        L.fs_chain_observe(one, None, one, one, one, 4, 3, 5.0, 1.2, 0, 3, _lib.ChainSeries(), None),    # ld < C
        L.fs_chain_observe(one, None, None, one, one, 4, 3, 5.0, 1.2, 0, 4, _lib.ChainSeries(E=one), None),
    ]
    assert bad == [-1] * len(bad), bad  # FS_EINVAL
    # C = 0 is a no-op
    assert L.fs_chain_autocov(None, 0, 5, 0, 0, 2, None, None, None) == 0
    assert L.fs_chain_tau(None, None, 0, 2, 5.0, None, None, None, None) == 0
    assert L.fs_chain_pool(None, None, 0, 2, 5, None, None, None) == 0
    assert L.fs_chain_transitions(None, None, 5, 0, 0, 3, None, None) == 0
    assert L.fs_chain_observe(None, None, None, None, None, 0, 3, 5.0, 1.2, 0, 0, _lib.ChainSeries(), None) == 0


# ---------------------------------------------------------------- the restatement
def _series(T, C, seed, drift=0.01):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (T, C)) + 3.0 + drift * np.arange(T)[:, None] * rng.normal(0, 1, C)


def test_autocov_matches_a_per_chain_loop():
    x = _series(12, 5, 0)
    W = 7
    mean, acov = autocov_ref(x, W)
    for c in range(5):
        s = x[0, c]
        for t in range(1, 12):
            s = s + x[t, c]
        m = s / 12
        assert mean[c] == m
        for k in range(W + 1):
            a = np.float64(0.0)
            for t in range(12 - k):
                a = a + (x[t, c] - m) * (x[t + k, c] - m)
            assert acov[k, c] == a / 12, (c, k)
    # against the textbook formula, loosely: the definition is the biased estimator
    d = x - x.mean(0)
    np.testing.assert_allclose(acov[3], (d[:-3] * d[3:]).sum(0) / 12, rtol=1e-12)


def test_constant_rule_and_nonfinite_rows():
    x = np.full((3, 2), 0.1)
    x[1, 1] = 0.25
    mean, acov = autocov_ref(x, 2)
    assert mean[0] == 0.1 and (acov[:, 0] == 0).all() and not np.signbit(acov[:, 0]).any()
    s = (np.float64(0.1) + 0.1 + 0.1) / 3
    assert s != 0.1  # what the rule is for: the plain mean leaves a residual
    assert acov[0, 1] > 0
    u8 = np.array([[1, 0], [1, 1], [1, 0]], np.uint8)
    mean, acov = autocov_ref(u8, 1)
    assert mean[0] == 1.0 and (acov[:, 0] == 0).all() and mean[1] == 1 / 3
    bad = _series(6, 3, 1)
    bad[2, 0], bad[4, 1] = np.inf, np.nan
    mean, acov = autocov_ref(bad, 3)
    assert mean[0] == np.inf and np.isnan(acov[0, 0]) and np.isnan(mean[1]) and np.isnan(acov[0, 1])
    assert np.isfinite(mean[2]) and np.isfinite(acov[:, 2]).all()
    tau, window, flags = tau_ref(mean, acov)
    assert list(flags[:2]) == [NONFINITE, NONFINITE] and tau[0] == 0 and window[1] == 0
    p = pool_truth(mean, acov, 6)
    assert p["n"] == 1 and p["gm"] == mean[2] and p["var"] == 0.0


@pytest.mark.parametrize("phi,W,flag", [(0.0, 8, 0), (0.5, 8, 0), (0.5, 40, 0), (0.9, 8, TRUNCATED), (0.9, 200, 0)])
def test_tau_window_on_exact_ar1(phi, W, flag):
    tau, window, flags = tau_ref([0.0], ar1(phi, W), 5.0)
    assert flags[0] == flag
    if flag == TRUNCATED:
        M = W
    else:
        M = next(m for m in range(1, W + 1) if m >= 5.0 * tau_closed(phi, m))
        assert all(m < 5.0 * tau_closed(phi, m) for m in range(1, M))
    assert window[0] == M
    assert tau[0] == pytest.approx(tau_closed(phi, M), rel=1e-13)
    if flag == 0 and phi:  # the window reaches the asymptote (1 + phi) / (2 (1 - phi)) to phi^M
        assert abs(tau[0] - 0.5 * (1 + phi) / (1 - phi)) <= phi ** (M + 1) / (1 - phi) * (1 + 1e-9)


def test_tau_flags_in_their_order():
    acov = np.array([[1.0, 0.0, np.nan, 1.0, 2.0], [0.5, 0.0, 0.1, 0.5, -0.75]])
    mean = np.array([0.0, 3.0, 0.0, np.inf, 1.0])
    tau, window, flags = tau_ref(mean, acov, 5.0)
    assert list(flags) == [TRUNCATED, CONSTANT, NONFINITE, NONFINITE, 0]
    assert list(window) == [1, 0, 0, 0, 1] and list(tau) == [1.0, 0.0, 0.0, 0.0, 0.125]
    tau, window, flags = tau_ref([1.0], np.array([[2.0]]), 5.0)  # W = 0
    assert (tau[0], window[0], flags[0]) == (0.5, 0, TRUNCATED)


def test_pool_truth_and_rhat():
    x = _series(50, 7, 3)
    mean, acov = autocov_ref(x, 10)
    p = pool_truth(mean, acov, 50)
    assert p["n"] == 7
    np.testing.assert_allclose(p["pooled"], acov.mean(1), rtol=1e-13)
    assert p["gm"] == pytest.approx(mean.mean(), rel=1e-14)
    assert p["var"] == pytest.approx(mean.var(ddof=1), rel=1e-12)
    assert p["mv"] == pytest.approx(x.var(0, ddof=1).mean(), rel=1e-12)  # acov[0] T / (T - 1) is the sample variance
    r = rhat_ref(p["var"], p["mv"], 7, 50)
    assert r == pytest.approx(math.sqrt(49 / 50 + mean.var(ddof=1) / x.var(0, ddof=1).mean()), rel=1e-12)
    assert rhat_ref(p["var"], 0.0, 7, 50) is None and rhat_ref(0.0, 1.0, 1, 50) is None
    assert var_bound(7, p["var_s"], p["gm_abs"]) < 1e-13 * max(p["var"], 1.0)


def test_transition_excursions():
    for states, want in EXCURSIONS.items():
        got = transitions_ref(*wells_of(states, 3), 3)
        assert tuple(got[0]) == want, states
    # n_a == N takes precedence, and a partly filled well is neither
    n_a = np.array([[3], [2], [0]], np.uint8)
    n_b = np.array([[3], [1], [3]], np.uint8)
    assert tuple(transitions_ref(n_a, n_b, 3)[0]) == (1, 1, 1, 1, 0, 2)


def test_observe_restatement_counts_by_dtype():
    rng = np.random.default_rng(5)
    hb, r0, N = 5.0, 1.2, 3
    centres = np.array([[2.5, 5.0], [7.5, 5.0]])
    state = centres[rng.integers(0, 2, (6, N))] + rng.uniform(-1.0, 1.0, (6, N, 2))
    state[0] = centres[0] + 0.1  # all in A
    state[1] = centres[1] - 0.1  # all in B
    is_f32 = np.array([1, 0, 1, 0, 1, 0], np.uint8)
    state[is_f32 == 1] = state[is_f32 == 1].astype(np.float32)
    avg_x, n_a, n_b = observe_ref(state, is_f32, hb, r0)
    assert (n_a[0], n_b[0], n_a[1], n_b[1]) == (3, 0, 0, 3)
    for c in range(6):
        q = state[c].astype(np.float32 if is_f32[c] else np.float64)
        cls = OA.classify(q[None], hb, r0)[0][0]
        assert (n_a[c], n_b[c]) == ((cls == 0).sum(), (cls == 1).sum())
        assert avg_x[c] == np.float64(np.mean(q[:, 0]))
