"""Importance weights of flow samples (include/flowstate.h 'Importance weights'), the part
that needs no GPU: the ABI's declarations and argument checks, the float64 numpy
restatement of the streaming statistics that tests/test_gpu_importance.py holds the kernels
to, and the defaults of the Python layers.  The reference has no such feature; the oracle
is the restatement below, checked here against brute force."""
import ctypes
import inspect
import math

import numpy as np
import pytest

from flowstate import _lib, analysis
from flowstate.algorithm2 import Algorithm2

U = 2.0 ** -53
NEW = ("fs_iw_state_bytes", "fs_iw_reset", "fs_importance_weights", "fs_weighted_reduce", "fs_weighted_hist2d")


# ---------------------------------------------------------------- restatement
def log_weights(beta, E, log_q):
    """lw = (-beta) E - (double)log_q in float64, one rounding per operation; -inf for a bad
    row (NaN / +-inf log_q, NaN / -inf E).  Returns (lw, zero mask, bad mask)."""
    E = np.asarray(E, np.float64)
    q = np.asarray(log_q, np.float32)
    bad = ~np.isfinite(q) | np.isnan(E) | (E == -np.inf)
    with np.errstate(invalid="ignore"):
        lw = (-beta) * E - q.astype(np.float64)
    lw[bad] = -np.inf
    return lw, (lw == -np.inf) & ~bad, bad


class Stream:
    """The seven running statistics, merged a batch at a time by the online log-sum-exp in
    plain numpy float64 (no particular summation order)."""

    def __init__(self):
        self.max_lw, self.s1, self.s2, self.sum_lw, self.n, self.n_zero, self.n_bad = -np.inf, 0.0, 0.0, 0.0, 0, 0, 0

    def add(self, beta, E, log_q):
        lw, zero, bad = log_weights(beta, E, log_q)
        new = max(self.max_lw, float(lw.max())) if lw.size else self.max_lw
        if new > -np.inf:
            f = math.exp(self.max_lw - new) if self.max_lw > -np.inf else 0.0
            w = np.exp(lw[lw > -np.inf] - new)
            self.s1 = self.s1 * f + float(w.sum())
            self.s2 = self.s2 * (f * f) + float((w * w).sum())
        self.max_lw = new
        self.sum_lw += float(lw[np.isfinite(lw)].sum())
        self.n, self.n_zero, self.n_bad = self.n + lw.size, self.n_zero + int(zero.sum()), self.n_bad + int(bad.sum())
        return lw

    def header(self):
        return (self.max_lw, self.s1, self.s2, self.sum_lw, self.n, self.n_zero, self.n_bad)


def truth(lw):
    """(max_lw, S1, S2, sum_lw, sum |lw|) of all rows at once: math.fsum over numpy.exp in
    float64 with the global maximum as shift."""
    lw = np.asarray(lw, np.float64)
    fin = lw[np.isfinite(lw)]
    if fin.size == 0:
        return -np.inf, 0.0, 0.0, 0.0, 0.0
    mx = float(fin.max())
    return (mx, math.fsum(np.exp(fin - mx)), math.fsum(np.exp(2 * (fin - mx))), math.fsum(fin),
            math.fsum(np.abs(fin)))


def bound(lw):
    """(n + 4 spread + 16) u, n the row count and spread the distance between the largest and
    the smallest finite lw: the relative bound of S1 in any summation order (n u for the
    sum, |lw - shift| u for each subtraction, a few ulp for exp).  S2 takes twice, ess four
    times, every weighted output twice this bound; sum_lw takes it relative to sum |lw|
    (recursive summation of n signed terms: n u sum |x|)."""
    lw = np.asarray(lw, np.float64)
    fin = lw[np.isfinite(lw)]
    spread = float(fin.max() - fin.min()) if fin.size else 0.0
    return (lw.size + 4 * spread + 16) * U


def normalised(lw):
    """w~ = exp(lw - max) / S1 in float64, S1 by fsum."""
    mx, s1 = truth(lw)[:2]
    with np.errstate(invalid="ignore"):
        w = np.where(np.isfinite(lw), np.exp(np.asarray(lw, np.float64) - mx), 0.0)
    return w / s1


def bins_of(v, edges):
    """np.histogram's bin of each value: searchsorted(edges, v, 'right') - 1 with the last
    edge inclusive; -1 outside."""
    v = np.asarray(v, np.float64)
    nb = edges.shape[0] - 1
    k = np.searchsorted(edges, v, "right") - 1
    k[v == edges[-1]] = nb - 1
    k[(v < edges[0]) | (v > edges[-1]) | np.isnan(v)] = -1
    return k


def weighted_hist(samples, half_box, edges, w):
    """hist_w by fsum per bin, binning (double)(sample - fl32(half_box))."""
    c = (np.asarray(samples, np.float32) - np.float32(half_box)).astype(np.float64)
    nb = edges.shape[0] - 1
    bx, by = bins_of(c[..., 0], edges), bins_of(c[..., 1], edges)
    terms = {}
    for m in range(c.shape[0]):
        if not w[m] > 0:
            continue
        for i in range(c.shape[1]):
            if bx[m, i] >= 0 and by[m, i] >= 0:
                terms.setdefault((bx[m, i], by[m, i]), []).append(w[m])
    out = np.zeros((nb, nb))
    for (i, j), t in terms.items():
        out[i, j] = math.fsum(t)
    return out


# ---------------------------------------------------------------- tests
def test_header_and_ctypes_table_declare_the_symbols():
    from test_host_cpu import header_symbols

    L = _lib.load()
    for s in NEW:
        assert s in header_symbols() and s in _lib.EXPORTED and hasattr(L, s), s
    assert L.fs_iw_state_bytes() == 64 + 1024 * 64


def _refused(L, rc, name):
    return rc == -1 and name.encode() in L.fs_last_error()


def test_entry_points_check_their_arguments():
    """Null pointers and out-of-range sizes return FS_EINVAL with the entry point's name in
    fs_last_error() before anything is launched; M = 0 is a successful no-op.  No GPU is
    needed for either."""
    L = _lib.load()
    one = ctypes.c_void_p(8)  # aligned, never dereferenced
    assert _refused(L, L.fs_iw_reset(None, None), "fs_iw_reset")
    assert _refused(L, L.fs_iw_reset(ctypes.c_void_p(4), None), "fs_iw_reset")

    iw = L.fs_importance_weights
    assert iw(1.0, 0, None, None, None, None, None) == 0
    for k in range(4):
        a = [one] * 4
        a[k] = None
        assert _refused(L, iw(1.0, 5, *a, None), "fs_importance_weights"), k
    assert _refused(L, iw(1.0, -1, one, one, one, one, None), "fs_importance_weights")
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        assert _refused(L, iw(beta, 5, one, one, one, one, None), "fs_importance_weights"), beta
    assert _refused(L, iw(1.0, 5, one, one, one, ctypes.c_void_p(12), None), "fs_importance_weights")

    wr = L.fs_weighted_reduce
    assert wr(None, 0, 50, None, None, None, None, None, None, None, None) == 0
    for k in range(8):
        a = [one] * 8
        a[k] = None
        assert _refused(L, wr(a[0], 5, 50, *a[1:], None), "fs_weighted_reduce"), k
    for nr in (0, 129):
        assert _refused(L, wr(one, 5, nr, one, one, one, one, one, one, one, None), "fs_weighted_reduce"), nr
    assert _refused(L, wr(one, -1, 50, one, one, one, one, one, one, one, None), "fs_weighted_reduce")

    wh = L.fs_weighted_hist2d
    assert wh(None, 0, 16, 5.0, one, 99, None, None, None, None) == 0
    for N, nb in ((65, 99), (0, 99), (16, 121), (16, 0)):
        assert _refused(L, wh(one, 5, N, 5.0, one, nb, one, one, one, None), "fs_weighted_hist2d"), (N, nb)
    for k in range(5):
        a = [one] * 5  # samples, edges, log_w, state, hist_w
        a[k] = None
        assert _refused(L, wh(a[0], 5, 16, 5.0, a[1], 99, a[2], a[3], a[4], None), "fs_weighted_hist2d"), k
    assert _refused(L, wh(one, 5, 16, 0.0, one, 99, one, one, one, None), "fs_weighted_hist2d")


@pytest.mark.parametrize("batches", [1, 3])
def test_restatement_against_brute_force(batches):
    """16 rows whose weights exp(lw) fit a double unshifted: ESS, log Z, mean log w and the
    largest weight from the plain definitions, one hard-core row and one NaN row included."""
    rng = np.random.default_rng(5)
    beta = 0.7
    E = rng.normal(0, 4, 16)
    q = rng.normal(-3, 2, 16).astype(np.float32)
    E[3], q[11] = np.inf, np.nan
    s = Stream()
    lw = np.concatenate([s.add(beta, e, l) for e, l in zip(np.array_split(E, batches), np.array_split(q, batches))])
    ok = np.ones(16, bool)
    ok[[3, 11]] = False
    w = np.zeros(16)
    w[ok] = np.exp(-beta * E[ok]) / np.exp(q[ok].astype(np.float64))
    assert lw[3] == -np.inf and lw[11] == -np.inf
    np.testing.assert_allclose(np.exp(lw[ok]), w[ok], rtol=1e-13)
    got = analysis.importance_summary(s.header())
    assert (got["n_zero"], got["n_bad"]) == (1, 1) and s.n == 16
    np.testing.assert_allclose(got["ess"], w.sum() ** 2 / (w * w).sum(), rtol=1e-13)
    np.testing.assert_allclose(got["ess_fraction"], got["ess"] / 16, rtol=1e-15)
    np.testing.assert_allclose(got["log_z"], np.log(w.sum() / 16), rtol=1e-13)
    np.testing.assert_allclose(got["mean_log_w"], np.log(w[ok]).mean(), rtol=1e-13)
    np.testing.assert_allclose(got["max_weight_fraction"], w.max() / w.sum(), rtol=1e-13)
    np.testing.assert_allclose(normalised(lw), w / w.sum(), rtol=1e-13)
    mx, s1, s2, sl, _ = truth(lw)
    b = bound(lw)
    assert s.max_lw == mx and abs(s.s1 - s1) <= b * s1 and abs(s.s2 - s2) <= 2 * b * s2


def test_restatement_handles_empty_weight():
    s = Stream()
    s.add(1.0, np.full(5, np.inf), np.zeros(5, np.float32))
    got = analysis.importance_summary(s.header())
    assert s.max_lw == -np.inf and s.s1 == 0.0 and got["ess"] == 0.0 and got["n_zero"] == 5
    s.add(1.0, np.array([1.0, 2.0]), np.zeros(2, np.float32))
    assert s.max_lw == -1.0 and s.s1 == 1.0 + math.exp(-1.0) and s.n == 7


def test_bins_of_is_numpy_histogram():
    rng = np.random.default_rng(2)
    edges = np.linspace(-3.0, 3.0, 11)
    v = np.concatenate([rng.uniform(-3.5, 3.5, 500), edges, [np.nextafter(3.0, 4.0)]])
    k = bins_of(v, edges)
    np.testing.assert_array_equal(np.bincount(k[k >= 0], minlength=10), np.histogram(v, edges)[0])


def test_python_defaults():
    """The new behaviour is opt-in: reweight=None, density_pass=False, reweight_analysis=False."""
    p = inspect.signature(analysis.sample_analysis).parameters
    assert p["reweight"].default is None and p["density_pass"].default is False and p["r0"].default == 1.2
    assert inspect.signature(Algorithm2.__init__).parameters["reweight_analysis"].default is False
