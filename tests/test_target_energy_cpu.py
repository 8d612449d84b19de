"""The inputs of tests/test_gpu_target_energy.py meet their stated conditions, and the float32
restatement's error against float64 (the envelope the kernels are held to) is what the GPU
test assumes: checked on the CPU, so the inputs stay checked wherever the suite runs."""
import numpy as np
import pytest
import torch

import target_energy_cases as TC


@pytest.mark.parametrize("N", TC.NS)
def test_uniform_rows_meet_conditions(N):
    """No pair (origin particle included) within 1e-3 of the core radius or closer than
    0.02, no coordinate within 1e-5 bound of a wrap half-way point, and the wrap acts."""
    x = TC.inputs(N, "uniform")
    bound = TC.bound_of(N)
    assert x.dtype == torch.float32 and x.shape == (TC.ROWS, 2 * N)
    r = TC.pair_distances(x.double(), bound)
    assert r.shape[1] == (N + 1) * N // 2
    assert float((r - TC.BK).abs().min()) >= 1e-3
    assert float(r.min()) >= 0.02
    assert TC.wrap_margin(x.double(), bound) >= 1e-5
    assert float(x.abs().max()) > bound and float(x.abs().max()) <= 1.3 * bound * (1 + 1e-6)
    if N >= 63:
        assert bool((x.abs() > bound).any(dim=1).all())  # every row has wrapped particles


@pytest.mark.parametrize("N", TC.NS)
def test_census_rows_have_exactly_one_close_pair(N):
    """Each pair-census row holds exactly one pair with r < 2: the chosen staged-index pair
    at r = 0.9, worth 6.6 / T: most of the row's energy scale, so a pair skipped or counted
    twice moves the energy by far more than 100 tolerances."""
    x = TC.inputs(N, "census")
    bound = TC.bound_of(N)
    pairs = TC.census_pairs(N)
    M, D = N + 1, (N + 1) // 2
    assert len(x) == len(pairs) >= (4 if N == 3 else 8)
    for need in ((0, 1), (0, D), (0, M - 1), (M - 2, M - 1)):
        assert need in pairs
    if N > 64:
        assert (1, 65) in pairs and (N - 64, N) in pairs
    if N > 128:
        assert (1, 129) in pairs
    s = TC.staged(x.double(), bound)
    iu = torch.triu_indices(M, M, offset=1)
    r = (s[:, iu[0]] - s[:, iu[1]]).norm(dim=-1)
    assert bool(((r < 2).sum(dim=1) == 1).all())
    k = r.argmin(dim=1)
    assert [(int(iu[0][i]), int(iu[1][i])) for i in k] == pairs
    np.testing.assert_allclose(r.min(dim=1).values.numpy(), 0.9, atol=2e-6)
    assert TC.wrap_margin(x.double(), bound) >= 1e-5
    e_pair = 4 * (0.9 ** -12 - 0.9 ** -6)
    for cset in ("drivers", "alt"):
        ref = TC.reference(N, cset, "census")
        T = TC.CONSTS[cset]["T"]
        assert float((e_pair / T / ref.S).min()) > 0.15, "the census pair must dominate the tolerance"
        assert e_pair / T / float(ref.S.max()) > 100 * (2 * ref.u32 + 2 * TC.EPS32)


@pytest.mark.parametrize("N", TC.NS)
def test_dense_rows_are_in_the_linear_core(N):
    x = TC.inputs(N, "dense")
    s = TC.staged(x.double(), TC.bound_of(N))[:, 1:]
    assert float((s - 1).norm(dim=-1).max()) <= 0.4 + 1e-6
    iu = torch.triu_indices(N, N, offset=1)
    r = (s[:, iu[0]] - s[:, iu[1]]).norm(dim=-1)
    assert float(r.max()) <= TC.BK - 1e-3 and float(r.min()) >= 1e-3
    r0 = s.norm(dim=-1)  # pairs with the origin particle: outside the core, off its edge
    assert float(r0.min()) > 1.0 and float(r0.max()) < 1.82


@pytest.mark.parametrize("N", TC.NS)
def test_wells_rows_sit_in_the_wells(N):
    """Rows of the wells kind: no pair closer than 1, and the well terms are most of the
    energy scale at every constant set, so a temperature applied to the double well, a wrong
    V0 / r0 / k or a well's minimum image that misses the box-length displacement shows."""
    x = TC.inputs(N, "wells")
    bound = TC.bound_of(N)
    assert x.shape == (TC.ROWS, 2 * N)
    assert float(TC.pair_distances(x.double(), bound).min()) >= 1.0
    assert TC.wrap_margin(x.double(), bound) >= 1e-5
    assert float(x.abs().max()) > 1.4 * bound  # displaced by a box length
    for cset in TC.CONSTS:
        ref = TC.reference(N, cset, "wells")
        lj = TC.energy_scale(TC.make_mod(N, cset, wells=0), x.double())
        assert float(((ref.S - lj) / ref.S).min()) > 0.5
        T = TC.CONSTS[cset]["T"]
        if T != 1.0:  # dividing the well part by T as well moves E by far more than the tolerance
            assert float(((ref.S - lj) * abs(1 / T - 1) / ref.S).min()) > 100 * (2 * ref.u32 + 2 * TC.EPS32)


@pytest.mark.parametrize("N,cset", TC.CASES)
def test_float32_envelope(N, cset):
    """The float32 restatement's own error against float64, which sizes the kernels'
    tolerance (u <= 2 u32 + 2 eps32, v <= 2 v32 + 2 eps32): finite, non-trivial, and small
    enough that the tolerance can see a single mis-counted pair or a wrong temperature."""
    for kind in TC.KINDS:
        ref = TC.reference(N, cset, kind)
        assert bool(torch.isfinite(ref.E64).all() and torch.isfinite(ref.g64).all())
        assert bool(torch.isfinite(ref.E32).all() and torch.isfinite(ref.g32).all())
        assert bool((ref.S > 0).all() and (ref.gmax > 0).all())
        print(f"N={N} {cset} {kind}: u32={ref.u32:.2e} v32={ref.v32:.2e}")
        # measured here: u32 <= 3.5e-5, v32 <= 6.4e-4 (an ill-conditioned uniform row at N = 5);
        # torch's float32 CPU sums differ between hosts, so the envelope is held to 5x that
        assert ref.u32 <= 2e-4 and ref.v32 <= 3e-3
    # the temperature matters at every set but the drivers': the LJ part alone moves E by more
    # than the tolerance when T is replaced by 1 / T or dropped
    if cset != "drivers":
        ref = TC.reference(N, cset, "dense")
        T = TC.CONSTS[cset]["T"]
        assert abs(1 / T - T) * 30 * N / float(ref.S.max()) > 100 * (2 * ref.u32 + 2 * TC.EPS32)


@pytest.mark.parametrize("wells", [0, 1])
def test_fewer_wells_reference_differs(wells):
    """num_wells 0 / 1 references (SimpleLJ; DoubleWellLJ cut to its first well) differ from
    the two-well energy on every row of the wells kind, so a kernel that ignores num_wells fails."""
    for N in TC.NS:
        two = TC.reference(N, "alt", "wells")
        ref = TC.reference(N, "alt", "wells", wells)
        assert float(((ref.E64 - two.E64).abs() / two.S).min()) > 100 * (2 * two.u32 + 2 * TC.EPS32)


@pytest.mark.parametrize("N", TC.EDGE_NS)
def test_edge_rows_nan_patterns(N):
    """torch's float32 autograd on the edge rows: coinciding particles and a pair whose
    (1/r)^11 overflows make both particles' gradients NaN, a particle on a well centre or on
    the origin particle only its own; energies stay finite.  The rows at the core radius
    land on both sides of the inclusive edge, 0.1 apart."""
    ref = TC.edge_reference(N)
    assert bool(torch.isfinite(ref.E32).all())
    nan = torch.isnan(ref.g32).reshape(len(TC.EDGE_NAMES), N, 2)
    want = TC.expected_nan_particles(N)
    for i, name in enumerate(TC.EDGE_NAMES):
        got = {int(p) for p in torch.nonzero(nan[i].any(dim=1)).flatten()}
        assert got == want[name], (name, got)
        assert bool((nan[i, list(got)]).all()) if got else True  # both coordinates
    E = dict(zip(TC.EDGE_NAMES, ref.E32.tolist()))
    T = TC.CONSTS["alt"]["T"]
    for a in ("core_origin", "core_pair"):
        jump = (E[a + "_up"] - E[a]) * T
        assert 0.08 < jump < 0.2, jump   # 4 (r^-12 - r^-6) - 30 at r = 0.82
    # on these rows float64 happens to take the same side, so the envelope stays sharp
    assert ref.u32 <= 1e-5
