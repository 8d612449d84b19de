"""The C oracle (oracle/physics.py) away from the drivers' square box and constants, before
any GPU test leans on it there: parameter sets P1-P3 of physics_params_cases.py (aspect 1.6 /
0.55, V0 = (-4, 3), r0 = 0.8, k = 7, two / one / no wells) against the numpy statement of the
reference's pair loop, and against vectors the reference itself produced
(tests/golden/physics_params.npz, made by tests/golden/make_params_golden.py; the reference's
classes accept one well, so P2 is in the fixture too)."""
import os

import numpy as np
import pytest

import physics_params_cases as PC
from oracle import physics as OP

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _close(a, b):
    return (np.isinf(a) and np.isinf(b) and a == b) or abs(a - b) <= 1e-12 * max(1.0, abs(b))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [3, 16])
@pytest.mark.parametrize("name", ["P1", "P2", "P3"])
def test_oracle_matches_pairloop_at_params(name, N, dtype):
    """OP.total_energy against OP.total_energy_pairloop (bit-exact to the reference on the
    square box, test_oracle_golden.py) within the tolerance the two are held to there, on
    rows with pairs inside r_cut only across the y edge, only across the x edge, a particle
    inside a well, and hard-core overlaps (inf)."""
    ph = PC.oracle_phys(N, name)
    assert ph.Lx != ph.Ly and abs(ph.Lx * ph.Ly - N / 0.03) < 1e-9
    C = PC.SPECIAL + 22
    pos = PC.positions(N, C, name, dtype)
    assert pos.dtype == dtype and (pos >= 0).all() and (pos[..., 0] <= ph.Lx).all() and (pos[..., 1] <= ph.Ly).all()
    PC.check_wrap_rows(pos, ph)
    Eb, Wb, ovb = OP.total_energy_batch(pos, ph)
    n_inf = 0
    for c in range(C):
        E, W, hit = OP.total_energy(pos[c], ph)
        Ep, Wp = OP.total_energy_pairloop(pos[c], ph)
        assert E == Eb[c] and W == Wb[c] and hit == bool(ovb[c])
        assert hit == bool(np.isinf(Ep))
        assert _close(E, Ep) and _close(W, Wp), (c, E, Ep, W, Wp)
        n_inf += hit
    assert 0 < n_inf < C - PC.SPECIAL
    # the well rows feel their well (where there is one): the last particle's well term is
    # most of what changes when the wells are switched off
    rows = range(PC.N_YWRAP + PC.N_XWRAP, PC.SPECIAL)
    free = PC.oracle_phys(N, "P3")
    free.Lx, free.Ly = ph.Lx, ph.Ly
    dE = np.array([OP.total_energy(pos[c], ph)[0] - OP.total_energy(pos[c], free)[0] for c in rows])
    if ph.num_wells == 2:
        assert (np.abs(dE) > 0.1).sum() >= 6 and (dE > 0.1).any() and (dE < -0.1).any()  # V0 = (-4, +3)
    elif ph.num_wells == 1:
        assert (dE < -0.1).sum() >= 3 and (np.abs(dE[1::2]) < 1e-3).all()  # only the first well exists
    else:
        assert (dE == 0).all()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N", [3, 16])
@pytest.mark.parametrize("name", ["P1", "P2"])
def test_oracle_matches_reference_at_params(name, N, dt):
    """The reference's own EnergyCalculator / SimulationBox outputs on a non-square box:
    total energy and virial and per-particle energy and virial within 1e-12, minimum-image
    vectors bit-exact in the reference's dtype."""
    f = np.load(os.path.join(G, "physics_params.npz"))
    tag = f"{name}_N{N}_{dt}"
    ph = PC.oracle_phys(N, name)
    np.testing.assert_array_equal(f[tag + "_box"], [ph.Lx, ph.Ly])
    pos = f[tag + "_pos"]
    assert pos.dtype == (np.float32 if dt == "f32" else np.float64)
    np.testing.assert_array_equal(pos, PC.positions(N, PC.SPECIAL + 2, name, pos.dtype)[list(fixture_rows())])
    n_fin = 0
    for c, x in enumerate(pos):
        E, W, hit = OP.total_energy(x, ph)
        Er, Wr = f[tag + "_EW"][c]
        assert hit == bool(np.isinf(Er))
        assert _close(E, Er) and _close(W, Wr), (c, E, Er)
        n_fin += not hit
        for p in range(N):
            e, w = OP.particle_energy(x, p, ph)
            er, wr = f[tag + "_particle_ew"][c, p]
            assert _close(e, er) and _close(w, wr), (c, p, e, er)
        for (i, j), want in zip(f[tag + "_ij"], f[tag + "_delta"][c]):
            got = OP.min_image(x[i], x[j], ph)
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got, want)
    assert n_fin >= 5
    # the wrap rows: the stored minimum images really cross the edge on one axis only
    d01 = f[tag + "_delta"][:4, 0]  # pair (0, 1) of the two y-wrap and the two x-wrap rows
    assert (f[tag + "_ij"][0] == [0, 1]).all()
    raw = pos[:4, 0] - pos[:4, 1]
    assert (np.abs(raw[:2, 1] - d01[:2, 1]) > ph.Ly / 2).all() and (raw[:2, 0] == d01[:2, 0]).all()
    assert (np.abs(raw[2:, 0] - d01[2:, 0]) > ph.Lx / 2).all() and (raw[2:, 1] == d01[2:, 1]).all()


def fixture_rows():
    """The rows of PC.positions() the fixture holds (make_params_golden.ROWS)."""
    s = PC.N_YWRAP + PC.N_XWRAP
    return (0, 1, PC.N_YWRAP, PC.N_YWRAP + 1, s, s + 1, PC.SPECIAL + 1, PC.SPECIAL)
