"""Generate tests/golden/physics_params.npz by running the REFERENCE itself.

Container-only, like make_goldens.py (whose import recipe it uses): the reference is
imported read-only and only arrays are stored.  Re-run with

    python tests/golden/make_params_golden.py

physics_params.npz: the reference's EnergyCalculator / SimulationBox away from the drivers'
square box and constants, at the parameter sets P1 (aspect 1.6, two wells) and P2 (aspect
0.55, one well) of tests/physics_params_cases.py (V0 = (-4, 3), r0 = 0.8, k = 7), N = 3 and
16, float32 and float64: a handful of configurations each (pairs that are neighbours only
through the y wrap or only through the x wrap, a particle inside a well, a jittered lattice, a
hard-core overlap) with calculate_total_energy_virial, minimum_image for a list of pairs and
calculate_particle_energy_virial for every particle.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "flow-state_amd"), os.path.join(REPO, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_goldens import import_reference  # noqa: E402
import physics_params_cases as PC  # noqa: E402

# rows of PC.positions(): two y-wrap, two x-wrap, two well rows, a lattice row, a uniform row
ROWS = (0, 1, PC.N_YWRAP, PC.N_YWRAP + 1, PC.N_YWRAP + PC.N_XWRAP, PC.N_YWRAP + PC.N_XWRAP + 1, PC.SPECIAL + 1,
        PC.SPECIAL)
C = PC.SPECIAL + 2


def main():
    _, MC, _ = import_reference()
    from energy_calculator import EnergyCalculator

    out = {}
    for name in ("P1", "P2"):
        prm = PC.PARAMS[name]
        for N in (3, 16):
            with contextlib.redirect_stdout(io.StringIO()):
                _, box = MC.initialise_fcc(num_particles=N, rho=0.03, aspect_ratio=prm["aspect"])
            ph = PC.oracle_phys(N, name)
            assert box.box_size_x == ph.Lx and box.box_size_y == ph.Ly
            for dt in (np.float32, np.float64):
                tag = f"{name}_N{N}_{'f32' if dt == np.float32 else 'f64'}"
                pos = PC.positions(N, C, name, dt)[list(ROWS)]
                ew, pe, delta = [], [], []
                ij = np.array([(i, j) for i in range(N) for j in range(N) if i != j][:24])
                for x in pos:
                    with contextlib.redirect_stdout(io.StringIO()):
                        ec = EnergyCalculator(num_particles=N, initial_particles=x, simulation_box=box,
                                              num_wells=prm["num_wells"], V0_list=list(prm["V0"]), r0=prm["r0"],
                                              k=prm["k"], timing=False, checking=False)
                    ew.append(ec.calculate_total_energy_virial(x))
                    pe.append([ec.calculate_particle_energy_virial(x, p) for p in range(N)])
                    d = np.stack([box.minimum_image(x[i], x[j]) for i, j in ij])
                    assert d.dtype == dt
                    delta.append(d)
                out[tag + "_pos"] = pos
                out[tag + "_box"] = np.array([box.box_size_x, box.box_size_y], np.float64)
                out[tag + "_EW"] = np.array(ew, np.float64)
                out[tag + "_particle_ew"] = np.array(pe, np.float64)
                out[tag + "_ij"] = ij
                out[tag + "_delta"] = np.stack(delta)
                print(f"{tag}: E {np.array(ew)[:, 0]}")
    np.savez_compressed(os.path.join(HERE, "physics_params.npz"), **out)


if __name__ == "__main__":
    main()
