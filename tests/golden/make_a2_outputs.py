"""Generate tests/golden/a2_outputs.npz by running the REFERENCE's own analysis code
(hybrid_NF_MCMC/utils.py) the way main_algorithm_2.py's checkpoint cycle calls it
(:493-525):

    a_ = a + HALF_BOX                                            float32
    plot_frequency_heatmap(a_ - HALF_BOX, dir, cmap, HALF_BOX, base_filename=...)
    calculate_pair_correlation(a_ - HALF_BOX, N, HALF_BOX, dr=HALF_BOX/50)

Usage:  python tests/golden/make_a2_outputs.py <path of a checkout of the reference>
(needs numpy, pandas, tqdm and matplotlib; the Agg backend is forced).  Never imported
by a test.  Data only: the float32 inputs and the reference's outputs for two cases,
N=3 / M=300 and N=16 / M=150 (M > 128: pandas' mean takes numpy's recursive pairwise
sum).  Inputs are uniform in [-hb, hb] with a few entries set to exactly +-fl32(hb), 0
and the float32 neighbours of interior heat-map edges, and one configuration with two
coincident particles (distance 0 is dropped from g(r)).
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_utils(ref):
    """hybrid_NF_MCMC/utils.py by path (get_project_root() wants a directory named
    flow_state above it: a link in a temp directory provides one)."""
    os.environ["MPLBACKEND"] = "Agg"
    sys.dont_write_bytecode = True
    link = os.path.join(tempfile.mkdtemp(), "flow_state")
    os.symlink(os.path.abspath(ref), link)
    for p in (link, os.path.join(link, "MCMC"), os.path.join(link, "NF")):
        sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location("hyb_utils", os.path.join(link, "hybrid_NF_MCMC", "utils.py"))
    U = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        spec.loader.exec_module(U)
    return U


def make_inputs(N, M, seed):
    hb = ((N / 0.03) ** (1 / 2)) / 2  # HALF_BOX (main_algorithm_2.py:65), a Python float
    hbf = np.float32(hb)
    rng = np.random.default_rng(seed)
    z = ((rng.random((M, N, 2)) * 2 - 1) * hb).astype(np.float32)
    np.clip(z, -hbf, hbf, out=z)
    flat = z.reshape(-1)
    edges = np.linspace(-hb, hb, 100)
    special = [hbf, -hbf, np.float32(0.0)]
    for e in edges[[1, 7, 49, 50, 98]]:
        c = np.float32(e)
        special += [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    where = rng.choice(flat.size, size=2 * len(special), replace=False)
    for k, i in enumerate(where):
        flat[i] = special[k % len(special)]
    z[1, 1] = z[1, 0]  # two coincident particles
    return hb, z


def case(U, N, M, seed):
    hb, z = make_inputs(N, M, seed)
    a_ = z + hb  # float32: HALF_BOX is a weak scalar
    assert a_.dtype == np.float32
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(io.StringIO()), \
            contextlib.redirect_stderr(io.StringIO()):
        U.plot_frequency_heatmap(a_ - hb, d + "/", None, hb, base_filename="frequency_heatmap_cycle_1")
        with open(os.path.join(d, "frequency_heatmap_cycle_1_data.json")) as f:
            hm = json.load(f)
        r, g = U.calculate_pair_correlation(a_ - hb, N, hb, dr=hb / 50)
    return {"z": z, "half_box": np.float64(hb), "samples": a_,
            "hist_relative": np.array(hm["hist_relative"], np.float64), "x_edges": np.array(hm["x_edges"], np.float64),
            "y_edges": np.array(hm["y_edges"], np.float64), "r": np.asarray(r, np.float64),
            "g_r": np.asarray(g, np.float64)}


def main(ref):
    U = load_utils(ref)
    out = {}
    for name, N, M, seed in (("n3", 3, 300, 31), ("n16", 16, 150, 32)):
        for k, v in case(U, N, M, seed).items():
            out[f"{name}/{k}"] = v
    path = os.path.join(HERE, "a2_outputs.npz")
    np.savez_compressed(path, **out)
    print("a2_outputs: ok,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
