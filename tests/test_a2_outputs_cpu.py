"""Host side of the Algorithm-2 checkpoint-cycle outputs (main_algorithm_2.py:458-526,
588-599): the numpy restatement of the analysis batch's three float32 steps against the
reference's own outputs (tests/golden/a2_outputs.npz, made by make_a2_outputs.py from
hybrid_NF_MCMC/utils.py), the checkpoint rule, the JSON / npy writers, the unchanged
defaults of Algorithm2 and the ABI's argument checks.  No GPU compute; the GPU tests
(test_gpu_a2_outputs.py) compare the kernel with `restate` at other shapes."""
import ctypes
import inspect
import json
import os
import types

import numpy as np
import pytest
import torch

from flowstate import _lib, io
from flowstate.algorithm2 import Algorithm2, is_checkpoint_cycle, saves_model
from oracle import analysis as OA

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("n3", "n16")


def restate(z, hb, bins=100, dr=None):
    """The checkpoint cycle's arithmetic on one (M, N, 2) float32 array of flow samples
    (main_algorithm_2.py:499, 510, 519 with numpy 2's weak Python scalars: HALF_BOX is
    rounded to float32 and both steps stay float32):
      a_ = a + HALF_BOX;  c = a_ - HALF_BOX
      np.histogram2d(c) over np.linspace(-hb, hb, bins)      (utils.py:488-495)
      calculate_pair_correlation(c, N, hb, dr)                (oracle.analysis.rdf)
    -> a_, hist (float64 counts), edges, r, g_r."""
    z = np.asarray(z)
    assert z.dtype == np.float32
    a_ = z + np.float32(hb)
    return (a_,) + analyse(a_, hb, bins, dr)


def analyse(a_, hb, bins=100, dr=None):
    """The heat map and g(r) of a_ - HALF_BOX (float32) -> hist, edges, r, g_r."""
    assert a_.dtype == np.float32
    c = a_ - np.float32(hb)
    edges = np.linspace(-hb, hb, bins)
    xy = c.reshape(-1, 2)
    hist, _, _ = np.histogram2d(xy[:, 0], xy[:, 1], bins=[edges, edges])
    r, g = OA.rdf(c, a_.shape[1], hb, dr=hb / 50 if dr is None else dr)
    return hist, edges, r, g


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(G, "a2_outputs.npz"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(fixture, name):
    f = {k.split("/", 1)[1]: fixture[k] for k in fixture.files if k.startswith(name + "/")}
    hb = float(f["half_box"])
    assert hb == ((f["z"].shape[1] / 0.03) ** (1 / 2)) / 2
    a_, hist, edges, r, g = restate(f["z"], hb)
    np.testing.assert_array_equal(a_, f["samples"])
    assert a_.dtype == f["samples"].dtype == np.float32
    np.testing.assert_array_equal(hist / hist.sum(), f["hist_relative"])
    np.testing.assert_array_equal(edges, f["x_edges"])
    np.testing.assert_array_equal(edges, f["y_edges"])
    np.testing.assert_array_equal(r, f["r"])
    np.testing.assert_array_equal(g, f["g_r"])


def test_fixture_holds_the_edge_inputs(fixture):
    """What makes the float32 rounding visible is in the inputs: entries at +-fl32(hb), 0,
    float32 neighbours of interior heat-map edges, a zero pair distance, and samples that
    a_ - HALF_BOX does not give back."""
    for name in CASES:
        z, hb = fixture[name + "/z"], float(fixture[name + "/half_box"])
        hbf = np.float32(hb)
        assert (z == hbf).any() and (z == -hbf).any() and (z == 0).any()
        e = np.float32(np.linspace(-hb, hb, 100)[49])
        assert (z == np.nextafter(e, np.float32(np.inf))).any() and (z == np.nextafter(e, np.float32(-np.inf))).any()
        assert (z[1, 0] == z[1, 1]).all()
        assert ((z + hbf) - hbf != z).any()
        assert fixture[name + "/hist_relative"].shape == (99, 99)
    assert fixture["n3/z"].shape == (300, 3, 2) and fixture["n16/z"].shape == (150, 16, 2)


@pytest.mark.parametrize("interval,cycles,want", [(10, 25, [10, 20, 25]), (3, 7, [3, 6, 7])])
def test_checkpoint_rule(interval, cycles, want):
    """The analysis (:485) and, through the precedence of `% CHECKPOINT_INTERVAL*2` (:468),
    the model saves fall on the same cycles."""
    assert [c + 1 for c in range(cycles) if is_checkpoint_cycle(c, interval, cycles)] == want
    assert [c + 1 for c in range(cycles) if saves_model(c, interval, cycles)] == want
    for c in range(cycles):  # the reference's own expression
        assert saves_model(c, interval, cycles) == ((c + 1) % interval*2 == 0 or c == cycles - 1)  # noqa: E226


def test_writers_round_trip(tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(0)
    hist = rng.integers(0, 50, (99, 99))
    edges = np.linspace(-5.0, 5.0, 100)
    p = io.write_frequency_heatmap(d, 4, hist, edges, edges, cmap_name="ICL_diverging")
    assert os.path.basename(p) == "frequency_heatmap_cycle_4_data.json"
    data = json.load(open(p))
    assert sorted(data) == ["cmap_name", "hist_relative", "x_edges", "y_edges"]
    np.testing.assert_array_equal(np.array(data["hist_relative"]), hist.astype(np.float64) / hist.sum())
    np.testing.assert_array_equal(np.array(data["x_edges"]), edges)
    np.testing.assert_array_equal(np.array(data["y_edges"]), edges)
    assert data["cmap_name"] == "ICL_diverging"
    assert json.load(open(io.write_frequency_heatmap(d, 5, torch.from_numpy(hist), edges, edges)))["cmap_name"] is None

    r, g = np.arange(0, 5.0, 0.1), rng.random(50)
    p = io.write_pair_correlation(d, 4, r, g)
    assert os.path.basename(p) == "pair_correlation_function_4_data.json"
    data = json.load(open(p))
    assert sorted(data) == ["directory", "g_r", "r"]
    np.testing.assert_array_equal(np.array(data["r"]), r)
    np.testing.assert_array_equal(np.array(data["g_r"]), g)
    assert data["directory"] == d + "/"

    s = rng.random((7, 3, 2)).astype(np.float32)
    p = io.save_samples(d, torch.from_numpy(s))
    assert os.path.basename(p) == "samples.npy"
    back = np.load(p)
    assert back.dtype == np.float32
    np.testing.assert_array_equal(back, s)

    p = io.write_loss_history(d, [1.5, -0.25])
    assert os.path.basename(p) == "loss_function_data.json"
    assert json.load(open(p)) == {"loss_epoch": [1.5, -0.25]}

    m = torch.nn.Linear(3, 2)
    p = io.save_model_checkpoint(d, 6, m)
    assert os.path.basename(p) == "model_checkpoint_cycle_6.pth"
    sd = torch.load(p, weights_only=True)
    m2 = torch.nn.Linear(3, 2)
    m2.load_state_dict(sd, strict=True)
    assert torch.equal(m2.weight, m.weight)


@pytest.mark.parametrize("cycles", [1, 4])
def test_p_acc_history_file(tmp_path, cycles):
    p_acc = [0.0] + [0.01 * (i + 1) for i in range(cycles)]
    p = io.write_p_acc_history(str(tmp_path), p_acc, 20000, 1000)
    assert os.path.basename(p) == "p_acc_history_data.json"
    txt = open(p).read()
    data = json.loads(txt)
    assert sorted(data) == ["p_acc_history", "total_samples_trained"]
    assert len(data["p_acc_history"]) == len(data["total_samples_trained"]) == cycles + 1
    assert data["total_samples_trained"] == [20000 + 1000 * i for i in range(cycles + 1)]
    assert data["p_acc_history"] == p_acc
    assert txt == json.dumps(data, indent=4)  # main_algorithm_2.py:599


def test_algorithm2_defaults_unchanged():
    """Without checkpoint_interval the driver is the one from before: the same attribute
    values, run(cycles, speculate=None), and run() never enters the checkpoint path."""
    a = Algorithm2(types.SimpleNamespace(C=100), torch.nn.Linear(2, 2), graphed=False)
    want = dict(batch_size=256, lr=0.000543510751759681, wd=9.5857178422352e-05, alpha=1.0, sf=10, group=None, world=1,
                production_runs=100, cumulative=False, training_data=None, total_mcmc_steps=0, loss_history=[],
                p_acc_history=[], mcmc_steps_history=[], graphed=False)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    assert a.checkpoint_interval is None and a.out_dir is None and a.num_samples_for_analysis == 50000
    assert a.initial_p_acc == 0.0 and a.cmap_name is None
    sig = inspect.signature(Algorithm2.run)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [
        ("self", inspect.Parameter.empty), ("cycles", inspect.Parameter.empty), ("speculate", None)]
    init = inspect.signature(Algorithm2.__init__).parameters
    assert [init[k].default for k in ("checkpoint_interval", "num_samples_for_analysis", "out_dir", "initial_p_acc",
                                      "cmap_name")] == [None, 50000, None, 0.0, None]
    with pytest.raises(ValueError, match="out_dir"):
        Algorithm2(types.SimpleNamespace(C=100), torch.nn.Linear(2, 2), graphed=False, checkpoint_interval=2)


def test_abi_declares_and_checks_fs_sample_analysis():
    """Header, ctypes table and library agree on the symbol; out-of-range sizes return
    FS_EINVAL with a message before anything is launched; M = 0 is a successful no-op."""
    from test_host_cpu import header_symbols

    L = _lib.load()
    assert "fs_sample_analysis" in header_symbols() and "fs_sample_analysis" in _lib.EXPORTED
    assert hasattr(L, "fs_sample_analysis")
    one = ctypes.c_void_p(1)  # never dereferenced
    for N, nb, nr, word in ((16, 121, 50, b"nbins"), (16, 99, 129, b"r_nbins"), (257, 99, 50, b"N <= 256")):
        rc = L.fs_sample_analysis(one, 4, N, 5.0, one, nb, one, nr, one, one, one, None)
        assert rc == -1 and b"fs_sample_analysis" in L.fs_last_error() and word in L.fs_last_error()
    assert L.fs_sample_analysis(one, 4, 16, 5.0, None, 99, one, 50, one, one, one, None) == -1
    assert L.fs_sample_analysis(None, 0, 16, 5.0, one, 99, one, 50, None, None, None, None) == 0
