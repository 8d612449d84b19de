"""The wide path of the general-shape mode (small batches, csrc/flow_general_kernels.hip
"Wide path"): the pass as 2 L + 1 launches on 32-row tiles.  It must be bit-identical to
flow_general_kernel in every pass mode, at every shape class and ragged batch size, under
the fused MH step's multi-step launches and inside a captured graph;
fs_general_wide_passes proves which path ran."""
import functools

import numpy as np
import pytest
import torch

from flowstate import _lib
from flowstate.MCMC import BatchedMonteCarlo, Physics
from flowstate.models import flow_from_state_dict, half_box
from oracle import flow as OF
from oracle import physics as OP
from test_gpu_general import MODE, SHAPES, _propose, case, check_against_oracle, model_of

pytestmark = pytest.mark.gpu

ALL = 65536


class general_wide_rows:
    """Set the general-shape wide-path row limit for a block (0 = always the fused kernel)."""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        self.prev = _lib.load().fs_set_general_wide_rows(self.rows)

    def __exit__(self, *exc):
        _lib.load().fs_set_general_wide_rows(self.prev)


def passes():
    return _lib.load().fs_general_wide_passes()


@functools.lru_cache(maxsize=None)
def model(shape):
    return model_of(shape)


def _three_passes(m, x, z0):
    lq = m.log_prob(x)
    z = m.inverse(x)
    xs, ld = m.forward_and_log_det(z0)
    torch.cuda.synchronize()
    return lq, z, xs, ld


@pytest.mark.parametrize("B", [1, 31, 33, 65, 200])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bit_identical_to_fused_kernel(shape, B):
    _, _, ref = case(shape)
    m = model(shape)
    x = ref["x"][-B:].cuda()  # the last rows: the two outside the box (one at B = 1) included
    z0 = ref["z0"][:B].cuda()
    with general_wide_rows(0):
        n0 = passes()
        fused = _three_passes(m, x, z0)
        assert passes() == n0
    with general_wide_rows(ALL):
        n0 = passes()
        wide = _three_passes(m, x, z0)
        assert passes() == n0 + 3
    for name, a, b in zip(("log_prob", "inverse", "samples", "log_det"), fused, wide):
        assert torch.equal(a, b), name
    outside = min(B, 2)
    assert torch.isneginf(wide[0][-outside:]).all() and torch.isfinite(wide[0][:-outside]).all()


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5]], ids=str)
def test_propose_bit_identical(shape):
    """Base draws keyed by the global row: equal on both paths, and a shard starting at row
    100 draws rows 100.. of the whole."""
    dims, _, _ = case(shape)
    m = model(shape)
    with general_wide_rows(0):
        n0 = passes()
        fused = _propose(m, dims, 300, 3, 5, 1000)
        assert passes() == n0
    with general_wide_rows(ALL):
        wide = _propose(m, dims, 300, 3, 5, 1000)
        shard = _propose(m, dims, 50, 3, 5, 1100)
        assert passes() == n0 + 2
    for name, a, b in zip(("config", "centered", "x", "log_q"), fused, wide):
        assert torch.equal(a, b), name
    for name, a, b in zip(("config", "centered", "x", "log_q"), shard, wide):
        assert torch.equal(a, b[100:150]), name
    assert not torch.equal(wide[0][0], wide[0][1])  # rows draw different proposals


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5]], ids=str)
def test_wide_path_matches_oracle(shape):
    with general_wide_rows(ALL):
        n0 = passes()
        check_against_oracle(model(shape), shape)
        assert passes() == n0 + 3


def test_mh_engine_bit_identical():
    """step(3) as one multi-step launch (1536 proposal rows keyed by rows_per_counter) and
    three single steps, on both paths: every chain ends in the same place, bit for bit."""
    N, C = 16, 512
    dims_kw = dict(L=3, H=96, nb=1, K=10)
    dims = OF.FlowDims(N=N, B=half_box(N), **dims_kw)
    sd = OF.random_state_dict(dims, seed=6)
    m = flow_from_state_dict(sd, N, bound=dims.B, **dims_kw).set_precision(MODE)
    L = float(np.sqrt(N / 0.03))
    init = np.mod(OP.fcc_lattice(N)[None] + np.random.default_rng(4).normal(0, 0.05, (C, N, 2)), L)
    seeds = np.arange(42, 42 + C, dtype=np.uint64)
    names = ("state", "E_old", "W_old", "nll_old", "pcg", "accept", "attempts", "accepted", "n_accept")

    def run(multi):
        bmc = BatchedMonteCarlo(m, init, Physics(L, L), seeds, chain_offset=1000)
        if multi:
            assert bmc.steps_per_launch() > 1
            bmc.step(3)
        else:
            bmc.MAX_STEPS_PER_LAUNCH = 1
            for _ in range(3):
                bmc.step()
        bmc.check_errors()
        assert bmc.step_count == 3
        return [getattr(bmc, n).clone() for n in names]

    runs = []
    for limit in (0, ALL):
        with general_wide_rows(limit):
            for multi in (True, False):
                n0 = passes()
                runs.append(run(multi))
                assert (passes() > n0) == (limit > 0)
    for other in runs[1:]:
        for n, a, b in zip(names, runs[0], other):
            assert torch.equal(a, b), n
    assert int(runs[0][names.index("accepted")].sum().item()) > 0


def test_limit_is_respected():
    shape = SHAPES[2]
    _, _, ref = case(shape)
    m = model(shape)
    x = ref["x"][:65].cuda()
    with general_wide_rows(ALL):
        n0 = passes()
        wide = m.log_prob(x)
        assert passes() == n0 + 1
    with general_wide_rows(64):
        n0 = passes()
        at_limit = m.log_prob(x)
        assert passes() == n0  # 65 rows > 64: the fused kernel
        below = m.log_prob(x[:64])
        assert passes() == n0 + 1
    assert torch.equal(at_limit, wide) and torch.equal(below, wide[:64])


def test_captured_graph_replays_the_wide_path():
    """A density pass captured on a stream that already owns a workspace replays the wide
    path; on a stream without one the capture silently takes the fused kernel (the
    workspace is never allocated during capture).  Both give the eager fused results."""
    shape = SHAPES[2]
    dims, _, ref = case(shape)
    m = model(shape)
    lib, p = _lib.load(), _lib.ptr
    inputs = [ref["x"][:100].cuda(), ref["x"][100:200].cuda()]
    with general_wide_rows(0):
        want = [m.log_prob(x) for x in inputs]
    packed, fdims = m.packed(), m.dims()
    x_static = torch.zeros_like(inputs[0])
    z, lq = torch.empty_like(x_static), torch.empty(100, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def launch():
        _lib.check(lib.fs_flow_log_prob(fdims, p(packed), p(x_static), 100, p(lq), p(z), p(err), _lib.stream_ptr()),
                   "fs_flow_log_prob")

    with general_wide_rows(ALL):
        for warm in (True, False):
            side = torch.cuda.Stream()
            if warm:  # one eager pass creates this stream's workspace
                n0 = passes()
                with torch.cuda.stream(side):
                    launch()
                side.synchronize()
                assert passes() == n0 + 1
            graph = torch.cuda.CUDAGraph()
            n0 = passes()
            with torch.cuda.graph(graph, stream=side):
                launch()
            if warm:
                assert passes() == n0 + 1  # the captured launches are the wide path's
            for x, w in zip(inputs, want):
                x_static.copy_(x)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(lq, w), warm
            del graph
    assert int(err.item()) == 0
