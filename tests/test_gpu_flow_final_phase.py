"""The final-layer phase of the f32 flow pass (csrc/flow_kernels.hip cond_spline /
spline_from_logits: the final tiles' operands issued ahead of their GEMMs, the bin found
by bisection with the bin's knots carried along) on inputs that sit on the search's edges.

Every case is a small flow (L=2, one residual block) at one of the kernel's (H, K)
instantiations, N = 2 and 3 transform features, 65 rows: one full 64-row workgroup and
one with a single row.  The transform coordinates that the FIRST conditional spline of
the pass sees are planted from the oracle's own float32 knots of that spline (computed
here on the CPU with the reference's op sequence, oracle/flow.py rqs_core):
  knot      exactly an interior knot
  last-     the last knot minus the searchsorted eps (1e-6, in float32)
  last      the last knot, +B itself (the eps keeps it in the last bin)
  last+     the last knot plus the eps: where float32 resolves it, outside the bound
            (identity, log q = -inf); where it rounds back to +B, the same as `last`
  first     -B, the first knot
  bin0      the middle of bin 0
  binK      the middle of bin K-1
The later layer sees whatever the first one made of them.  Tolerances are those of
test_gpu_flow.py, unchanged: log q within 1e-5 relative + 1e-4, latents within 2e-4 B,
samples within 5e-4 B, the sampling log-det within 1e-4 relative + 1e-3, on every row whose
coordinates do not leave the box on the way (see beyond()).  The fused kernel and the
wide path must agree bit for bit on every row."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import flow as OF

RTOL, ATOL = 1e-5, 1e-4
ROWS = 65
SHAPES = [(256, 32), (128, 32), (128, 15), (64, 8), (32, 5)]
CASES = [(H, K, N) for (H, K) in SHAPES for N in (2, 3)]
IDS = [f"h{H}-k{K}-n{N}" for (H, K, N) in CASES]
KINDS = ("knot", "last-", "last", "last+", "first", "bin0", "binK")
EPS = np.float32(1e-6)  # splines.py:11-13


def close(a, b, rtol=RTOL, atol=ATOL):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin])
    err = np.abs(a[fin] - b[fin])
    bad = err > rtol * np.abs(b[fin]) + atol
    assert not bad.any(), f"{bad.sum()} / {bad.size} out of tolerance; worst rel {np.max(err / (np.abs(b[fin]) + 1e-30))}"


def oracle_knots(u, B):
    """cumwidths / cumheights of rqs_core from their logits, the same float32 ops."""
    K = u.shape[-1]
    w = F.softmax(u, dim=-1)
    w = OF.MIN_W + (1 - OF.MIN_W * K) * w
    c = F.pad(torch.cumsum(w, dim=-1), pad=(1, 0), mode="constant", value=0.0)
    c = (B - -B) * c + -B
    c[..., 0] = -B
    c[..., -1] = B
    return c


def first_spline_knots(sd, u, dims, inverse):
    """Searched knots [rows, N, K+1] of the first conditional spline of a pass over the
    coupling input u (sampling: after the roll), and the layer's parameters."""
    lp = OF.layer_params(sd, 0 if inverse else dims.L - 1)
    ident = u[:, lp["idf"]]
    if inverse:
        ident, _ = OF._uncond_spline(lp, ident, dims.B, inverse=True)
    params = OF.conditioner(lp, ident, dims.B).reshape(len(u), dims.N, -1)
    K = dims.K
    logits = (params[..., K:2 * K] if inverse else params[..., :K]) / np.sqrt(dims.H)
    return oracle_knots(logits, dims.B), lp


def planted(dims, sd, seed, inverse):
    """[ROWS, D] inputs of a pass (x for the density direction, z for sampling) whose first
    conditional spline meets every KINDS value in every transform feature, and the kind of
    each (row, feature)."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand((ROWS, dims.D), generator=g) * 2 - 1) * dims.B
    split = dims.D // 2
    u = torch.cat([v[:, split:], v[:, :split]], dim=1) if inverse else v.clone()
    kn, lp = first_spline_knots(sd, u, dims, inverse)
    kn = kn.numpy()
    B32 = np.float32(dims.B)
    kinds = np.empty((ROWS, dims.N), dtype=object)
    for r in range(ROWS):
        for t in range(dims.N):
            kind = KINDS[(r + 3 * t) % len(KINDS)]
            k = kn[r, t]
            val = {"knot": k[1 + (r // len(KINDS)) % (dims.K - 1)], "last-": B32 - EPS, "last": B32, "last+": B32 + EPS,
                   "first": -B32, "bin0": np.float32(0.5) * (k[0] + k[1]),
                   "binK": np.float32(0.5) * (k[-2] + k[-1])}[kind]
            u[r, int(lp["trf"][t])] = float(np.float32(val))
            kinds[r, t] = kind
    v = torch.cat([u[:, split:], u[:, :split]], dim=1) if inverse else u  # undo the roll (D = 2 split)
    # the planting left the conditioner's inputs alone: same knots, and each value where it was meant to be
    kn2, _ = first_spline_knots(sd, torch.cat([v[:, split:], v[:, :split]], dim=1) if inverse else v, dims, inverse)
    assert np.array_equal(kn2.numpy(), kn)
    return v.contiguous(), kinds, kn, lp


@functools.lru_cache(maxsize=None)
def case(H, K, N):
    dims = OF.FlowDims(N=N, L=2, H=H, nb=1, K=K, B=OF.half_box(N))
    sd = OF.random_state_dict(dims, seed=100 + H + K + N)
    x, kx, knx, lpx = planted(dims, sd, 1, inverse=False)
    z, kz, knz, lpz = planted(dims, sd, 2, inverse=True)
    lq, zlat, _ = OF.log_prob(sd, x.clone(), dims, per_layer=True)
    xs, ld = OF.sample_from(sd, z.clone(), dims, with_logdet=True)
    return dict(dims=dims, sd=sd, x=x, z=z, kx=kx, kz=kz, knx=knx, knz=knz, lpx=lpx, lpz=lpz,
                lq=lq.numpy(), zlat=zlat.numpy(), xs=xs.numpy(), ld=ld.numpy())


@pytest.mark.parametrize("H,K,N", CASES, ids=IDS)
def test_oracle_is_finite_on_the_planted_inputs(H, K, N):
    """No GPU: the inputs hit what they are meant to hit, and the oracle itself is finite
    on them (log q is -inf exactly on the rows with a coordinate beyond +B)."""
    c = case(H, K, N)
    dims = c["dims"]
    B32 = np.float32(dims.B)
    split = dims.D // 2
    for v, kinds, kn, lp, inverse in ((c["x"], c["kx"], c["knx"], c["lpx"], False),
                                      (c["z"], c["kz"], c["knz"], c["lpz"], True)):
        u = torch.cat([v[:, split:], v[:, :split]], dim=1).numpy() if inverse else v.numpy()
        seen = set()
        for r in range(ROWS):
            for t in range(dims.N):
                val, k, kind = u[r, int(lp["trf"][t])], kn[r, t], kinds[r, t]
                bin_ = int(np.sum(val >= np.concatenate([k[:-1], [k[-1] + EPS]]))) - 1
                seen.add(kind)
                if kind == "knot":
                    assert val in k[1:-1] and k[bin_] == val
                elif kind in ("last-", "last"):
                    assert bin_ == dims.K - 1 and val <= B32
                elif kind == "last+":
                    assert val >= B32
                elif kind == "first":
                    assert val == -B32 and bin_ == 0
                elif kind == "bin0":
                    assert bin_ == 0
                else:
                    assert bin_ == dims.K - 1
        assert seen == set(KINDS)
    beyond_x = (c["x"].numpy() > B32).any(axis=1)
    assert np.isfinite(c["lq"][~beyond_x]).all() and np.isneginf(c["lq"][beyond_x]).all()
    assert np.isfinite(c["zlat"]).all() and np.isfinite(c["xs"]).all() and np.isfinite(c["ld"]).all()


def beyond(vec, B32):
    """Per row, the coordinates beyond +-fl32(B).  One that is outside on input (`last+`) is
    passed through by every layer, in the pass and in the oracle alike, and such a row is
    held to the full tolerance.  A coordinate planted ON +-B comes out of its spline on the
    box's edge, where float32 rounding decides whether it is a last ulp inside or outside
    (the reference's own root * width + knot lands one ulp beyond +B on some rows; the kernel
    pins the root to the bin).  Every later layer passes an outside coordinate through and
    conditions on it, which is another function of the input, so a row that has more
    coordinates outside at the end than it came with, in the pass or in the oracle, left the
    box on the way and is held to finiteness only (the rule of flow_sharp_cases.py's
    escaped_rows); only rows with a value planted on the edge may do so."""
    return (np.abs(np.asarray(vec, np.float64)) > B32).sum(axis=1)


class wide_rows:
    """Set the wide-path row limit for a block (0 = always the fused kernel)."""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        from flowstate import _lib

        self.prev = _lib.load().fs_set_wide_rows(self.rows)

    def __exit__(self, *exc):
        from flowstate import _lib

        _lib.load().fs_set_wide_rows(self.prev)


@pytest.mark.gpu
@pytest.mark.parametrize("H,K,N", CASES, ids=IDS)
def test_passes_match_oracle_and_wide_path_on_planted_inputs(H, K, N):
    from flowstate.models import flow_from_state_dict

    c = case(H, K, N)
    dims = c["dims"]
    m = flow_from_state_dict(c["sd"], N, dims.L, dims.H, dims.nb, dims.K, bound=dims.B)
    x, z = c["x"].cuda(), c["z"].cuda()

    def run():
        lq = m.log_prob(x).clone()
        zl = m.inverse(x).clone()
        xs, ld = m.forward_and_log_det(z)
        torch.cuda.synchronize()
        return lq, zl, xs.clone(), ld.clone()

    with wide_rows(0):
        fused = run()
    with wide_rows(16384):
        wide = run()
    for a, b in zip(fused, wide):
        assert torch.equal(a, b)
    lq, zl, xs, ld = (t.cpu().numpy() for t in fused)
    B32 = float(np.float32(dims.B))
    assert np.isneginf(lq[(c["x"].numpy() > B32).any(axis=1)]).all()  # an input beyond +B: log q = -inf
    edge = ("last-", "last", "last+", "first")
    for name, vec, vec_ref, sc, sc_ref, kinds, vtol, stol in (
            ("density", zl, c["zlat"], lq, c["lq"], c["kx"], 2e-4 * dims.B, (RTOL, ATOL)),
            ("sampling", xs, c["xs"], ld, c["ld"], c["kz"], 5e-4 * dims.B, (1e-4, 1e-3))):
        nin = beyond(c["x"] if name == "density" else c["z"], B32)
        esc = (beyond(vec, B32) != nin) | (beyond(vec_ref, B32) != nin)
        planted_edge = np.array([any(k in edge for k in row) for row in kinds])
        print(f"{name}: {esc.sum()} of {ROWS} rows left the box on the way, in the pass or in the oracle")
        assert not (esc & ~planted_edge).any(), np.flatnonzero(esc & ~planted_edge)
        assert np.isfinite(vec).all() and not np.isnan(sc).any() and not np.isposinf(sc).any()
        np.testing.assert_allclose(vec[~esc], vec_ref[~esc], rtol=0, atol=vtol)
        close(sc[~esc], sc_ref[~esc], *stol)
