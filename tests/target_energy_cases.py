"""Inputs and CPU references shared by test_target_energy_cpu.py and
test_gpu_target_energy.py: DoubleWellLJ / SimpleLJ (flowstate/normflows/Energy.py) away from
the drivers' constants and particle counts.

The reference is the torch restatement evaluated in float64 on the float32 inputs
(x.double()), autograd for dE/dx.  The same restatement in float32 is a second reference: it
sizes the tolerance (its own error against float64, per case) and carries torch's NaN
gradient quirks natively.  Everything here runs on the CPU and is computed once per case."""
import functools

import numpy as np
import torch

from flowstate.normflows.Energy import DoubleWellLJ, SimpleLJ
from oracle import flow as OF
from oracle import physics as OP

EPS32 = 2.0 ** -23
BK = 0.82  # SimpleLJ's core radius: the energy jumps by ~0.1 there

# N -> the branch it reaches (M = N + 1 staged points; 64 lanes; 256-strided staging)
NS = (3, 5, 63, 65, 100, 129, 255, 256, 300)
ROWS = 7
ROW_COUNTS = (1, 2, 3, 5, 7)   # at N = 5 and N = 65: the gradient kernel's four-row workgroups
CONSTS = {
    "drivers": dict(T=1.0, V0=(-10.0, -10.5), r0=1.2, k=15.0),
    "alt": dict(T=0.7, V0=(-3.0, 2.5), r0=0.9, k=6.0),
    "hot": dict(T=2.5, V0=(-3.0, 2.5), r0=0.9, k=6.0),   # N = 5 and N = 65 only
}
CASES = [(N, c) for N in NS for c in ("drivers", "alt")] + [(5, "hot"), (65, "hot")]


def bound_of(N):
    return float(OF.half_box(N))


def make_mod(N, cset, wells=2):
    """The module the kernel is checked against: two wells (DoubleWellLJ), one (centers /
    V0_list cut to the first) or none (SimpleLJ)."""
    c = CONSTS[cset]
    if wells == 0:
        return SimpleLJ(2 * N, N, c["T"], bound_of(N))
    mod = DoubleWellLJ(2 * N, N, c["T"], bound_of(N), V0_list=list(c["V0"]), r0=c["r0"], k=c["k"])
    if wells == 1:
        mod.centers = mod.centers[:1].clone()
        mod.V0_list = mod.V0_list[:1].clone()
    return mod


def restatement(mod, x):
    """The torch restatement (never the device kernel), in x's dtype."""
    return mod._energy_torch(x) if isinstance(mod, DoubleWellLJ) else mod._energy(x)


def weights(rows, dtype=torch.float64):
    return torch.linspace(0.5, 1.5, rows, dtype=dtype)  # one row: 0.5, never E.sum()


def energy_and_grad(mod, x):
    """E and d((E * w).sum())/dx by autograd through the restatement, in x's dtype."""
    x = x.detach().clone().requires_grad_(True)
    E = restatement(mod, x)
    (g,) = torch.autograd.grad((E * weights(len(E), E.dtype)).sum(), x)
    return E.detach(), g


def staged(x64, bound):
    """(rows, M, 2) float64: the origin particle, then each particle wrapped into the box."""
    xp = x64.reshape(x64.shape[0], -1, 2)
    d = xp - 2 * bound * torch.round(xp / (2 * bound))
    return torch.cat((torch.zeros_like(d[:, :1]), d), dim=1)


def pair_distances(x64, bound):
    """(rows, M (M - 1) / 2) float64 distances of all unordered staged pairs."""
    s = staged(x64, bound)
    M = s.shape[1]
    iu = torch.triu_indices(M, M, offset=1)
    return (s[:, iu[0]] - s[:, iu[1]]).norm(dim=-1)


def energy_scale(mod, x64):
    """S per row: the float64 sum of |pair energy| / T plus |well terms| (what the energy's
    float32 error is measured against: E itself cancels between pairs and wells)."""
    r = pair_distances(x64, mod.bound)
    en = torch.where(r <= BK, -80 * (r - BK) + 30, 4 * ((1 / r) ** 12 - (1 / r) ** 6))
    S = en.abs().sum(dim=1) / mod.temperature
    if isinstance(mod, DoubleWellLJ):
        L = 2 * mod.bound
        xp = x64.reshape(x64.shape[0], -1, 2)
        for c, v in zip(mod.centers.double(), mod.V0_list.double()):
            dx = xp[:, :, 0] - c[0]
            dy = xp[:, :, 1] - c[1]
            dx = dx - L * torch.round(dx / L)
            dy = dy - L * torch.round(dy / L)
            rr = torch.sqrt(dx ** 2 + dy ** 2)
            S = S + (v * (1 - 0.5 * (1 + torch.tanh(mod.k * (rr - mod.r0))))).abs().sum(dim=1)
    return S


def wrap_margin(x64, bound):
    """Smallest distance of a coordinate to a half-way point of the particle wrap
    (|x| = bound, 3 bound, ...), in units of bound."""
    t = x64 / (2 * bound)
    return float(((t - torch.floor(t)) - 0.5).abs().min()) * 2


# --- kind 1: uniform rows -----------------------------------------------------------------
def uniform_ok(x, bound):
    r = pair_distances(x.double(), bound)
    return bool(((r - BK).abs() >= 1e-3).all() and (r >= 0.02).all() and wrap_margin(x.double(), bound) >= 1e-5)


def uniform_rows(N):
    """ROWS rows uniform in +-1.3 bound (so the per-particle wrap acts), re-drawn by seed
    until no pair sits at the core radius or nearly coincides and no coordinate sits on a
    wrap half-way point: there the float64 reference itself is not defined to 1e-7."""
    bound = bound_of(N)
    for attempt in range(50):
        g = torch.Generator().manual_seed(N + 1000 * attempt)
        x = ((torch.rand((ROWS, 2 * N), generator=g) * 2 - 1) * (1.3 * bound)).float()
        if uniform_ok(x, bound):
            return x
    raise AssertionError(f"no admissible uniform rows at N={N}")


# --- kind 2: pair-census rows ---------------------------------------------------------------
def census_pairs(N):
    """Staged-index pairs (a < b; 0 is the origin particle, p + 1 particle p) that sit on the
    edges of both kernels' pair enumerations."""
    M = N + 1
    D = M // 2
    want = [(0, 1), (0, D), (0, M - 1), (1, 2), (1, 1 + D), (D - 1, M - 1), (D, D + 1), (M - 2, M - 1), (1, M - 1)]
    if N > 64:  # particles that share a lane of the gradient kernel
        want += [(p + 1, p + 65) for p in (0, N - 65)]
    if N > 128:
        want += [(1, 129)]
    out = []
    for a, b in want:
        if 0 <= a < b < M and (a, b) not in out:
            out.append((a, b))
    return out


_SHIFTS = [(0.0, 0.0)] + [(0.61 * k, 0.37 * k) for k in range(1, 40)]


def census_rows(N):
    """One row per census pair: the FCC lattice of the golden generator (spacing >= 5.7, far
    pairs worth ~1e-4) with particle b put at a + (0.9, 0), a single pair worth ~ +6.6 / T.
    The lattice is shifted by a constant until that pair is the only one with r < 2."""
    bound = bound_of(N)
    base = torch.from_numpy(OP.fcc_lattice(N) - bound)
    rows = []
    for a, b in census_pairs(N):
        for sx, sy in _SHIFTS:
            p = base + torch.tensor([sx, sy], dtype=torch.float64)
            p = p.float()
            src = p[a - 1] if a > 0 else torch.zeros(2)
            p[b - 1] = src + torch.tensor([0.9, 0.0])
            x = p.reshape(1, -1)
            if int((pair_distances(x.double(), bound) < 2).sum()) == 1 and wrap_margin(x.double(), bound) >= 1e-5:
                rows.append(x)
                break
        else:
            raise AssertionError(f"no admissible lattice shift at N={N} pair {(a, b)}")
    return torch.cat(rows)


# --- kind 3: dense core rows ----------------------------------------------------------------
def dense_rows(N):
    """Two rows with every particle inside a disc of radius 0.4 around (1, 1): every
    particle pair in the linear core (30 .. 95 each).  Re-drawn until no pair is closer than
    1e-3 ((1/r)^11 overflows float32 below 3.2e-4: that is an edge case, tested apart)."""
    bound = bound_of(N)
    for attempt in range(200):
        g = torch.Generator().manual_seed(7000 + N + 1000 * attempt)
        rad = 0.4 * torch.sqrt(torch.rand((2, N), generator=g))
        ang = 2 * np.pi * torch.rand((2, N), generator=g)
        x = torch.stack((1 + rad * torch.cos(ang), 1 + rad * torch.sin(ang)), dim=-1).reshape(2, 2 * N).float()
        r = pair_distances(x.double(), bound)
        if bool((r >= 1e-3).all() and ((r - BK).abs() >= 1e-3).all()):
            return x
    raise AssertionError(f"no admissible dense rows at N={N}")


# --- kind 4: rows inside the wells --------------------------------------------------------------
def well_particles(N):
    """The particles put around the well centres: the first and the last ones (at N > 64 the
    last shares a lane of the gradient kernel with an earlier one)."""
    return sorted({p for p in (0, 1, 2, 3, N - 2, N - 1) if 0 <= p < N})


def wells_rows(N):
    """ROWS rows on the shifted lattice with up to six particles at 0.15 .. 1.3 from a well centre
    (alternating wells; every other one displaced by a box length, +-2 bound in x or y, which
    the wells' minimum image on the raw coordinates must undo).  Uniform rows leave the wells
    nearly empty; here the well terms are most of the energy scale.  Re-drawn until no pair
    is closer than 1 (so the LJ part stays small) and nothing sits on a wrap half-way point."""
    bound = bound_of(N)
    base = (torch.from_numpy(OP.fcc_lattice(N) - bound) + torch.tensor([0.61, 0.37], dtype=torch.float64)).float()
    placed = well_particles(N)
    rows, attempt = [], 0
    while len(rows) < ROWS:
        attempt += 1
        assert attempt < 2000, f"no admissible wells rows at N={N}"
        g = torch.Generator().manual_seed(9000 + N + 1000 * attempt)
        p = base.clone()
        for i, q in enumerate(placed):
            rad = 0.15 + 1.15 * float(torch.rand((), generator=g))
            ang = 2 * np.pi * float(torch.rand((), generator=g))
            cx = -bound / 2 if i % 2 == 0 else bound / 2
            pos = [cx + rad * np.cos(ang), rad * np.sin(ang)]
            if i % 4 == 1:
                pos[0] += -2 * bound if cx > 0 else 2 * bound
            if i % 4 == 2:
                pos[1] += 2 * bound if i % 8 == 2 else -2 * bound
            p[q] = torch.tensor(pos, dtype=torch.float64).float()
        x = p.reshape(1, -1)
        if float(pair_distances(x.double(), bound).min()) >= 1.0 and wrap_margin(x.double(), bound) >= 1e-5:
            rows.append(x)
    return torch.cat(rows)


KINDS = {"uniform": uniform_rows, "census": census_rows, "dense": dense_rows, "wells": wells_rows}


@functools.lru_cache(maxsize=None)
def inputs(N, kind):
    return KINDS[kind](N)


class Ref:
    """One (module, input) case: float64 and float32 restatements and the float32 one's
    own error envelope (u32 on energies over S, v32 on gradients over the row's max |g64|)."""

    def __init__(self, mod, x):
        self.x = x
        self.E64, self.g64 = energy_and_grad(mod, x.double())
        self.E32, self.g32 = energy_and_grad(mod, x)
        self.S = energy_scale(mod, x.double())
        fin = torch.isfinite(self.g64)
        self.gmax = torch.where(fin, self.g64.abs(), torch.zeros_like(self.g64)).max(dim=1).values
        self.u32 = self.u(self.E32)
        self.v32 = self.v(self.g32, mask=fin & torch.isfinite(self.g32))

    def u(self, E):
        return float(((E.double().cpu() - self.E64).abs() / self.S).max())

    def v(self, g, mask=None):
        err = (g.double().cpu() - self.g64).abs() / self.gmax[:, None]
        if mask is not None:
            err = torch.where(mask, err, torch.zeros_like(err))
        return float(err.max())


@functools.lru_cache(maxsize=None)
def reference(N, cset, kind, wells=2, rows=None):
    """The case's references, computed once; rows: only the first so many rows (with
    their own gradient weights)."""
    return Ref(make_mod(N, cset, wells), inputs(N, kind)[:rows])


# --- exact edges ------------------------------------------------------------------------------
EDGE_NS = (5, 65)
EDGE_NAMES = ("coincide", "well_centre", "on_origin", "overflow", "core_origin", "core_origin_up", "core_pair",
              "core_pair_up")


def edge_particles(N):
    """The two particles the edge rows act on: at N = 65 they share lane 0 of the gradient
    kernel (p and p + 64)."""
    return (0, 64) if N > 64 else (1, 3)


@functools.lru_cache(maxsize=None)
def edge_rows(N):
    """Rows on which torch's float32 autograd returns NaN gradients, and rows with a pair at
    exactly the (inclusive) core radius in float32 and one float above it.  Built on the
    census lattice, shifted so that nothing else is close."""
    bound = bound_of(N)
    pa, pb = edge_particles(N)
    base = (torch.from_numpy(OP.fcc_lattice(N) - bound) + torch.tensor([0.61, 0.37], dtype=torch.float64)).float()
    bk = np.float32(0.82)
    up = np.nextafter(bk, np.float32(1))
    rows = {}
    p = base.clone()
    p[pb] = p[pa]
    rows["coincide"] = p
    p = base.clone()
    p[pb] = torch.tensor([np.float32(-bound / 2), 0.0])
    rows["well_centre"] = p
    p = base.clone()
    p[pa] = torch.zeros(2)
    rows["on_origin"] = p
    p = base.clone()
    p[pb] = p[pa] + torch.tensor([2e-4, 0.0])
    rows["overflow"] = p
    for name, r in (("core_origin", bk), ("core_origin_up", up)):
        p = base.clone()
        p[pb] = torch.tensor([float(r), 0.0])   # sqrt(fl(r^2)) == r in binary floating point
        rows[name] = p
    for name, r in (("core_pair", bk), ("core_pair_up", up)):
        p = base.clone()
        p[pa] = torch.tensor([-0.25, 1.5])
        p[pb] = torch.tensor([float(np.float32(r - np.float32(0.25))), 1.5])   # exact: the difference is r
        rows[name] = p
    return torch.stack([rows[n].reshape(-1) for n in EDGE_NAMES])


def expected_nan_particles(N):
    """Per edge row, the particles whose four / two gradient entries torch makes NaN."""
    pa, pb = edge_particles(N)
    return {"coincide": {pa, pb}, "well_centre": {pb}, "on_origin": {pa}, "overflow": {pa, pb},
            "core_origin": set(), "core_origin_up": set(), "core_pair": set(), "core_pair_up": set()}


@functools.lru_cache(maxsize=None)
def edge_reference(N, cset="alt"):
    return Ref(make_mod(N, cset), edge_rows(N))
