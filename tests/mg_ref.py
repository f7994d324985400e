"""The expectation for the multigrid calls (stencil_restrict_residual,
stencil_prolong_add, stencil_residual_norms, stencil_mg_*): include/stencil_hip.h
"Geometric multigrid" stated in numpy.  A plain helper module for
tests/test_mg_ref.py (which pins it on hand-computed cells),
tests/test_gpu_mg.py and tests/golden/make_mg_golden.py.

Arrays are dense and ghost-padded (the oracle's layout) unless a name says
`interior`.  numpy's add, subtract and multiply are the IEEE operations in the
array's dtype, so every value below is the stated sequence of roundings:
  residual      source_ref.sweep (J = fl(fl(sum6 * avg) + g)), then J - u
  restriction   slices and adds along x, then y, then z, then * 0.0625
  prolongation  slices along x, then y, then z: odd indices are copies, even
                ones 0.5 * (lo + hi); then u + p
  V-cycle       plain recursion over relax_ref.sweeps
"""
from __future__ import annotations

import numpy as np

from tests import relax_ref as rr
from tests import source_ref as sr

NP = rr.NP
problem = sr.problem


def coarse_size(nx: int, ny: int, nz: int):
    assert all(n >= 3 and n % 2 == 1 for n in (nx, ny, nz)), (nx, ny, nz)
    return (nx - 1) // 2, (ny - 1) // 2, (nz - 1) // 2


def max_levels(nx: int, ny: int, nz: int) -> int:
    n = 1
    while all(m >= 3 and m % 2 == 1 for m in (nx, ny, nz)):
        nx, ny, nz = coarse_size(nx, ny, nz)
        n += 1
    return n


def residual(p, u: np.ndarray, g: np.ndarray) -> np.ndarray:
    """r = fl(J - u) at the interior cells: an (nz, ny, nx) array."""
    j = sr.sweep(p, u, g)
    with np.errstate(all="ignore"):
        return j[1:-1, 1:-1, 1:-1] - u[1:-1, 1:-1, 1:-1]


def weigh(v: np.ndarray, axis: int) -> np.ndarray:
    """The 1-D full weighting along `axis` (odd length n -> (n - 1) / 2):
    fl(fl(v(i-1) + v(i+1)) + fl(v(i) + v(i))), i = 2X + 1."""
    n = v.shape[axis]
    assert n % 2 == 1 and n >= 3

    def take(first):
        sl = [slice(None)] * v.ndim
        sl[axis] = slice(first, first + n - 2, 2)
        return v[tuple(sl)]

    lo, mid, hi = take(0), take(1), take(2)
    with np.errstate(all="ignore"):
        return (lo + hi) + (mid + mid)


def restrict(r: np.ndarray, order=(2, 1, 0)) -> np.ndarray:
    """g_c = fl(0.0625 * A_z(A_y(A_x(r)))) of an interior residual array
    (`order`: the axes in turn; the definition's is x, y, z = 2, 1, 0)."""
    a = r
    for axis in order:
        a = weigh(a, axis)
    with np.errstate(all="ignore"):
        return r.dtype.type(0.0625) * a


def restrict_residual(p, u: np.ndarray, g: np.ndarray) -> np.ndarray:
    """The coarse source's interior, (cnz, cny, cnx)."""
    return restrict(residual(p, u, g))


def interp(e: np.ndarray, axis: int) -> np.ndarray:
    """The 1-D interpolation along `axis`: m + 2 coarse cells (ghosts at the
    ends) -> 2 m + 1 fine cells; odd fine indices copy, even ones average."""
    m = e.shape[axis] - 2
    shape = list(e.shape)
    shape[axis] = 2 * m + 1
    out = np.empty(shape, dtype=e.dtype)

    def sl(arr, s):
        idx = [slice(None)] * arr.ndim
        idx[axis] = s
        return arr[tuple(idx)]

    with np.errstate(all="ignore"):
        sl(out, slice(0, None, 2))[...] = e.dtype.type(0.5) * (sl(e, slice(0, m + 1)) + sl(e, slice(1, m + 2)))
    sl(out, slice(1, None, 2))[...] = sl(e, slice(1, m + 1))
    return out


def prolong(e: np.ndarray, order=(2, 1, 0)) -> np.ndarray:
    """P(e) of a ghost-padded coarse array: the fine interior, (nz, ny, nx)."""
    a = e
    for axis in order:
        a = interp(a, axis)
    return a


def prolong_add(u: np.ndarray, e: np.ndarray, begin: int = 0, end: int | None = None) -> np.ndarray:
    """u + P(e) at the interior cells of fine planes [begin, end): a new array."""
    nz = u.shape[0] - 2
    end = nz if end is None else end
    out = u.copy()
    with np.errstate(all="ignore"):
        out[1 + begin:1 + end, 1:-1, 1:-1] = u[1 + begin:1 + end, 1:-1, 1:-1] + prolong(e)[begin:end]
    return out


def residual_norms(p, u: np.ndarray, g: np.ndarray):
    """stencil_residual_norms: per-plane max |d| and sum d*d, d = double(r);
    both NaN for a plane that holds a NaN."""
    with np.errstate(all="ignore"):
        d = residual(p, u, g).astype(np.float64)
        mx = np.array([np.nan if np.isnan(pl).any() else (np.abs(pl).max() if pl.size else 0.0) for pl in d])
        sq = np.array([float((pl * pl).sum()) for pl in d])
    sq[np.isnan(mx)] = np.nan
    return mx, sq


def residual_norm(p, u: np.ndarray, g: np.ndarray) -> float:
    """The scalar max norm of the residual (NaN if any plane is NaN)."""
    mx, _ = residual_norms(p, u, g)
    if np.isnan(mx).any():
        return float("nan")
    return float(mx.max()) if mx.size else 0.0


class Hierarchy:
    """Levels 0 (fine) .. L-1: problems, ghost-padded fields `u` and sources `g`."""

    def __init__(self, dtype: str, nx: int, ny: int, nz: int, levels: int, field: np.ndarray, source: np.ndarray):
        most = max_levels(nx, ny, nz)
        levels = most if levels == 0 else levels
        assert 1 <= levels <= most
        self.dtype, self.p, self.u, self.g = dtype, [], [], []
        for i in range(levels):
            self.p.append(problem(dtype, nx, ny, nz))
            shape = (nz + 2, ny + 2, nx + 2)
            self.u.append(field.astype(NP[dtype]).copy() if i == 0 else np.zeros(shape, dtype=NP[dtype]))
            self.g.append(source.astype(NP[dtype]).copy() if i == 0 else np.zeros(shape, dtype=NP[dtype]))
            if i + 1 < levels:
                nx, ny, nz = coarse_size(nx, ny, nz)
        assert self.u[0].shape == self.g[0].shape == (self.p[0].nz + 2, self.p[0].ny + 2, self.p[0].nx + 2)


def vcycle(h: Hierarchy, pre: int, post: int, coarse_sweeps: int, omegas, level: int = 0) -> None:
    """One V-cycle on `level` and below, in place on the hierarchy."""
    p = h.p[level]
    if level + 1 == len(h.p):
        h.u[level] = rr.sweeps(p, h.u[level], h.g[level], coarse_sweeps, omegas)
        return
    h.u[level] = rr.sweeps(p, h.u[level], h.g[level], pre, omegas)
    h.g[level + 1] = np.zeros_like(h.g[level + 1])
    h.g[level + 1][1:-1, 1:-1, 1:-1] = restrict_residual(p, h.u[level], h.g[level])
    h.u[level + 1] = np.zeros_like(h.u[level + 1])
    vcycle(h, pre, post, coarse_sweeps, omegas, level + 1)
    h.u[level] = prolong_add(h.u[level], h.u[level + 1])
    h.u[level] = rr.sweeps(p, h.u[level], h.g[level], post, omegas)


def solve(h: Hierarchy, tol: float, max_cycles: int, check_every: int, pre: int, post: int, coarse_sweeps: int, omegas):
    """stencil_mg_solve's stopping rule (max norm).  Returns (cycles done,
    converged, last norm, the norms of every check)."""
    done, last, history = 0, float("inf"), []
    while done < max_cycles:
        block = min(check_every, max_cycles - done)
        for _ in range(block):
            vcycle(h, pre, post, coarse_sweeps, omegas)
        done += block
        last = residual_norm(h.p[0], h.u[0], h.g[0])
        history.append(last)
        if last <= tol:
            return done, True, last, history
        if last != last:
            break
    return done, False, last, history


# The solve that tests/golden/mg_known_answers.json records (tests/golden/make_mg_golden.py) and
# tests/test_mg_ref.py / tests/test_gpu_mg.py repeat: 31^3 fp64, 4 levels, V(2,2), omega = 6/7, 8 coarse sweeps,
# from the reference initial field with a seeded uniform(-1, 1) * 1e-3 source.
GOLDEN = {"dtype": "fp64", "size": (31, 31, 31), "levels": 4, "pre": 2, "post": 2, "coarse_sweeps": 8,
          "omegas": (6.0 / 7.0,), "seed": 20260, "cycles": 6}


def golden_setup():
    """(ghost-padded field, ghost-padded source) of the GOLDEN solve."""
    from oracle import binding as ob
    nx, ny, nz = GOLDEN["size"]
    p = problem(GOLDEN["dtype"], nx, ny, nz)
    u = ob.init(p)
    g = np.zeros_like(u)
    g[1:-1, 1:-1, 1:-1] = np.random.default_rng(GOLDEN["seed"]).uniform(-1.0, 1.0, (nz, ny, nx)) * 1e-3
    return u, g


def golden_hierarchy() -> Hierarchy:
    u, g = golden_setup()
    return Hierarchy(GOLDEN["dtype"], *GOLDEN["size"], GOLDEN["levels"], u, g)
