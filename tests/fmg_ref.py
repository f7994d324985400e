"""The expectation for the full multigrid calls (stencil_restrict_source,
stencil_inject_ghosts, stencil_prolong_cubic, stencil_mg_fmg):
include/stencil_hip.h "Full multigrid" stated in numpy, on top of
tests/mg_ref.py.  A plain helper module for tests/test_fmg_ref.py (which pins
it on hand-computed cells), tests/test_gpu_fmg.py and
tests/golden/make_fmg_golden.py.

Arrays are dense and ghost-padded unless a name says `interior`; padded index
P is coarse (or fine) index P - 1.  numpy's add and multiply are the IEEE
operations in the array's dtype, so every value is the stated sequence of
roundings:
  coarse source   mg_ref.restrict of g's interior
  injection       strided slices: coarse padded P is fine padded 2 P
  prolongation    along x, then y, then z; odd indices are copies, even ones
                  0.0625 * ((w0 p0 + w1 p1) + (w2 p2 + w3 p3)), every product
                  and sum rounded; 0.5 * (lo + hi) where the coarse extent is 1
  the pass        plain loops over mg_ref.vcycle and relax_ref.sweeps
"""
from __future__ import annotations

import numpy as np

from tests import mg_ref as mr
from tests import relax_ref as rr

NP = mr.NP
W_FIRST, W_LAST, W_MID = (5, 15, -5, 1), (1, -5, 15, 5), (-1, 9, 9, -1)


def coarse_source(g: np.ndarray) -> np.ndarray:
    """g_c = fl(0.0625 * A_z(A_y(A_x(g)))) of a ghost-padded source: the coarse
    interior, (mz, my, mx).  g's ghost cells are not read."""
    return mr.restrict(g[1:-1, 1:-1, 1:-1])


def shell_mask(shape) -> np.ndarray:
    """True at the ghost shell of a padded shape: the box minus its interior."""
    m = np.ones(shape, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = False
    return m


def inject_ghosts(uf: np.ndarray, uc: np.ndarray) -> np.ndarray:
    """uc with its ghost shell (edges and corners included) taken from the fine
    ghost-shell cells it sits on: a new array."""
    picked = uf[::2, ::2, ::2]
    assert picked.shape == uc.shape, (uf.shape, uc.shape)
    out = uc.copy()
    mask = shell_mask(uc.shape)
    out[mask] = picked[mask]
    return out


def window(k: int, m: int):
    """(first padded node, weights) of even fine index 2 k on a coarse line of m >= 2 interior cells."""
    if k == 0:
        return 0, W_FIRST       # c(-1 .. 2)
    if k == m:
        return m - 2, W_LAST    # c(m-3 .. m)
    return k - 1, W_MID         # c(k-2 .. k+1)


def weighted(p0, p1, p2, p3, w, fma: bool = False):
    """fl(0.0625 * fl(fl(fl(w0 p0) + fl(w1 p1)) + fl(fl(w2 p2) + fl(w3 p3)))); `fma`: the sum contracted as a
    compiler would (each pair w_a p_a + fl(w_b p_b) in one rounding) -- NOT the definition, for the census."""
    T = p0.dtype.type
    with np.errstate(all="ignore"):
        if fma:
            def pair(wa, pa, wb, pb):
                exact = pa.astype(np.float64) * np.float64(wa) + (T(wb) * pb).astype(np.float64)
                return exact.astype(T)  # fp32 only: the product and the sum are exact in double
            return T(0.0625) * (pair(w[0], p0, w[1], p1) + pair(w[2], p2, w[3], p3))
        return T(0.0625) * ((T(w[0]) * p0 + T(w[1]) * p1) + (T(w[2]) * p2 + T(w[3]) * p3))


def interp_cubic(e: np.ndarray, axis: int, fma: bool = False) -> np.ndarray:
    """The 1-D cubic interpolation along `axis`: m + 2 padded coarse cells ->
    2 m + 1 fine cells."""
    m = e.shape[axis] - 2
    assert m >= 1
    e = np.moveaxis(e, axis, -1)
    out = np.empty(e.shape[:-1] + (2 * m + 1,), dtype=e.dtype)
    out[..., 1::2] = e[..., 1:m + 1]
    for k in range(m + 1):
        if m == 1:
            with np.errstate(all="ignore"):
                out[..., 2 * k] = e.dtype.type(0.5) * (e[..., k] + e[..., k + 1])
        else:
            s, w = window(k, m)
            out[..., 2 * k] = weighted(e[..., s], e[..., s + 1], e[..., s + 2], e[..., s + 3], w, fma)
    return np.moveaxis(out, -1, axis)


def prolong_cubic(e: np.ndarray, order=(2, 1, 0), fma: bool = False) -> np.ndarray:
    """The cubic prolongation of a ghost-padded coarse array: the fine
    interior, (nz, ny, nx) (`order`: the axes in turn; the definition's is
    x, y, z = 2, 1, 0)."""
    a = e
    for axis in order:
        a = interp_cubic(a, axis, fma)
    return a


def prolong_cubic_set(u: np.ndarray, e: np.ndarray, begin: int = 0, end: int | None = None) -> np.ndarray:
    """u with the interior cells of fine planes [begin, end) set to the
    prolongation of e: a new array."""
    nz = u.shape[0] - 2
    end = nz if end is None else end
    out = u.copy()
    out[1 + begin:1 + end, 1:-1, 1:-1] = prolong_cubic(e)[begin:end]
    return out


def fmg(h: mr.Hierarchy, cycles: int, pre: int, post: int, coarse_sweeps: int, omegas) -> None:
    """stencil_mg_fmg, in place on the hierarchy (h.u[0]'s ghost shell is the
    Dirichlet data, its interior is ignored)."""
    levels = len(h.p)
    for lv in range(levels - 1):
        h.g[lv + 1] = np.zeros_like(h.g[lv + 1])
        h.g[lv + 1][1:-1, 1:-1, 1:-1] = coarse_source(h.g[lv])
        h.u[lv + 1] = inject_ghosts(h.u[lv], np.zeros_like(h.u[lv + 1]))
    last = levels - 1
    if levels == 1:
        h.u[0] = h.u[0].copy()
        h.u[0][1:-1, 1:-1, 1:-1] = 0
    h.u[last] = rr.sweeps(h.p[last], h.u[last], h.g[last], coarse_sweeps, omegas)
    for lv in range(levels - 2, -1, -1):
        h.u[lv] = prolong_cubic_set(h.u[lv], h.u[lv + 1])
        h.u[lv + 1] = np.zeros_like(h.u[lv + 1])
        for _ in range(cycles):
            mr.vcycle(h, pre, post, coarse_sweeps, omegas, lv)


# The problem of DESIGN.md 5.10's table: -Laplace u = f on the unit cube, u* = sin(pi x) cos(pi y) e^z, Dirichlet
# data from u*, fp64, V(2,2), omega = 6/7, 8 coarse sweeps, every level the extents give.
GOLDEN = {"dtype": "fp64", "sizes": (15, 31), "cycles": 2, "pre": 2, "post": 2, "coarse_sweeps": 8,
          "omegas": (6.0 / 7.0,)}


def model_problem(n: int):
    """(u* ghost-padded, g = h^2 f / 6 ghost-padded with zero ghosts) on an n^3 grid, h = 1 / (n + 1), fp64."""
    h = 1.0 / (n + 1)
    t = np.arange(n + 2) * h
    z, y, x = np.meshgrid(t, t, t, indexing="ij")
    exact = np.sin(np.pi * x) * np.cos(np.pi * y) * np.exp(z)
    f = (2.0 * np.pi ** 2 - 1.0) * exact  # -Laplace u*
    g = np.zeros_like(exact)
    g[1:-1, 1:-1, 1:-1] = (h * h / 6.0) * f[1:-1, 1:-1, 1:-1]
    return exact, g


def model_hierarchy(n: int, interior=None) -> mr.Hierarchy:
    """The model problem's hierarchy: ghost shell u*, interior zero (or `interior`)."""
    exact, g = model_problem(n)
    u = exact.copy()
    u[1:-1, 1:-1, 1:-1] = 0.0 if interior is None else interior
    return mr.Hierarchy("fp64", n, n, n, 0, u, g)


def discrete_solution(n: int, tol: float = 1e-15, max_cycles: int = 60) -> np.ndarray:
    """u_h: V-cycles from zero until the residual's max norm stalls at rounding level."""
    g = GOLDEN
    h = model_hierarchy(n)
    best = float("inf")
    for _ in range(max_cycles):
        mr.vcycle(h, g["pre"], g["post"], g["coarse_sweeps"], g["omegas"])
        r = mr.residual_norm(h.p[0], h.u[0], h.g[0])
        if r <= tol or r >= best:
            break
        best = r
    return h.u[0]


def max_diff(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.abs(a[1:-1, 1:-1, 1:-1] - b[1:-1, 1:-1, 1:-1]).max())


def trilinear_fmg(h: mr.Hierarchy, cycles: int, pre: int, post: int, coarse_sweeps: int, omegas) -> None:
    """The pass with mg_ref's trilinear prolongation in the cubic one's place (the table's comparison rows)."""
    levels = len(h.p)
    for lv in range(levels - 1):
        h.g[lv + 1] = np.zeros_like(h.g[lv + 1])
        h.g[lv + 1][1:-1, 1:-1, 1:-1] = coarse_source(h.g[lv])
        h.u[lv + 1] = inject_ghosts(h.u[lv], np.zeros_like(h.u[lv + 1]))
    last = levels - 1
    h.u[last] = rr.sweeps(h.p[last], h.u[last], h.g[last], coarse_sweeps, omegas)
    for lv in range(levels - 2, -1, -1):
        start = h.u[lv].copy()
        start[1:-1, 1:-1, 1:-1] = 0
        h.u[lv] = mr.prolong_add(start, h.u[lv + 1])
        h.u[lv + 1] = np.zeros_like(h.u[lv + 1])
        for _ in range(cycles):
            mr.vcycle(h, pre, post, coarse_sweeps, omegas, lv)


def cycles_to_reach(n: int, target: float, u_h: np.ndarray, cap: int = 30) -> int:
    """Zero-start V-cycles until max |u - u_h| <= target."""
    g = GOLDEN
    h = model_hierarchy(n)
    for c in range(1, cap + 1):
        mr.vcycle(h, g["pre"], g["post"], g["coarse_sweeps"], g["omegas"])
        if max_diff(h.u[0], u_h) <= target:
            return c
    return cap + 1


def golden_ratios(n: int) -> dict:
    """alg = max |u_FMG - u_h|, disc = max |u_h - u*| and their ratio for the
    cubic and the trilinear pass at 1 and 2 cycles per level."""
    g = GOLDEN
    args = (g["pre"], g["post"], g["coarse_sweeps"], g["omegas"])
    exact, _ = model_problem(n)
    u_h = discrete_solution(n)
    disc = max_diff(u_h, exact)
    out = {"n": n, "disc": disc}
    for name, run in (("cubic", fmg), ("trilinear", trilinear_fmg)):
        for cycles in (1, 2):
            h = model_hierarchy(n)
            run(h, cycles, *args)
            alg = max_diff(h.u[0], u_h)
            out[f"{name}_{cycles}"] = {"alg": alg, "ratio": alg / disc, "zero_start_cycles": cycles_to_reach(n, alg, u_h)}
    return out
