"""The expectation for sweeps with a source term (stencil_*_source): a plain
helper module for tests/test_source_ref.py (which pins it on hand-computed
cases), tests/test_source_plan.py and tests/test_gpu_source.py.

One source sweep is the oracle's sweep into a copy, then `interior +=
src_interior` in the grid's numpy dtype: numpy's add is the IEEE add, so every
cell is fl(fl(sum6 * avg) + src) -- two roundings, never one fma.  K sweeps
and jobs are that in a loop.  Arrays are dense and ghost-padded (the oracle's
layout); of a source array only the interior is read.
"""
from __future__ import annotations

import numpy as np

from oracle import binding as ob

K_MAX = 4  # sweeps of the fused source launch (STENCIL_SOURCE_MAX_STEPS), fp32 and fp64
# StripTile (kernels_strip.hip) of the source launches, 8 waves each: (cells per lane V, rows per wave RY)
STRIP = {("fp32", 2): (2, 7), ("fp32", 3): (2, 6), ("fp32", 4): (2, 5),
         ("fp64", 2): (1, 7), ("fp64", 3): (1, 6), ("fp64", 4): (1, 5)}


def tile(dtype, k):
    """Output tile (TX, TY) of the K-step source launch: a region of 64 V x 8 RY
    cells less a ring of ceil(K / V) lane vectors per x side and K rows per y side."""
    v, ry = STRIP[dtype, k]
    return 64 * v - 2 * (-(-k // v)) * v, 8 * ry - 2 * k


def problem(dtype, nx, ny, nz):
    return ob.problem(3, dtype, "star", 1, "naive", nx, ny, nz)


def sweep(p, u: np.ndarray, src: np.ndarray, begin: int = 0, end: int | None = None) -> np.ndarray:
    """One source sweep of planes [begin, end): a new array, `u` elsewhere."""
    end = p.nz if end is None else end
    out = u.copy()
    ob.sweep(p, u, out, begin, end, 1)
    with np.errstate(all="ignore"):
        out[1 + begin:1 + end, 1:-1, 1:-1] += src[1 + begin:1 + end, 1:-1, 1:-1]
    return out


def sweeps(p, u: np.ndarray, src: np.ndarray, steps: int) -> np.ndarray:
    """`steps` source sweeps of the whole grid."""
    for _ in range(steps):
        u = sweep(p, u, src)
    return u


def sweepk(p, u: np.ndarray, src: np.ndarray, begin: int, end: int, steps: int) -> np.ndarray:
    """What a K-step source launch over [begin, end) stores: `steps` sweeps of
    the whole grid, taken on planes [begin, end) (a launch reads `u` as far
    beyond its range as it needs); `u` elsewhere."""
    full = sweeps(p, u, src, steps)
    out = u.copy()
    out[1 + begin:1 + end, 1:-1, 1:-1] = full[1 + begin:1 + end, 1:-1, 1:-1]
    return out


def update_norm(cur: np.ndarray, old: np.ndarray, norm: str = "max") -> float:
    """stencil_diff_norms' scalar norm of two dense grids' interiors."""
    with np.errstate(all="ignore"):
        d = cur[1:-1, 1:-1, 1:-1].astype(np.float64) - old[1:-1, 1:-1, 1:-1].astype(np.float64)
        if np.isnan(d).any():
            return float("nan")
        if norm == "max":
            return float(np.abs(d).max()) if d.size else 0.0
        total = 0.0
        for plane in d:  # per-plane sums are compared elsewhere; the max norm is what these tests use
            total += float((plane * plane).sum())
        return float(np.sqrt(total))


def until(p, u: np.ndarray, src: np.ndarray, tol: float, cap: int, every: int):
    """stencil_iterate_until_source's stopping rule (max norm): blocks of
    min(every, cap - done) sweeps, the update checked after each.  Returns
    (final grid, sweeps done, converged, last norm)."""
    done, last = 0, float("inf")
    while done < cap:
        block = min(every, cap - done)
        for _ in range(block):
            old, u = u, sweep(p, u, src)
        done += block
        last = update_norm(u, old)
        if last <= tol:
            return u, done, True, last
        if last != last:
            break
    return u, done, False, last


def interior_sum(u: np.ndarray) -> float:
    """The interior added up in double in ascending z, y, x order (the CLI's
    "interior sum" line)."""
    total = 0.0
    for v in u[1:-1, 1:-1, 1:-1].astype(np.float64).ravel():
        total += float(v)
    return total
