"""The expectation for relaxed source sweeps (stencil_*_relax): a plain helper
module for tests/test_relax_ref.py (which pins it on hand-computed cells),
tests/test_relax_plan.py and tests/test_gpu_relax.py.

One relaxed sweep with the weight omega is source_ref.sweep -- J = fl(fl(sum6 *
avg) + src) -- and then, on the interior of its planes, in the grid's numpy
dtype, u + w * (J - u) with w = dtype(omega): numpy's subtract, multiply and
add are the IEEE operations, so every cell is fl(u + fl(w * fl(J - u))), four
roundings after the multiply and never an fma.  Sweep i of a job (0-based)
takes omegas[(phase + i) % len(omegas)].  Arrays are dense and ghost-padded
(the oracle's layout); of a source array only the interior is read.
"""
from __future__ import annotations

import math

import numpy as np

from tests import source_ref as sr

K_MAX = sr.K_MAX  # sweeps of the fused relaxed launch, fp32 and fp64
# StripTile (kernels_strip.hip) of the relaxed launches, 8 waves each: (cells per lane V, rows per wave RY);
# the source shapes' but for fp64 K = 4, which takes 4 rows (5 spill)
STRIP = {("fp32", 2): (2, 7), ("fp32", 3): (2, 6), ("fp32", 4): (2, 5),
         ("fp64", 2): (1, 7), ("fp64", 3): (1, 6), ("fp64", 4): (1, 4)}
NP = {"fp32": np.float32, "fp64": np.float64}

problem = sr.problem
update_norm = sr.update_norm
interior_sum = sr.interior_sum


def tile(dtype, k):
    """Output tile (TX, TY) of the K-step relaxed launch (as source_ref.tile)."""
    v, ry = STRIP[dtype, k]
    return 64 * v - 2 * (-(-k // v)) * v, 8 * ry - 2 * k


def sweep(p, u: np.ndarray, src: np.ndarray, omega: float, begin: int = 0, end: int | None = None) -> np.ndarray:
    """One relaxed sweep of planes [begin, end): a new array, `u` elsewhere."""
    end = p.nz if end is None else end
    out = sr.sweep(p, u, src, begin, end)
    sl = np.s_[1 + begin:1 + end, 1:-1, 1:-1]
    w = u.dtype.type(omega)
    with np.errstate(all="ignore"):
        d = out[sl] - u[sl]
        wd = w * d
        out[sl] = u[sl] + wd
    return out


def weight(omegas, i: int, phase: int = 0) -> float:
    return omegas[(phase + i) % len(omegas)]


def sweeps(p, u: np.ndarray, src: np.ndarray, steps: int, omegas, phase: int = 0) -> np.ndarray:
    """`steps` relaxed sweeps of the whole grid, sweep i with omegas[(phase + i) % len]."""
    for i in range(steps):
        u = sweep(p, u, src, weight(omegas, i, phase))
    return u


def sweepk(p, u: np.ndarray, src: np.ndarray, begin: int, end: int, omegas) -> np.ndarray:
    """What a relaxed launch of len(omegas) sweeps over [begin, end) stores: the
    sweeps of the whole grid, taken on planes [begin, end); `u` elsewhere."""
    full = sweeps(p, u, src, len(omegas), omegas)
    out = u.copy()
    out[1 + begin:1 + end, 1:-1, 1:-1] = full[1 + begin:1 + end, 1:-1, 1:-1]
    return out


def until(p, u: np.ndarray, src: np.ndarray, tol: float, cap: int, every: int, omegas, phase: int = 0):
    """stencil_iterate_until_relax's stopping rule (max norm): blocks of
    min(every, cap - done) sweeps, the update checked after each; the schedule
    index runs on across blocks.  Returns (final grid, sweeps done, converged,
    last norm)."""
    done, last = 0, float("inf")
    while done < cap:
        block = min(every, cap - done)
        for i in range(block):
            old, u = u, sweep(p, u, src, weight(omegas, done + i, phase))
        done += block
        last = update_norm(u, old)
        if last <= tol:
            return u, done, True, last
        if last != last:
            break
    return u, done, False, last


def spectral_radius(nx: int, ny: int, nz: int) -> float:
    """Jacobi's spectral radius on the Dirichlet 7-point problem."""
    return (math.cos(math.pi / float(nx + 1)) + math.cos(math.pi / float(ny + 1)) + math.cos(math.pi / float(nz + 1))) / 3.0


def chebyshev_order(period: int) -> list:
    """The Lebedev-Finogenov order: perm_1 = [0]; perm_2m is perm_m with every
    entry p replaced by the pair (p, 2m - 1 - p)."""
    if period < 1 or period > 64 or period & (period - 1):
        raise ValueError(f"the period must be a power of two in 1..64 (got {period})")
    perm, m = [0], 1
    while m < period:
        perm = [q for p_ in perm for q in (p_, 2 * m - 1 - p_)]
        m *= 2
    return perm


def chebyshev_weights(nx: int, ny: int, nz: int, period: int, ascending: bool = False) -> list:
    """stencil_chebyshev_weights in pure Python (ascending: the same weights in
    ascending j, the order that is NOT returned)."""
    rho = spectral_radius(nx, ny, nz)
    order = list(range(period)) if ascending else chebyshev_order(period)
    if ascending:
        chebyshev_order(period)  # the same argument check
    return [1.0 / (1.0 - rho * math.cos(math.pi * float(2 * j + 1) / float(2 * period))) for j in order]
