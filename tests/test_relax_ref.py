"""tests/relax_ref.py pinned: hand-computed cells (one where the fma form gives
other bits), the fraction of fp32 cells where the fma form differs, the
Chebyshev helper in C against the pure-Python one, and the convergence
conditions with their recorded counts (tests/golden/relax_known_answers.json)."""
import ctypes
import functools
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import binding as ob
from stencil_amd import _lib
from tests import relax_ref as rr
from tests import source_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relax_known_answers.json")


def one_cell(dtype, centre, nbrs, g):
    """A 1 x 1 x 1 grid: the centre cell, its six ghost neighbours (x-, x+, y-, y+, z-, z+), the source."""
    p = rr.problem(dtype, 1, 1, 1)
    u = np.zeros((3, 3, 3), dtype=rr.NP[dtype])
    u[1, 1, 1] = centre
    u[1, 1, 0], u[1, 1, 2], u[1, 0, 1], u[1, 2, 1], u[0, 1, 1], u[2, 1, 1] = nbrs
    src = np.full_like(u, np.nan)
    src[1, 1, 1] = g
    return p, u, src


def test_hand_computed_exact_cell():
    # sum6 = 6, J = fl(6 * fl(1/6)) + 0.5 = 1.5 (6 * fl(1/6) rounds to 1 in both types); d = 1.5 - 0.25 = 1.25;
    # w = 0.5: 0.25 + 0.625 = 0.875 -- every step exact
    for dt in ("fp32", "fp64"):
        p, u, src = one_cell(dt, 0.25, (1, 1, 1, 1, 1, 1), 0.5)
        out = rr.sweep(p, u, src, 0.5)
        assert out[1, 1, 1] == 0.875 and out.dtype == u.dtype
        ghosts = out.copy()
        ghosts[1, 1, 1] = u[1, 1, 1]
        assert np.array_equal(ghosts, u)  # ghost cells keep their value


def fl32(x):
    return float(np.float32(x))


def test_hand_computed_cell_where_fma_differs():
    """fp32, exact rational arithmetic rounded by hand at each of the four steps."""
    t = np.float32
    centre, g, omega = t(1) / t(3), t(0.1), 1.25
    nbrs = tuple(t(v) for v in (0.7, 0.2, 0.9, 0.4, 0.6, 0.3))
    p, u, src = one_cell("fp32", centre, nbrs, g)
    s = t(0)
    for v in nbrs:
        s = t(s + v)
    avg = t(1) / t(6)
    j = t(t(s * avg) + g)
    d = t(Fraction(float(j)) - Fraction(float(centre)))        # rounded once
    w = t(omega)
    wd = t(Fraction(float(w)) * Fraction(float(d)))            # rounded once
    want = t(Fraction(float(centre)) + Fraction(float(wd)))    # rounded once
    got = rr.sweep(p, u, src, omega)[1, 1, 1]
    assert got.tobytes() == want.tobytes()
    fma = t(Fraction(float(w)) * Fraction(float(d)) + Fraction(float(centre)))  # one rounding
    assert fma.tobytes() != want.tobytes(), "choose another cell: the fma form gives the same bits here"


def test_fma_form_differs_in_some_fp32_cells():
    p = rr.problem("fp32", 24, 20, 12)
    u = ob.init(p, "random", 11)
    src = np.zeros_like(u)
    src[1:-1, 1:-1, 1:-1] = np.random.default_rng(12).uniform(-1, 1, (12, 20, 24)).astype(np.float32)
    omega = 0.8
    want = rr.sweep(p, u, src, omega)[1:-1, 1:-1, 1:-1]
    j = sr.sweep(p, u, src)[1:-1, 1:-1, 1:-1]
    c = u[1:-1, 1:-1, 1:-1]
    d = (j - c).astype(np.float64)
    fma = (np.float64(np.float32(omega)) * d + c.astype(np.float64)).astype(np.float32)  # exact in double, one rounding
    frac = float((fma.view(np.uint32) != want.view(np.uint32)).mean())
    print(f"fma form differs in {frac:.4f} of the fp32 cells")
    assert frac > 0.0


def test_omega_one_is_not_the_source_sweep():
    p = rr.problem("fp32", 24, 20, 12)
    u = ob.init(p, "random", 11)
    src = np.zeros_like(u)
    a, b = rr.sweep(p, u, src, 1.0), sr.sweep(p, u, src)
    assert not np.array_equal(a, b) and np.allclose(a, b, rtol=1e-6, atol=1e-7)


def test_schedule_indexing():
    p = rr.problem("fp64", 7, 5, 6)
    u = ob.init(p, "random", 3)
    src = np.zeros_like(u)
    w = [0.8, 1.7, 0.6]
    by_hand = u
    for i in range(7):
        by_hand = rr.sweep(p, by_hand, src, w[(2 + i) % 3])
    assert np.array_equal(rr.sweeps(p, u, src, 7, w, phase=2), by_hand)
    # continuing with phase equals one call
    first = rr.sweeps(p, u, src, 4, w, phase=2)
    assert np.array_equal(rr.sweeps(p, first, src, 3, w, phase=6), by_hand)
    got = rr.sweepk(p, u, src, 2, 4, w)
    full = rr.sweeps(p, u, src, 3, w)
    assert np.array_equal(got[3:5, 1:-1, 1:-1], full[3:5, 1:-1, 1:-1]) and np.array_equal(got[1:3], u[1:3])


def test_tile_table():
    assert rr.tile("fp64", 4) == (56, 24) and rr.tile("fp32", 4) == (120, 32)
    assert rr.tile("fp64", 3) == (58, 42) and rr.tile("fp32", 3) == (120, 42)
    assert rr.tile("fp64", 2) == (60, 52) and rr.tile("fp32", 2) == (124, 52)
    for key, (v, ry) in rr.STRIP.items():
        assert v == sr.STRIP[key][0] and ry <= sr.STRIP[key][1]


# ------------------------------------------------------ the Chebyshev helper
def c_weights(nx, ny, nz, period):
    lib = _lib.load(debug=False)
    prob = _lib.make_problem(dims=3, dtype=_lib.F64, nx=nx, ny=ny, nz=nz)
    w, rho = (ctypes.c_double * period)(), ctypes.c_double(0.0)
    assert lib.stencil_chebyshev_weights(ctypes.byref(prob), period, w, ctypes.byref(rho)) == 0
    return list(w), rho.value


def test_order():
    assert rr.chebyshev_order(1) == [0] and rr.chebyshev_order(2) == [0, 1] and rr.chebyshev_order(4) == [0, 3, 1, 2]
    assert rr.chebyshev_order(8) == [0, 7, 3, 4, 1, 6, 2, 5]
    for period in (16, 64):
        assert sorted(rr.chebyshev_order(period)) == list(range(period))
    for bad in (0, 3, 12, 128):
        with pytest.raises(ValueError):
            rr.chebyshev_order(bad)


@pytest.mark.parametrize("size", [(15, 15, 15), (31, 31, 31), (70, 37, 23), (1, 2, 3), (512, 512, 512)])
@pytest.mark.parametrize("period", [1, 2, 4, 16, 64])
def test_c_helper_is_the_python_one(size, period):
    got, rho = c_weights(*size, period)
    want = rr.chebyshev_weights(*size, period)
    assert [x.hex() for x in got] == [x.hex() for x in want]
    assert rho.hex() == rr.spectral_radius(*size).hex()
    if period == 4:
        asc = rr.chebyshev_weights(*size, 4, ascending=True)
        assert got == [asc[0], asc[3], asc[1], asc[2]]
    assert all(0.5 < x <= 1.0 / (1.0 - rho) for x in got)


def test_period_one_is_plain_jacobi_weight():
    got, _ = c_weights(15, 15, 15, 1)
    assert got == [1.0 / (1.0 - rr.spectral_radius(15, 15, 15) * math.cos(math.pi * 1.0 / 2.0))]
    assert abs(got[0] - 1.0) < 1e-15


# ------------------------------------------------------------- convergence
@functools.lru_cache(maxsize=None)
def run_until(dtype, n, tol, cap, every, schedule):
    p = rr.problem(dtype, n, n, n)
    u = ob.init(p)
    omegas = {"omega1": [1.0], "cheby8": rr.chebyshev_weights(n, n, n, 8), "cheby64": rr.chebyshev_weights(n, n, n, 64),
              "ascending64": rr.chebyshev_weights(n, n, n, 64, ascending=True)}[schedule]
    _, done, conv, last = rr.until(p, u, np.zeros_like(u), tol, cap, every, omegas)
    return done, conv, last


def known():
    with open(GOLDEN) as f:
        return json.load(f)


def as_recorded(result):
    done, conv, last = result
    return [done, conv, "nan" if last != last else last]


@pytest.mark.parametrize("dtype,tol", [("fp64", 1e-8), ("fp32", 1e-5)])
def test_chebyshev_needs_a_third_of_the_sweeps(dtype, tol):
    k = known()[f"15_{dtype}"]
    assert (k["tol"], k["every"]) == (tol, 16)
    plain = run_until(dtype, 15, tol, 4000, 16, "omega1")
    cheb = run_until(dtype, 15, tol, 4000, 16, "cheby8")
    print(f"15^3 {dtype} tol {tol}: omega = 1 {plain}, P = 8 {cheb}")
    assert plain[1] and cheb[1]
    assert 3 * cheb[0] <= plain[0]
    assert as_recorded(plain) == k["omega1"] and as_recorded(cheb) == k["cheby8"]


def test_schedule_order_matters():
    k = known()["31_fp32"]
    assert (k["tol"], k["every"]) == (1e-5, 64)
    good = run_until("fp32", 31, 1e-5, 640, 64, "cheby64")
    bad = run_until("fp32", 31, 1e-5, 640, 64, "ascending64")
    print(f"31^3 fp32: helper's order {good}, ascending {bad}")
    assert good[1] and good[0] <= 256
    assert not bad[1] and bad[0] <= 640 and (bad[2] != bad[2] or bad[2] > 1e-3)
    assert as_recorded(good) == k["cheby64"] and as_recorded(bad) == k["ascending64"]
