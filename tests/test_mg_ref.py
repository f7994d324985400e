"""tests/mg_ref.py -- the numpy statement of the multigrid definitions
(include/stencil_hip.h "Geometric multigrid") -- pinned on hand-computed cells,
on the properties the operators must have, on the convergence the definition
promises and on tests/golden/mg_known_answers.json.  CPU only."""
import json
import os

import numpy as np
import pytest

from tests import mg_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mg_known_answers.json")
NP = mr.NP


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_residual_and_one_coarse_cell_term_by_term(dtype):
    """A 3 x 3 x 3 fine grid has ONE coarse cell: every residual and then every
    partial sum of the restriction written out in scalar arithmetic."""
    T = NP[dtype]
    rng = np.random.default_rng(11)
    u = rng.standard_normal((5, 5, 5)).astype(T)
    g = np.full((5, 5, 5), np.nan, dtype=T)
    g[1:-1, 1:-1, 1:-1] = rng.standard_normal((3, 3, 3)).astype(T)
    p = mr.problem(dtype, 3, 3, 3)
    avg = T(1) / T(6)
    r = np.zeros((3, 3, 3), dtype=T)
    for z in range(3):
        for y in range(3):
            for x in range(3):
                c = (z + 1, y + 1, x + 1)
                s = T(0)
                for d in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)):
                    s = T(s + u[c[0] + d[0], c[1] + d[1], c[2] + d[2]])
                j = T(T(s * avg) + g[c])
                r[z, y, x] = T(j - u[c])
    got = mr.residual(p, u, g)
    assert np.array_equal(bits(got), bits(r))

    def a(lo, mid, hi):
        return T(T(lo + hi) + T(mid + mid))

    ax = [[a(r[z, y, 0], r[z, y, 1], r[z, y, 2]) for y in range(3)] for z in range(3)]   # along x
    ay = [a(ax[z][0], ax[z][1], ax[z][2]) for z in range(3)]                             # then y
    want = T(T(0.0625) * a(ay[0], ay[1], ay[2]))                                         # then z, then the scale
    gc = mr.restrict_residual(p, u, g)
    assert gc.shape == (1, 1, 1) and gc.dtype == T
    assert bits(gc)[0, 0, 0] == bits(np.array([want]))[0]


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_one_prolonged_cell_of_each_parity(dtype):
    """Fine cells (z, y, x) in {2, 3}^3 of a 5^3 fine grid over a 2^3 coarse
    one: all eight parities, each written out from e's cells."""
    T = NP[dtype]
    e = np.random.default_rng(12).standard_normal((4, 4, 4)).astype(T)  # ghost-padded 2 x 2 x 2, own ghost values
    got = mr.prolong(e)
    assert got.shape == (5, 5, 5)
    half = T(0.5)

    def along(i):
        """(padded coarse indices, is a copy) of fine index i"""
        return ((i - 1) // 2 + 1,) if i % 2 else (i // 2, i // 2 + 1)

    seen = set()
    for z in (2, 3):
        for y in (2, 3):
            for x in (2, 3):
                zs, ys, xs = along(z), along(y), along(x)
                ex = {(k, j): (e[k, j, xs[0]] if len(xs) == 1 else T(half * T(e[k, j, xs[0]] + e[k, j, xs[1]])))
                      for k in zs for j in ys}
                ey = {k: (ex[k, ys[0]] if len(ys) == 1 else T(half * T(ex[k, ys[0]] + ex[k, ys[1]]))) for k in zs}
                want = ey[zs[0]] if len(zs) == 1 else T(half * T(ey[zs[0]] + ey[zs[1]]))
                assert bits(got)[z, y, x] == bits(np.array([want]))[0], (z, y, x)
                seen.add((z % 2, y % 2, x % 2))
    assert len(seen) == 8
    # the all-odd cell is a copy; the all-even corner cell reads the ghost ring's corner
    assert bits(got)[3, 3, 3] == bits(e)[2, 2, 2]
    corner = mr.prolong(np.where(np.arange(64).reshape(4, 4, 4) == 0, T(8), T(0)).astype(T))
    assert corner[0, 0, 0] == T(1) and np.count_nonzero(corner) == 1


def test_odd_index_is_a_copy_not_an_average():
    """0.5 * (e + e) overflows for huge e; the definition copies."""
    for T in (np.float32, np.float64):
        e = np.zeros((3, 3, 3), dtype=T)
        e[1, 1, 1] = np.finfo(T).max
        got = mr.prolong(e)
        assert got.shape == (3, 3, 3) and got[1, 1, 1] == np.finfo(T).max
        with np.errstate(all="ignore"):
            assert np.isinf(T(0.5) * (e[1, 1, 1] + e[1, 1, 1]))


def test_bits_depend_on_the_order_and_on_fma():
    """The bitwise GPU tests show something only if other evaluation orders
    give other bits: count the fp32 cells that differ when the axes are taken
    z, y, x instead of x, y, z, and when J is one fma instead of two roundings."""
    T = np.float32
    rng = np.random.default_rng(13)
    nx, ny, nz = 31, 15, 7
    p = mr.problem("fp32", nx, ny, nz)
    u = rng.standard_normal((nz + 2, ny + 2, nx + 2)).astype(T)
    g = rng.standard_normal((nz + 2, ny + 2, nx + 2)).astype(T)
    r = mr.residual(p, u, g)
    n_restrict = int((bits(mr.restrict(r)) != bits(mr.restrict(r, order=(0, 1, 2)))).sum())
    e = rng.standard_normal((5, 9, 17)).astype(T)
    n_prolong = int((bits(mr.prolong(e)) != bits(mr.prolong(e, order=(0, 1, 2)))).sum())
    # J with the multiply and the add as one rounding (the product of two floats is exact in double)
    s = np.zeros((nz, ny, nx), dtype=T)
    for sl in ((slice(1, -1), slice(1, -1), slice(0, -2)), (slice(1, -1), slice(1, -1), slice(2, None)),
               (slice(1, -1), slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None), slice(1, -1)),
               (slice(0, -2), slice(1, -1), slice(1, -1)), (slice(2, None), slice(1, -1), slice(1, -1))):
        s = s + u[sl]
    inner = (slice(1, -1),) * 3
    two = (s * (T(1) / T(6)) + g[inner]) - u[inner]
    assert np.array_equal(bits(two), bits(r))  # the slicing above is the oracle's sum
    fused = (s.astype(np.float64) * np.float64(T(1) / T(6)) + g[inner].astype(np.float64)).astype(T) - u[inner]
    n_fma = int((bits(fused) != bits(r)).sum())
    assert n_restrict > 0 and n_prolong > 0 and n_fma > 0, (n_restrict, n_prolong, n_fma)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_constant_restricts_to_four_times_and_linear_prolongs_to_itself(dtype):
    T = NP[dtype]
    c = T(0.3)
    gc = mr.restrict(np.full((7, 5, 9), c, dtype=T))
    assert gc.shape == (3, 2, 4) and (gc == T(4) * c).all()   # 64 c / 16: powers of two, exact
    # a field linear in x, y, z with dyadic coefficients: every mean is exact
    mz, my, mx = 3, 2, 4
    Z, Y, X = np.meshgrid(np.arange(-1, mz + 1), np.arange(-1, my + 1), np.arange(-1, mx + 1), indexing="ij")
    e = (2.0 * X + 4.0 * Y - 6.0 * Z + 1.0).astype(T)                 # coarse cell X sits at fine x = 2X + 1
    z, y, x = np.meshgrid(np.arange(2 * mz + 1), np.arange(2 * my + 1), np.arange(2 * mx + 1), indexing="ij")
    want = ((x - 1.0) + 2.0 * (y - 1.0) - 3.0 * (z - 1.0) + 1.0).astype(T)
    assert np.array_equal(mr.prolong(e), want)


def test_prolong_add_range_and_ghosts():
    rng = np.random.default_rng(14)
    u = rng.standard_normal((9, 7, 5))
    e = rng.standard_normal((5, 4, 3))
    full = mr.prolong_add(u, e)
    part = mr.prolong_add(u, e, 2, 5)
    assert np.array_equal(part[3:6, 1:-1, 1:-1], full[3:6, 1:-1, 1:-1])
    mask = np.ones(u.shape, dtype=bool)
    mask[3:6, 1:-1, 1:-1] = False
    assert np.array_equal(part[mask], u[mask])


def test_residual_norms_nan_rule():
    p = mr.problem("fp64", 5, 3, 3)
    rng = np.random.default_rng(15)
    u, g = rng.standard_normal((5, 5, 7)), rng.standard_normal((5, 5, 7))
    mx, sq = mr.residual_norms(p, u, g)
    r = mr.residual(p, u, g)
    assert np.array_equal(mx, np.abs(r).max(axis=(1, 2))) and np.allclose(sq, (r * r).sum(axis=(1, 2)), rtol=1e-14)
    g[2, 2, 3] = np.nan
    mx, sq = mr.residual_norms(p, u, g)
    assert np.isnan(mx[1]) and np.isnan(sq[1]) and not np.isnan(mx[[0, 2]]).any()
    assert np.isnan(mr.residual_norm(p, u, g))


def test_levels():
    assert mr.max_levels(15, 15, 15) == 4 and mr.max_levels(31, 15, 7) == 3 and mr.max_levels(31, 31, 31) == 5
    assert mr.max_levels(8, 9, 9) == 1 and mr.max_levels(7, 5, 3) == 2
    assert mr.coarse_size(7, 5, 3) == (3, 2, 1)


def test_convergence_and_golden():
    """31^3 fp64, 4 levels, V(2,2), omega = 6/7, 8 coarse sweeps: the max
    residual falls by better than 0.35 in each of cycles 1..6 (the prototype of
    the definition gave 0.249-0.266; the number judges the definition), and the
    residuals are the golden file's."""
    g = mr.GOLDEN
    h = mr.golden_hierarchy()
    assert len(h.p) == 4 and (h.p[-1].nx, h.p[-1].ny, h.p[-1].nz) == (3, 3, 3)
    start = mr.residual_norm(h.p[0], h.u[0], h.g[0])
    done, conv, last, history = mr.solve(h, 0.0, g["cycles"], 1, g["pre"], g["post"], g["coarse_sweeps"], g["omegas"])
    assert (done, conv) == (6, False) and last == history[-1]
    ratios = [b / a for a, b in zip([start] + history[:-1], history)]
    print("max-residual ratios per cycle:", ratios)
    assert all(0.0 < q < 0.35 for q in ratios), ratios
    gold = json.load(open(GOLDEN))
    assert gold["setup"]["size"] == list(g["size"]) and gold["setup"]["seed"] == g["seed"]
    assert gold["residual_start"] == start and float.fromhex(gold["residual_start_hex"]) == start
    assert gold["residual_after_cycle"] == history
    assert [float.fromhex(v) for v in gold["residual_after_cycle_hex"]] == history


def test_solve_stopping_rule():
    g = mr.GOLDEN
    gold = json.load(open(GOLDEN))["residual_after_cycle"]
    args = (g["pre"], g["post"], g["coarse_sweeps"], g["omegas"])
    assert mr.solve(mr.golden_hierarchy(), 1e-3, 0, 1, *args) == (0, False, float("inf"), [])
    done, conv, last, hist = mr.solve(mr.golden_hierarchy(), 1e-3, 10, 1, *args)
    assert (done, conv, last) == (4, True, gold[3]) and hist == gold[:4]
    done, conv, last, hist = mr.solve(mr.golden_hierarchy(), 1e-3, 10, 3, *args)   # checks after 3 and 6
    assert (done, conv, last) == (6, True, gold[5]) and hist == [gold[2], gold[5]]
    done, conv, last, hist = mr.solve(mr.golden_hierarchy(), 1e-30, 5, 2, *args)   # never reached: 2, 4, 5
    assert (done, conv, last) == (5, False, gold[4]) and hist == [gold[1], gold[3], gold[4]]
