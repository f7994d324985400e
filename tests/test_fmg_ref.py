"""tests/fmg_ref.py -- the numpy statement of the full multigrid definitions
(include/stencil_hip.h "Full multigrid") -- pinned on hand-computed cells, on
the properties the operators must have, on the accuracy the pass promises and
on tests/golden/fmg_known_answers.json.  CPU only."""
import json
import os

import numpy as np
import pytest

from tests import boundary_data as bd
from tests import fmg_ref as fr
from tests import mg_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fmg_known_answers.json")
NP = mr.NP


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return bits(np.asarray(a)).tolist() == bits(np.asarray(b)).tolist()


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_one_prolonged_value_of_each_case_term_by_term(dtype):
    """A 1-D line: m = 1; and on m = 5 the first window (k = 0), the last
    (k = m), a central one and an odd index, each from scalar arithmetic."""
    T = NP[dtype]
    rng = np.random.default_rng(21)
    c = rng.standard_normal(3).astype(T)                   # m = 1: c(-1), c(0), c(1)
    got = fr.interp_cubic(c, 0)
    assert got.shape == (3,)
    assert same(got, [T(T(0.5) * T(c[0] + c[1])), c[1], T(T(0.5) * T(c[1] + c[2]))])

    m = 5
    c = rng.standard_normal(m + 2).astype(T)               # padded: c(X) is c[X + 1]
    got = fr.interp_cubic(c, 0)
    assert got.shape == (2 * m + 1,)

    def node(X):
        return c[X + 1]

    def value(w, X0):
        p = [node(X0 + j) for j in range(4)]
        left = T(T(T(w[0]) * p[0]) + T(T(w[1]) * p[1]))
        right = T(T(T(w[2]) * p[2]) + T(T(w[3]) * p[3]))
        return T(T(0.0625) * T(left + right))

    assert same(got[0], value((5, 15, -5, 1), -1))         # k = 0: c(-1 .. 2)
    assert same(got[2 * m], value((1, -5, 15, 5), m - 3))  # k = m: c(m-3 .. m)
    assert same(got[4], value((-1, 9, 9, -1), 0))          # k = 2: c(0 .. 3)
    assert same(got[2], value((-1, 9, 9, -1), -1))         # k = 1: c(-1 .. 2), the first central window
    assert same(got[2 * m - 2], value((-1, 9, 9, -1), m - 3))
    for i in range(1, 2 * m, 2):                           # odd i: c((i - 1) / 2), a copy
        assert same(got[i], node((i - 1) // 2))
    # m = 2: all three windows are c(-1 .. 2)
    c = rng.standard_normal(4).astype(T)
    got = fr.interp_cubic(c, 0)
    for k, w in ((0, fr.W_FIRST), (1, fr.W_MID), (2, fr.W_LAST)):
        assert fr.window(k, 2) == (0, w)
        assert same(got[2 * k], fr.weighted(c[0:1], c[1:2], c[2:3], c[3:4], w)[0])
    # the copy is exact where the weighted form would overflow
    big = np.full(5, np.finfo(T).max, dtype=T)
    assert (fr.interp_cubic(big, 0)[1::2] == np.finfo(T).max).all()


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_cubic_polynomials_are_reproduced(dtype):
    """A cubic sampled on the padded coarse grid comes back at every fine
    cell.  The bound is derived: along one axis the value is
    0.0625 * ((w0 p0 + w1 p1) + (w2 p2 + w3 p3)); the scale and the products by
    1 and 5 .. 15 add at most one rounding each and the three sums one each, so
    at most 3 roundings lie on any path from a node to the sum -- an absolute
    error <= 3 eps * 0.0625 * sum |w_j| |p_j| <= 3 eps * (26 / 16) * max |p|
    per axis (sum |w| = 26 for the one-sided windows, 20 for the central one).
    Errors of an earlier axis pass through a later one amplified by at most
    sum |w| / 16 = 26 / 16.  With A = 26 / 16 and M = max |samples| the total
    is <= 3 eps M (A + A^2 + A^3) (1 + small).  The coarse samples are rounded
    to T once (eps M each), which passes through the three axes: eps M A^3.  The
    test allows eps M (3.03 (A + A^2 + A^3) + A^3); eps is the unit roundoff."""
    T = NP[dtype]
    eps = np.finfo(T).eps / 2
    mz, my, mx = 4, 2, 7

    def poly(x, y, z):
        return (0.25 * x ** 3 - 0.5 * x * x * y + 0.125 * z ** 3 + 0.75 * y * z * x - 0.375 * y ** 3 + x - 2.0 * z
                + 0.5)

    # coordinates in fine units scaled to [-1, 1]: coarse padded index P sits at fine padded index 2 P
    def axis(m):
        return (np.arange(2 * m + 3) - (m + 1.0)) / (m + 1.0)

    zf, yf, xf = np.meshgrid(axis(mz), axis(my), axis(mx), indexing="ij")
    fine64 = poly(xf, yf, zf)
    e = fine64[::2, ::2, ::2].astype(T)
    got = fr.prolong_cubic(e)
    assert got.shape == (2 * mz + 1, 2 * my + 1, 2 * mx + 1) and got.dtype == T
    big = float(np.abs(fine64).max())
    a = 26.0 / 16.0
    bound = eps * big * (3.03 * (a + a * a + a ** 3) + a ** 3)
    err = float(np.abs(got.astype(np.float64) - fine64[1:-1, 1:-1, 1:-1]).max())
    print(f"{dtype}: cubic reproduction error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # ... and the trilinear prolongation does not reproduce it (the test can tell the two apart)
    assert float(np.abs(mr.prolong(e).astype(np.float64) - fine64[1:-1, 1:-1, 1:-1]).max()) > 1e-3


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_constant_source_restricts_to_four_times(dtype):
    T = NP[dtype]
    c = T(0.3)
    g = np.full((9, 7, 11), np.nan, dtype=T)   # ghost cells are never read
    g[1:-1, 1:-1, 1:-1] = c
    gc = fr.coarse_source(g)
    assert gc.shape == (3, 2, 4) and gc.dtype == T and (gc == T(4) * c).all()
    rng = np.random.default_rng(22)
    g[1:-1, 1:-1, 1:-1] = rng.standard_normal((7, 5, 9)).astype(T)
    assert same(fr.coarse_source(g), mr.restrict(g[1:-1, 1:-1, 1:-1]))


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_injection_on_a_ring_of_distinct_values(dtype):
    T = NP[dtype]
    nx, ny, nz = 7, 5, 3
    mx, my, mz = mr.coarse_size(nx, ny, nz)
    uf = bd.ring_field((nz + 2, ny + 2, nx + 2), 1, 23, T, False)   # a box's ring: edges and corners have values
    shell = uf[fr.shell_mask(uf.shape)]
    assert len(np.unique(shell)) == shell.size
    uc0 = np.random.default_rng(24).standard_normal((mz + 2, my + 2, mx + 2)).astype(T)
    uc = fr.inject_ghosts(uf, uc0)
    assert same(uc[1:-1, 1:-1, 1:-1], uc0[1:-1, 1:-1, 1:-1])        # the interior stays
    for Z in range(-1, mz + 1):
        for Y in range(-1, my + 1):
            for X in range(-1, mx + 1):
                if -1 < Z < mz and -1 < Y < my and -1 < X < mx:
                    continue
                assert same(uc[Z + 1, Y + 1, X + 1], uf[2 * Z + 2, 2 * Y + 2, 2 * X + 2]), (X, Y, Z)
    # every coarse shell cell comes from the FINE shell: coarse ghost -1 sits on fine ghost -1, m on n
    fine_shell = set(bits(shell).tolist())
    assert set(bits(uc[fr.shell_mask(uc.shape)]).tolist()) <= fine_shell


def test_bits_depend_on_the_order_and_on_fma():
    """The bitwise GPU tests show something only if other evaluations give
    other bits: the fp32 cells that differ when the axes are taken z, y, x,
    and when the weighted sum's two pairs are contracted to fmas."""
    T = np.float32
    rng = np.random.default_rng(25)
    e = rng.standard_normal((6, 9, 17)).astype(T)
    want = fr.prolong_cubic(e)
    n_order = int((bits(want) != bits(fr.prolong_cubic(e, order=(0, 1, 2)))).sum())
    n_fma = int((bits(want) != bits(fr.prolong_cubic(e, fma=True))).sum())
    g = rng.standard_normal((9, 17, 33)).astype(T)
    n_restrict = int((bits(mr.restrict(g)) != bits(mr.restrict(g, order=(0, 1, 2)))).sum())
    print("cells that differ: axis order", n_order, "fma", n_fma, "restriction order", n_restrict, "of", want.size)
    assert n_order > 0 and n_fma > 0 and n_restrict > 0


def test_prolong_set_range_and_pass_invariants():
    rng = np.random.default_rng(26)
    u = rng.standard_normal((9, 7, 5))
    e = rng.standard_normal((5, 4, 3))
    full = fr.prolong_cubic_set(u, e)
    part = fr.prolong_cubic_set(u, e, 2, 5)
    assert np.array_equal(part[3:6, 1:-1, 1:-1], full[3:6, 1:-1, 1:-1])
    mask = np.ones(u.shape, dtype=bool)
    mask[3:6, 1:-1, 1:-1] = False
    assert np.array_equal(part[mask], u[mask])
    assert np.array_equal(full[1:-1, 1:-1, 1:-1], fr.prolong_cubic(e))   # a set: u's interior is not read
    # the pass leaves zero ghost cells on every coarse level and ignores the fine interior
    size = (15, 15, 15)
    start = bd.ring_field((17, 17, 17), 1, 27, np.float64, False)
    g = np.zeros_like(start)
    g[1:-1, 1:-1, 1:-1] = rng.standard_normal((15, 15, 15))
    h1 = mr.Hierarchy("fp64", *size, 4, start, g)
    other = start.copy()
    other[1:-1, 1:-1, 1:-1] = np.nan
    h2 = mr.Hierarchy("fp64", *size, 4, other, g)
    for h in (h1, h2):
        fr.fmg(h, 1, 2, 3, 5, (0.8, 1.1))
    for lv in range(4):
        assert same(h1.u[lv], h2.u[lv]) and same(h1.g[lv], h2.g[lv])
        if lv:
            assert not h1.u[lv][fr.shell_mask(h1.u[lv].shape)].any()
    assert same(h1.u[0][fr.shell_mask(start.shape)], start[fr.shell_mask(start.shape)])


def test_fmg_reaches_discretization_accuracy():
    """The model problem at 15^3 and 31^3, fp64, two cycles per level:
    alg / disc < 0.5 (FMG's promise is < 1; the prototype gave 0.21), the two
    ratios within 10 % of each other (n-independence), and the values are
    the golden file's."""
    gold = json.load(open(GOLDEN))
    g = fr.GOLDEN
    assert gold["setup"]["sizes"] == list(g["sizes"]) and gold["setup"]["cycles"] == g["cycles"]
    args = (g["pre"], g["post"], g["coarse_sweeps"], g["omegas"])
    ratios = []
    for n, rec in zip(g["sizes"], gold["problems"]):
        exact, _ = fr.model_problem(n)
        u_h = fr.discrete_solution(n)
        disc = fr.max_diff(u_h, exact)
        h = fr.model_hierarchy(n)
        fr.fmg(h, g["cycles"], *args)
        alg = fr.max_diff(h.u[0], u_h)
        print(f"{n}^3: disc {disc:.6e} alg {alg:.6e} alg / disc {alg / disc:.4f}")
        assert rec["n"] == n and rec["disc"] == disc
        assert rec["cubic_2"]["alg"] == alg and rec["cubic_2"]["ratio"] == alg / disc
        assert alg / disc < 0.5
        ratios.append(alg / disc)
        # for the record (the table of DESIGN.md 5.10): only the cubic pass with two cycles gets below disc
        assert rec["cubic_1"]["ratio"] > 1 and rec["trilinear_1"]["ratio"] > 1 and rec["trilinear_2"]["ratio"] > 1
    assert abs(ratios[0] - ratios[1]) <= 0.1 * min(ratios), ratios
