"""Multigrid on the GPU (stencil_restrict_residual, stencil_prolong_add,
stencil_residual_norms, stencil_mg_*; stencil_amd/multigrid.py), against
tests/mg_ref.py.

Every comparison is bit for bit, NaNs compared as NaNs
(tests/special_values.assert_same_values); the one tolerance is the derived
bound on the order of a sum of squares (test_residual_norms).  Fields carry a
value of their own in every ghost cell and poison NaN in all padding
(tests/boundary_data.py), source grids are NaN outside their interior, the
coarse field `e` has its own values in its whole ghost ring (edges and corners
too: the prolongation reads them), destinations hold a sentinel.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from stencil_amd import multigrid as mgm
from stencil_amd.engine import JacobiEngine, StencilSpec
from tests import boundary_data as bd
from tests import mg_ref as mr
from tests import special_values as sv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mg_known_answers.json")
DTYPES = ("fp32", "fp64")
NP = mr.NP
SENTINEL = -777.25
WEIGHTS = (0.8, 1.1)
TX, TY = mgm.RESTRICT_TILE
# one coarse cell more than a tile in x and in y (a ragged second tile), one coarse plane more than a z-run
SEAM = (2 * (TX + 1) + 1, 2 * (TY + 1) + 1, 2 * (mgm.RESTRICT_ZRUN + 1) + 1)
SHAPES = [(7, 5, 3), (15, 15, 15), (131, 61, 29), SEAM]


def test_shapes():
    assert mr.coarse_size(7, 5, 3) == (3, 2, 1)
    cx, cy, cz = mr.coarse_size(*SEAM)
    assert (cx, cy, cz) == (TX + 1, TY + 1, mgm.RESTRICT_ZRUN + 1)
    cx, cy, _ = mr.coarse_size(131, 61, 29)
    assert cx > 2 * TX and cy > 3 * TY  # several tiles, the last one ragged


def engines(gpu, dtype, size):
    fine = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=gpu)
    coarse = mgm.coarsen(fine)
    assert (int(coarse.prob.nx), int(coarse.prob.ny), int(coarse.prob.nz)) == mr.coarse_size(*size)
    return fine, coarse


def poison(grid):
    bd.ibits(grid).fill_(bd.nan_pattern(grid.dtype))


def put_box(e, grid, dense):
    """The whole allocation poison, the ghost-padded box = `dense`."""
    poison(grid)
    bd.box_view(e, grid).copy_(torch.from_numpy(np.ascontiguousarray(dense)))


def source_dense(shape, dtype, seed, values=None):
    """A source array: NaN but for its interior."""
    nx, ny, nz = shape
    g = np.full((nz + 2, ny + 2, nx + 2), np.nan, dtype=NP[dtype])
    g[1:-1, 1:-1, 1:-1] = (np.random.default_rng(seed).uniform(-1, 1, (nz, ny, nx)) if values is None
                           else values).astype(NP[dtype])
    return g


def sentinel_dense(shape, dtype, seed):
    """A destination: boundary_data's ring (poison edges), the sentinel in the interior."""
    nx, ny, nz = shape
    d = bd.ring_field((nz + 2, ny + 2, nx + 2), 1, seed, NP[dtype], True)
    d[1:-1, 1:-1, 1:-1] = SENTINEL
    return d


def coarse_ranges(n):
    return [r for r in ((0, n), (0, 1), (n - 1, n), (1, min(n, 4)), (1, 1)) if 0 <= r[0] <= r[1] <= n]


def check_restrict(fine, coarse, u, g, ranges, what=""):
    """u, g: dense fine arrays already in fine.a / fine.b; coarse.a the destination."""
    size = (int(fine.prob.nx), int(fine.prob.ny), int(fine.prob.nz))
    csize = mr.coarse_size(*size)
    dtype = fine.spec.dtype
    want = mr.restrict_residual(mr.problem(dtype, *size), u, g)
    put_box(coarse, coarse.a, sentinel_dense(csize, dtype, 77))
    torch.cuda.synchronize()
    u0, g0, d0 = fine.a.clone(), fine.b.clone(), coarse.a.clone()
    for cb, ce in ranges:
        coarse.a.copy_(d0)
        mgm.restrict_residual(fine, fine.a, fine.b, coarse, coarse.a, cb, ce)
        got = coarse.interior(coarse.a).cpu().numpy()
        sv.assert_same_values(got[cb:ce], want[cb:ce], f"{what} restriction on coarse planes [{cb}, {ce})")
        rest = np.delete(got, np.s_[cb:ce], axis=0)
        assert (rest == NP[dtype](SENTINEL)).all(), "a coarse plane outside the range was written"
        bd.assert_only_wrote(coarse, d0, coarse.a, cb, ce)
        bd.assert_untouched(fine, u0, fine.a, "fine field")
        bd.assert_untouched(fine, g0, fine.b, "fine source")
    return want


def check_prolong(fine, coarse, u, e, ranges, what=""):
    """u: dense fine array in fine.a; e: dense coarse array in coarse.a."""
    torch.cuda.synchronize()
    u0, e0 = fine.a.clone(), coarse.a.clone()
    full = mr.prolong_add(u, e)
    for b, en in ranges:
        fine.a.copy_(u0)
        mgm.prolong_add(coarse, coarse.a, fine, fine.a, b, en)
        got = fine.to_numpy(fine.a)
        want = mr.prolong_add(u, e, b, en)
        sv.assert_same_values(got[1:-1, 1:-1, 1:-1], want[1:-1, 1:-1, 1:-1], f"{what} prolongation on planes [{b}, {en})")
        bd.assert_only_wrote(fine, u0, fine.a, b, en)
        bd.assert_untouched(coarse, e0, coarse.a, "coarse field")
    fine.a.copy_(u0)
    return full


# --------------------------------------------------------------- operators
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_restrict_residual(gpu, dtype, size):
    fine, coarse = engines(gpu, dtype, size)
    u = bd.poison_and_fill(fine, 901, True, same_ghosts=False)
    g = source_dense(size, dtype, 902)
    put_box(fine, fine.b, g)
    check_restrict(fine, coarse, u, g, coarse_ranges(int(coarse.prob.nz)))


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_prolong_add(gpu, dtype, size):
    fine, coarse = engines(gpu, dtype, size)
    u = bd.poison_and_fill(fine, 903, True, same_ghosts=False)
    cx, cy, cz = mr.coarse_size(*size)
    e = bd.ring_field((cz + 2, cy + 2, cx + 2), 1, 904, NP[dtype], False)  # a box's ring: edges and corners have values
    assert not np.isnan(e).any()
    put_box(coarse, coarse.a, e)
    nz = size[2]
    ranges = [r for r in ((0, nz), (0, 1), (nz - 1, nz), (1, min(nz, 4)), (2, 2)) if r[0] <= r[1] <= nz]
    check_prolong(fine, coarse, u, e, ranges)


def test_odd_index_copy_is_visible():
    """The prolongation's helper differs from one that averages (e + e) at odd
    indices on the overflow class: the special-values case below can tell."""
    e = sv.ring_field((5, 7, 9), 1, 913, np.float32, False, kind="overflow", q=0.05)
    assert (np.abs(e[1:-1, 1:-1, 1:-1]) > np.finfo(np.float32).max / 2).any()


@pytest.mark.parametrize("kind", ["subnormal", "overflow", "nonfinite"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(gpu, dtype, kind):
    """Subnormal, huge, infinite and NaN cells in u, g and e, through the
    restriction, the residual norms and the prolongation."""
    size = (15, 11, 7)
    csize = mr.coarse_size(*size)
    nx, ny, nz = size
    q = {"overflow": 0.05, "nonfinite": 0.01}.get(kind, 0.0)
    padded = (nz + 2, ny + 2, nx + 2)
    cpadded = tuple(n + 2 for n in reversed(csize))
    fine, coarse = engines(gpu, dtype, size)
    p = mr.problem(dtype, *size)
    plain_u = bd.ring_field(padded, 1, 910, NP[dtype], True)
    plain_g = source_dense(size, dtype, 911)
    # few planted sites: a planted cell reaches every coarse cell around it, and most of the result should stay finite
    special_u = sv.ring_field(padded, 1, 912, NP[dtype], True, kind=kind, q=q, limit=4)
    special_g = source_dense(size, dtype, 0, values=sv.draw(kind, (nz, ny, nx), np.random.default_rng(914), NP[dtype], q))
    seen = []  # (result, both operands special)
    for what, u, g in (("special u", special_u, plain_g), ("special g", plain_u, special_g),
                       ("special u and g", special_u, special_g)):
        put_box(fine, fine.a, u)
        put_box(fine, fine.b, g)
        seen.append((check_restrict(fine, coarse, u, g, [(0, csize[2]), (1, 2)], what), "and" in what))
        mx, sq = mgm.residual_norms(fine, fine.a, fine.b)
        wmx, wsq = mr.residual_norms(p, u, g)
        assert np.array_equal(np.isnan(mx), np.isnan(wmx)) and np.array_equal(np.isnan(sq), np.isnan(wsq)), what
        ok = ~np.isnan(wmx)
        assert np.array_equal(mx[ok], wmx[ok]), what
        assert np.array_equal(np.isinf(sq[ok]), np.isinf(wsq[ok])), what
        fin = ok & np.isfinite(wsq)
        assert np.allclose(sq[fin], wsq[fin], rtol=nx * ny * 2.0 ** -52, atol=0), what
    plain_e = bd.ring_field(cpadded, 1, 915, NP[dtype], False)
    special_e = sv.ring_field(cpadded, 1, 916, NP[dtype], False, kind=kind, q=q, limit=4)
    for what, u, e in (("special e", plain_u, special_e), ("special u", special_u, plain_e),
                       ("special u and e", special_u, special_e)):
        put_box(fine, fine.a, u)
        put_box(coarse, coarse.a, e)
        seen.append((check_prolong(fine, coarse, u, e, [(0, nz), (2, 5)], what)[1:-1, 1:-1, 1:-1], "and" in what))
    # the class reached the results: no test passes on a field that has degenerated
    for a, both in seen:
        c = sv.census(a)
        if kind == "subnormal":
            assert not both or c["subnormal"] >= 1, c
        else:
            with np.errstate(invalid="ignore"):
                huge = int((np.isfinite(a) & (np.abs(a) > np.finfo(a.dtype).max / 8)).sum())
            assert c["+inf"] + c["-inf"] + c["nan"] + huge >= 1 and c["normal"] - huge >= 1, (c, huge)


# ------------------------------------------------------------ residual norms
@pytest.mark.parametrize("size", [(15, 15, 15), (131, 61, 29), (301, 9, 5)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_norms(gpu, dtype, size):
    """max_abs is the numpy value bit for bit; sum_sq lies within a relative
    (cells per plane) * 2^-52 of the exact sum of the same squares -- the
    worst case of any order of adding n non-negative terms is (n - 1) 2^-53
    relative, so the bound is derived, not measured."""
    nx, ny, nz = size
    fine = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=gpu)
    p = mr.problem(dtype, *size)
    u = bd.poison_and_fill(fine, 920, True, same_ghosts=False)
    g = source_dense(size, dtype, 921)
    put_box(fine, fine.b, g)
    torch.cuda.synchronize()
    u0, g0 = fine.a.clone(), fine.b.clone()
    d = mr.residual(p, u, g).astype(np.float64)
    want_max = np.abs(d).max(axis=(1, 2))
    want_sum = np.array([math.fsum((pl * pl).ravel().tolist()) for pl in d])
    for b, en in ((0, nz), (1, min(nz, 4)), (nz - 1, nz), (2, 2)):
        mx, sq = mgm.residual_norms(fine, fine.a, fine.b, b, en)
        assert mx.shape == sq.shape == (en - b,)
        assert np.array_equal(mx, want_max[b:en]), (b, en)
        err = np.abs(sq - want_sum[b:en]) / want_sum[b:en] if en > b else np.zeros(0)
        print(f"{dtype} {size} [{b}, {en}): largest relative error of sum_sq {err.max() if en > b else 0.0:.3e}, "
              f"bound {nx * ny * 2.0 ** -52:.3e}")
        assert (err <= nx * ny * 2.0 ** -52).all(), (b, en, err.max())
    again = mgm.residual_norms(fine, fine.a, fine.b)
    assert bd.same_bits(again[1], mgm.residual_norms(fine, fine.a, fine.b)[1])  # equal grids give equal bits
    bd.assert_untouched(fine, u0, fine.a, "field")
    bd.assert_untouched(fine, g0, fine.b, "source")
    # a NaN cell makes its plane NaN, in both outputs, and no other plane
    z = nz // 2
    fine.interior(fine.b)[z, ny // 2, nx // 3] = float("nan")
    mx, sq = mgm.residual_norms(fine, fine.a, fine.b)
    assert np.isnan(mx[z]) and np.isnan(sq[z])
    rest = np.arange(nz) != z
    assert np.array_equal(mx[rest], want_max[rest]) and not np.isnan(sq[rest]).any()


# --------------------------------------------------------------- the cycle
def start_arrays(dtype, size, seed):
    nx, ny, nz = size
    u = bd.ring_field((nz + 2, ny + 2, nx + 2), 1, seed, NP[dtype], True)
    g = np.zeros_like(u)
    g[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed + 5).uniform(-1, 1, (nz, ny, nx)).astype(NP[dtype])
    return u, g


def assert_levels(mg, h, what):
    assert mg.levels == len(h.p)
    for i in range(mg.levels):
        lv = mg.level(i)
        assert lv.shape == (h.p[i].nx, h.p[i].ny, h.p[i].nz)
        sv.assert_same_values(lv.to_numpy(lv.field), h.u[i], f"{what}: field of level {i}")
        sv.assert_same_values(lv.to_numpy(lv.source), h.g[i], f"{what}: source of level {i}")


@pytest.mark.parametrize("size,levels", [((15, 15, 15), 4), ((31, 15, 7), 2)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_vcycle(gpu, dtype, size, levels):
    """One and three V(2,3) cycles with distinct non-dyadic weights: every
    level's field and source are the helper's, bit for bit."""
    u, g = start_arrays(dtype, size, 930)
    mg = mgm.PoissonMultigrid(StencilSpec(dims=3, dtype=dtype), *size, levels=levels, device=gpu)
    try:
        assert mg.levels == levels
        if size == (15, 15, 15):
            assert mg.level(levels - 1).shape == (1, 1, 1)
            assert mgm.PoissonMultigrid(StencilSpec(dims=3, dtype=dtype), *size, device=gpu).levels == 4  # 0 = all
        mg.set_field(u)
        mg.set_source(g)
        h = mr.Hierarchy(dtype, *size, levels, u, g)
        assert_levels(mg, h, "before any cycle")
        done = 0
        for cycles in (1, 3):
            mg.vcycle(pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS, cycles=cycles - done)
            for _ in range(cycles - done):
                mr.vcycle(h, 2, 3, 5, WEIGHTS)
            done = cycles
            assert_levels(mg, h, f"after {cycles} cycles")
            sv.assert_same_values(mg.download(), h.u[0], "download")
            assert mg.residual_norm("max") == mr.residual_norm(h.p[0], h.u[0], h.g[0])
        plan = mg.plan(pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS)
        assert plan["levels"] == levels and plan["launches"] == 2 * (levels - 1) + 2 * (levels - 1) + 2
    finally:
        mg.close()
    assert mg.mg is None


# --------------------------------------------------------------- the solve
def golden_mg(gpu):
    g = mr.GOLDEN
    mg = mgm.PoissonMultigrid(StencilSpec(dims=3, dtype=g["dtype"]), *g["size"], levels=g["levels"], device=gpu)
    u, src = mr.golden_setup()
    mg.set_field(u)
    mg.set_source(src)
    return mg


def golden_args():
    g = mr.GOLDEN
    return dict(pre=g["pre"], post=g["post"], coarse_sweeps=g["coarse_sweeps"], omegas=g["omegas"])


def ref_args():
    g = mr.GOLDEN
    return (g["pre"], g["post"], g["coarse_sweeps"], g["omegas"])


def test_solve_golden_residuals(gpu):
    """31^3 fp64 from the golden file's setup: the residual after every cycle is the file's."""
    gold = json.load(open(GOLDEN))
    mg = golden_mg(gpu)
    try:
        assert mg.residual_norm("max") == gold["residual_start"]
        got = []
        for _ in range(mr.GOLDEN["cycles"]):
            mg.vcycle(**golden_args())
            got.append(mg.residual_norm("max"))
        print("max residual after each cycle:", got)
        assert got == gold["residual_after_cycle"]
        mx, sq = mg.residual_norms()
        assert mg.residual_norm("l2") == float(np.sqrt(sum(float(v) for v in sq))) and mx.max() == got[-1]
    finally:
        mg.close()


@pytest.mark.parametrize("tol,cap,every", [(1e-3, 10, 1), (1e-3, 10, 3), (1e-30, 5, 2), (1e-3, 0, 1), (0.0, 3, 5)])
def test_solve(gpu, tol, cap, every):
    """cycles_done, converged, last_norm and the final grid are mg_ref.solve's:
    convergence, check_every > 1, a tolerance never reached (a last block
    shorter than check_every), max_cycles = 0."""
    h = mr.golden_hierarchy()
    done, conv, last, _ = mr.solve(h, tol, cap, every, *ref_args())
    mg = golden_mg(gpu)
    try:
        r = mg.solve(tol, cap, check_every=every, norm="max", timed=True, **golden_args())
        assert (r.iterations, r.converged) == (done, conv)
        assert r.norm == last
        assert r.ms is not None and (r.ms > 0.0) == (cap > 0)
        lv = mg.level(0)
        assert r.grid.data_ptr() == lv.field.data_ptr()
        sv.assert_same_values(lv.to_numpy(r.grid), h.u[0], "the solve's final grid")
        sv.assert_same_values(mg.download(), h.u[0], "download")
    finally:
        mg.close()
    expect = {(1e-3, 10, 1): (4, True), (1e-3, 10, 3): (6, True), (1e-30, 5, 2): (5, False), (1e-3, 0, 1): (0, False),
              (0.0, 3, 5): (3, False)}
    assert (done, conv) == expect[tol, cap, every]
    if cap == 0:
        assert last == float("inf")


def test_solve_nan_stops(gpu):
    """A NaN residual ends the solve after its first check, not converged."""
    mg = golden_mg(gpu)
    try:
        _, src = mr.golden_setup()
        src[5, 6, 7] = np.nan
        mg.set_source(src)
        r = mg.solve(1e-3, 10, check_every=2, **golden_args())
        assert r.iterations == 2 and not r.converged and math.isnan(r.norm)
    finally:
        mg.close()
