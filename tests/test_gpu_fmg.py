"""Full multigrid on the GPU (stencil_restrict_source, stencil_inject_ghosts,
stencil_prolong_cubic, stencil_mg_fmg; stencil_amd/multigrid.py), against
tests/fmg_ref.py.

Every comparison is bit for bit, NaNs compared as NaNs
(tests/special_values.assert_same_values).  Fields carry a value of their own
in every ghost cell -- edges and corners of the ring too: the injection copies
them and the prolongation reads them -- and poison NaN in all padding
(tests/boundary_data.py); source grids are NaN outside their interior;
destinations hold a sentinel, and every launch is followed by a check of the
whole allocation of both grids.
"""
import json
import os

import numpy as np
import pytest
import torch

from stencil_amd import multigrid as mgm
from stencil_amd.engine import JacobiEngine, StencilSpec
from tests import boundary_data as bd
from tests import fmg_ref as fr
from tests import mg_ref as mr
from tests import special_values as sv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fmg_known_answers.json")
DTYPES = ("fp32", "fp64")
NP = mr.NP
SENTINEL = -777.25
WEIGHTS = (0.8, 1.1)
TX, TY = mgm.RESTRICT_TILE
# one coarse cell more than a restriction tile in x and in y, one coarse plane more than a z-run
SEAM = (2 * (TX + 1) + 1, 2 * (TY + 1) + 1, 2 * (mgm.RESTRICT_ZRUN + 1) + 1)
# (7, 5, 3): coarse extents 3, 2, 1 -- the central window, both one-sided ones and the linear case in one shape
SHAPES = [(7, 5, 3), (15, 15, 15), (131, 61, 29), SEAM]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def test_shapes():
    assert SEAM == (67, 19, 19) and mr.coarse_size(7, 5, 3) == (3, 2, 1)
    assert fr.window(1, 3)[1] == fr.W_MID and fr.window(0, 2)[1] == fr.W_FIRST and fr.window(2, 2)[1] == fr.W_LAST


def engines(gpu, dtype, size):
    fine = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=gpu)
    coarse = mgm.coarsen(fine)
    assert (int(coarse.prob.nx), int(coarse.prob.ny), int(coarse.prob.nz)) == mr.coarse_size(*size)
    return fine, coarse


def put_box(e, grid, dense):
    """The whole allocation poison, the ghost-padded box = `dense`."""
    bd.ibits(grid).fill_(bd.nan_pattern(grid.dtype))
    bd.box_view(e, grid).copy_(torch.from_numpy(np.ascontiguousarray(dense)))


def padded(size):
    return (size[2] + 2, size[1] + 2, size[0] + 2)


def source_dense(size, dtype, seed, values=None):
    """A source array: NaN but for its interior."""
    nx, ny, nz = size
    g = np.full(padded(size), np.nan, dtype=NP[dtype])
    g[1:-1, 1:-1, 1:-1] = (np.random.default_rng(seed).uniform(-1, 1, (nz, ny, nx)) if values is None
                           else values).astype(NP[dtype])
    return g


def sentinel_dense(size, dtype, seed, star=True):
    """A destination: boundary_data's ring, the sentinel in the interior."""
    d = bd.ring_field(padded(size), 1, seed, NP[dtype], star)
    d[1:-1, 1:-1, 1:-1] = SENTINEL
    return d


def distinct_ring(size, dtype, seed):
    """A dense field whose ghost-shell cells (edges and corners included) all differ: a seeded permutation of
    0.5, 1.0, 1.5, ... with alternating signs (exact in fp32; seeded normals collide at these counts)."""
    u = bd.ring_field(padded(size), 1, seed, NP[dtype], False)
    mask = fr.shell_mask(u.shape)
    n = int(mask.sum())
    vals = (np.random.default_rng(seed + 2).permutation(n) + 1) * 0.5
    u[mask] = (vals * np.where(np.arange(n) % 2, -1.0, 1.0)).astype(NP[dtype])
    return u


def ranges_of(n):
    return [r for r in ((0, n), (0, 1), (n - 1, n), (1, min(n, 4)), (1, 1)) if 0 <= r[0] <= r[1] <= n]


def check_restrict_source(fine, coarse, g, ranges, what=""):
    """g: the dense fine source already in fine.b; coarse.a the destination."""
    dtype = fine.spec.dtype
    csize = (int(coarse.prob.nx), int(coarse.prob.ny), int(coarse.prob.nz))
    want = fr.coarse_source(g)
    put_box(coarse, coarse.a, sentinel_dense(csize, dtype, 77))
    torch.cuda.synchronize()
    g0, d0 = fine.b.clone(), coarse.a.clone()
    for cb, ce in ranges:
        coarse.a.copy_(d0)
        mgm.restrict_source(fine, fine.b, coarse, coarse.a, cb, ce)
        got = coarse.interior(coarse.a).cpu().numpy()
        sv.assert_same_values(got[cb:ce], want[cb:ce], f"{what} source restriction on coarse planes [{cb}, {ce})")
        bd.assert_only_wrote(coarse, d0, coarse.a, cb, ce)
        bd.assert_untouched(fine, g0, fine.b, "fine source")
    # the whole range as two launches
    cz = csize[2]
    cut = max(1, cz // 2) if cz > 1 else 0
    coarse.a.copy_(d0)
    mgm.restrict_source(fine, fine.b, coarse, coarse.a, 0, cut)
    mgm.restrict_source(fine, fine.b, coarse, coarse.a, cut, cz)
    sv.assert_same_values(coarse.interior(coarse.a).cpu().numpy(), want, f"{what} source restriction in two launches")
    bd.assert_only_wrote(coarse, d0, coarse.a, 0, cz)
    bd.assert_untouched(fine, g0, fine.b, "fine source")
    return want


def check_prolong_cubic(fine, coarse, u, e, ranges, what=""):
    """u: the dense fine destination in fine.a; e: the dense coarse array in coarse.a."""
    torch.cuda.synchronize()
    u0, e0 = fine.a.clone(), coarse.a.clone()
    nz = int(fine.prob.nz)
    for b, en in ranges:
        fine.a.copy_(u0)
        mgm.prolong_cubic(coarse, coarse.a, fine, fine.a, b, en)
        got = fine.to_numpy(fine.a)
        want = fr.prolong_cubic_set(u, e, b, en)
        sv.assert_same_values(got[1:-1, 1:-1, 1:-1], want[1:-1, 1:-1, 1:-1], f"{what} cubic prolongation on planes [{b}, {en})")
        bd.assert_only_wrote(fine, u0, fine.a, b, en)
        bd.assert_untouched(coarse, e0, coarse.a, "coarse field")
    cut = nz // 2 + 1  # an odd or an even first plane of the second launch, by shape
    fine.a.copy_(u0)
    mgm.prolong_cubic(coarse, coarse.a, fine, fine.a, 0, cut)
    mgm.prolong_cubic(coarse, coarse.a, fine, fine.a, cut, nz)
    full = fr.prolong_cubic_set(u, e)
    sv.assert_same_values(fine.to_numpy(fine.a)[1:-1, 1:-1, 1:-1], full[1:-1, 1:-1, 1:-1],
                          f"{what} cubic prolongation in two launches")
    bd.assert_only_wrote(fine, u0, fine.a, 0, nz)
    bd.assert_untouched(coarse, e0, coarse.a, "coarse field")
    fine.a.copy_(u0)
    return full


def check_inject(fine, coarse, u, c, what=""):
    """u: the dense fine field in fine.a; c: the dense coarse start in coarse.a.
    The coarse allocation afterwards is the one before with the box's shell
    replaced, bit for bit (copies: NaN payloads too)."""
    torch.cuda.synchronize()
    u0, c0 = fine.a.clone(), coarse.a.clone()
    mgm.inject_ghosts(fine, fine.a, coarse, coarse.a)
    torch.cuda.synchronize()
    want = fr.inject_ghosts(u, c)
    expect = c0.clone()
    bd.box_view(coarse, expect).copy_(torch.from_numpy(np.ascontiguousarray(want)))
    changed = bd.ibits(expect) != bd.ibits(coarse.a)
    n = int(changed.sum().item())
    if n:
        i = int(torch.nonzero(changed)[0].item())
        raise AssertionError(f"{what} injection: {n} elements of the coarse allocation are wrong; first at "
                             f"{bd.locate(coarse, i)}")
    assert bd.same_bits(want[1:-1, 1:-1, 1:-1], c[1:-1, 1:-1, 1:-1])  # the interior stayed
    bd.assert_untouched(fine, u0, fine.a, "fine field")
    return want


# --------------------------------------------------------------- the kernels
@pytest.mark.parametrize("size", SHAPES, ids=IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_restrict_source(gpu, dtype, size):
    fine, coarse = engines(gpu, dtype, size)
    g = source_dense(size, dtype, 951)
    put_box(fine, fine.b, g)
    check_restrict_source(fine, coarse, g, ranges_of(int(coarse.prob.nz)))


@pytest.mark.parametrize("size", SHAPES, ids=IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_inject_ghosts(gpu, dtype, size):
    fine, coarse = engines(gpu, dtype, size)
    u = distinct_ring(size, dtype, 952)
    shell = u[fr.shell_mask(u.shape)]
    assert not np.isnan(shell).any() and len(np.unique(shell)) == shell.size
    put_box(fine, fine.a, u)
    c = sentinel_dense(mr.coarse_size(*size), dtype, 953, star=False)
    put_box(coarse, coarse.a, c)
    want = check_inject(fine, coarse, u, c)
    assert (want[1:-1, 1:-1, 1:-1] == NP[dtype](SENTINEL)).all()


@pytest.mark.parametrize("size", SHAPES, ids=IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_prolong_cubic(gpu, dtype, size):
    fine, coarse = engines(gpu, dtype, size)
    u = sentinel_dense(size, dtype, 954)
    put_box(fine, fine.a, u)
    e = bd.ring_field(padded(mr.coarse_size(*size)), 1, 955, NP[dtype], False)
    assert not np.isnan(e).any()
    put_box(coarse, coarse.a, e)
    nz = size[2]
    ranges = [r for r in ((0, nz), (0, 1), (nz - 1, nz), (1, min(nz, 4)), (2, 2)) if r[0] <= r[1] <= nz]
    check_prolong_cubic(fine, coarse, u, e, ranges)


def test_prolongation_is_a_set(gpu):
    """A NaN interior of u does not reach the result: u is not read."""
    size = (15, 11, 7)
    fine, coarse = engines(gpu, "fp64", size)
    u = bd.ring_field(padded(size), 1, 956, np.float64, True)
    u[1:-1, 1:-1, 1:-1] = np.nan
    put_box(fine, fine.a, u)
    e = bd.ring_field(padded(mr.coarse_size(*size)), 1, 957, np.float64, False)
    put_box(coarse, coarse.a, e)
    mgm.prolong_cubic(coarse, coarse.a, fine, fine.a)
    got = fine.to_numpy(fine.a)[1:-1, 1:-1, 1:-1]
    assert not np.isnan(got).any() and bd.same_bits(got, fr.prolong_cubic(e))


@pytest.mark.parametrize("kind", ["subnormal", "overflow", "nonfinite"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(gpu, dtype, kind):
    """Subnormal, huge, infinite and NaN cells in g, in e and in the ring,
    through the three kernels; compared as the existing special-value tests do."""
    size = (15, 11, 7)
    csize = mr.coarse_size(*size)
    nx, ny, nz = size
    q = {"overflow": 0.05, "nonfinite": 0.01}.get(kind, 0.0)
    fine, coarse = engines(gpu, dtype, size)
    seen = []
    g = source_dense(size, dtype, 0, values=sv.draw(kind, (nz, ny, nx), np.random.default_rng(960), NP[dtype], q))
    put_box(fine, fine.b, g)
    seen.append(check_restrict_source(fine, coarse, g, [(0, csize[2]), (1, 2)], "special g"))
    e = sv.ring_field(padded(csize), 1, 961, NP[dtype], False, kind=kind, q=q, limit=4)
    u = sentinel_dense(size, dtype, 962)
    put_box(fine, fine.a, u)
    put_box(coarse, coarse.a, e)
    seen.append(check_prolong_cubic(fine, coarse, u, e, [(0, nz), (2, 5)], "special e")[1:-1, 1:-1, 1:-1])
    ring = sv.ring_field(padded(size), 1, 963, NP[dtype], False, kind=kind, q=q, limit=4)
    put_box(fine, fine.a, ring)
    c = sentinel_dense(csize, dtype, 964, star=False)
    put_box(coarse, coarse.a, c)
    inj = check_inject(fine, coarse, ring, c, "special ring")
    seen.append(inj[fr.shell_mask(inj.shape)])
    # the class reached the results: no test passes on a field that has degenerated
    for a in seen:
        cen = sv.census(a)
        if kind == "subnormal":
            assert cen["subnormal"] >= 1, cen
        else:
            with np.errstate(invalid="ignore"):
                huge = int((np.isfinite(a) & (np.abs(a) > np.finfo(a.dtype).max / 64)).sum())
            assert cen["+inf"] + cen["-inf"] + cen["nan"] + huge >= 1, (cen, huge)


# ----------------------------------------------------------------- the pass
def start_arrays(dtype, size, seed):
    """A field whose interior is NaN (the pass ignores it) inside a ring of
    distinct values, edges and corners included; a seeded source."""
    nx, ny, nz = size
    u = bd.ring_field(padded(size), 1, seed, NP[dtype], False)
    u[1:-1, 1:-1, 1:-1] = np.nan
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


def levels_of(mg):
    out = []
    for i in range(mg.levels):
        lv = mg.level(i)
        out.append((lv.to_numpy(lv.field), lv.to_numpy(lv.source)))
    return out


@pytest.mark.parametrize("size,levels", [((15, 15, 15), 4), ((31, 15, 7), 2), ((15, 15, 15), 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fmg(gpu, dtype, size, levels):
    """The pass with 0, 1 and 2 V(2,3) cycles per level, distinct non-dyadic
    weights, 5 coarse sweeps: every level's field and source are the helper's,
    bit for bit."""
    u, g = start_arrays(dtype, size, 970)
    mg = mgm.PoissonMultigrid(StencilSpec(dims=3, dtype=dtype), *size, levels=levels, device=gpu)
    try:
        assert mg.levels == levels
        mg.set_source(g)
        for cycles in (0, 1, 2):
            mg.set_field(u)
            mg.fmg(cycles=cycles, pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS)
            h = mr.Hierarchy(dtype, *size, levels, u, g)
            fr.fmg(h, cycles, 2, 3, 5, WEIGHTS)
            assert_levels(mg, h, f"{cycles} cycles per level")
            assert not np.isnan(h.u[0]).any()
            sv.assert_same_values(mg.download(), h.u[0], "download")
        # (L-1) x (source restriction, injection, cubic prolongation), the coarsest run, 2 cycles from every level
        plan = mg.fmg_plan(cycles=2, pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS)
        assert plan == {"levels": levels, "launches": 3 * (levels - 1) + mg_cycle_launches(mg, levels - 1)
                        + 2 * sum(mg_cycle_launches(mg, s) for s in range(levels - 1))}, plan
    finally:
        mg.close()


def mg_cycle_launches(mg, start):
    """The launches of a V(2,3) cycle with 5 coarse sweeps started at level `start` of mg's hierarchy."""
    shape = mg.shape
    for _ in range(start):
        shape = mr.coarse_size(*shape)
    return mgm.mg_plan(mg.spec, *shape, levels=mg.levels - start, pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS)["launches"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_vcycles_after_fmg_find_zero_ghosts(gpu, dtype):
    """The pass injects Dirichlet data into both field grids of every coarse
    level; a V-cycle relies on their ghost cells being zero.  After fmg, a
    V-cycle from an uploaded field equals, on every level, the same cycle on
    a freshly created hierarchy -- and a second fmg reproduces the first."""
    size, levels = (15, 15, 15), 4
    u, g = start_arrays(dtype, size, 980)
    field = bd.ring_field(padded(size), 1, 985, NP[dtype], True)
    spec = StencilSpec(dims=3, dtype=dtype)
    mg = mgm.PoissonMultigrid(spec, *size, levels=levels, device=gpu)
    fresh = mgm.PoissonMultigrid(spec, *size, levels=levels, device=gpu)
    try:
        mg.set_source(g)
        mg.set_field(u)
        mg.fmg(cycles=2, pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS)
        first = levels_of(mg)
        fresh.set_source(g)
        h = mr.Hierarchy(dtype, *size, levels, field, g)
        for n in (1, 2):   # two cycles: the second runs on the grids the first left
            for m in (mg, fresh):
                if n == 1:
                    m.set_field(field)
                m.vcycle(pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS)
            mr.vcycle(h, 2, 3, 5, WEIGHTS)
            for i, ((fa, sa), (fb, sb)) in enumerate(zip(levels_of(mg), levels_of(fresh))):
                sv.assert_same_values(fa, fb, f"cycle {n} after fmg: field of level {i}")
                sv.assert_same_values(sa, sb, f"cycle {n} after fmg: source of level {i}")
            assert_levels(mg, h, f"cycle {n} after fmg")
        mg.set_field(u)
        mg.fmg(cycles=2, pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS)
        for i, ((fa, sa), (fb, sb)) in enumerate(zip(levels_of(mg), first)):
            assert bd.same_bits(fa, fb) and bd.same_bits(sa, sb), f"the second fmg differs on level {i}"
        # without a new upload too: the pass ignores the interior it left
        mg.fmg(cycles=2, pre=2, post=3, coarse_sweeps=5, omegas=WEIGHTS)
        for i, ((fa, sa), (fb, sb)) in enumerate(zip(levels_of(mg), first)):
            assert bd.same_bits(fa, fb) and bd.same_bits(sa, sb), f"the third fmg differs on level {i}"
    finally:
        mg.close()
        fresh.close()


def test_golden_problem(gpu):
    """31^3 fp64, the model problem of tests/fmg_ref.py: the downloaded field
    gives the stored alg / disc, and a following solve converges."""
    gold = json.load(open(GOLDEN))
    g = fr.GOLDEN
    n = 31
    rec = [p for p in gold["problems"] if p["n"] == n][0]
    exact, src = fr.model_problem(n)
    start = exact.copy()
    start[1:-1, 1:-1, 1:-1] = 0.0
    u_h = fr.discrete_solution(n)
    args = dict(pre=g["pre"], post=g["post"], coarse_sweeps=g["coarse_sweeps"], omegas=g["omegas"])
    mg = mgm.PoissonMultigrid(StencilSpec(dims=3, dtype="fp64"), n, n, n, device=gpu)
    try:
        assert mg.levels == 5
        mg.set_field(start)
        mg.set_source(src)
        mg.fmg(cycles=g["cycles"], **args)
        got = mg.download()
        alg, disc = fr.max_diff(got, u_h), fr.max_diff(u_h, exact)
        print(f"31^3: alg {alg:.6e} disc {disc:.6e} alg / disc {alg / disc:.4f} (stored {rec['cubic_2']['ratio']:.4f})")
        assert disc == rec["disc"] and alg == rec["cubic_2"]["alg"] and alg / disc == rec["cubic_2"]["ratio"]
        assert alg / disc < 0.5
        before = mg.residual_norm("max")
        r = mg.solve(1e-12, 15, **args)
        print(f"residual after fmg {before:.3e}; solve: {r.iterations} cycles to {r.norm:.3e}")
        assert r.converged and r.norm <= 1e-12 < before
        assert fr.max_diff(mg.download(), u_h) < 1e-3 * alg
    finally:
        mg.close()
