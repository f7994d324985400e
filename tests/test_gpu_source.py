"""Sweeps with a source term on the GPU (stencil_sweepk_source,
stencil_iterate_source, stencil_iterate_until_source, JacobiEngine's methods,
the CLI's --source), against tests/source_ref.py.

Every comparison is bit for bit, NaNs compared as NaNs
(tests/special_values.assert_same_values); there are no tolerances.  Sizes
come from the source shapes' tiles (source_ref.tile).  The field has a value of
its own in every ghost cell and poison NaN in all padding
(tests/boundary_data.py); the source grid is NaN everywhere but its interior,
so a source value read from a ghost cell, a padding column or the tail pad
shows in the result.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import binding as ob
from stencil_amd.engine import JacobiEngine, StencilSpec
from tests import boundary_data as bd
from tests import source_ref as sr
from tests import special_values as sv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "build", "bin", "stencil_main")
K = sr.K_MAX
DTYPES = ("fp32", "fp64")
STEPS = tuple(range(1, K + 1))
NP = {"fp32": np.float32, "fp64": np.float64}
SENTINEL = -777.25


def strip_k(steps):
    """The strip shape whose tiles size a case: the launch's own, K's for the single sweep."""
    return steps if steps >= 2 else K


def seam_size(dtype, steps, nz=9):
    tx, ty = sr.tile(dtype, strip_k(steps))
    nx = tx + 11 if (tx + 11) % 2 else tx + 12
    return nx, ty + 5, nz


def test_tile_table():
    assert sr.tile("fp64", 4) == (56, 32) and sr.tile("fp32", 4) == (120, 32)
    assert sr.tile("fp64", 3) == (58, 42) and sr.tile("fp32", 3) == (120, 42)
    assert sr.tile("fp64", 2) == (60, 52) and sr.tile("fp32", 2) == (124, 52)
    for dt in DTYPES:
        for steps in STEPS:
            nx, ny, _ = seam_size(dt, steps)
            tx, ty = sr.tile(dt, strip_k(steps))
            assert nx % 2 == 1 and tx < nx < 2 * tx and ty < ny < 2 * ty


def make_engine(gpu, dtype, size):
    bd.require_bounded(3, dtype, "star", 1, "naive")
    return JacobiEngine(StencilSpec(dims=3, dtype=dtype), size[0], size[1], size[2], device=gpu)


def set_interior(e, grid, dense, values):
    """Interior cells of a device grid and of its dense host image."""
    e.interior(grid).copy_(torch.from_numpy(np.ascontiguousarray(values)))
    dense[1:-1, 1:-1, 1:-1] = values


def setup(gpu, dtype, size, seed, same_ghosts=False, field=None, source=None):
    """Engine with: grid a = the oracle's `random` interior (or `field`) inside
    boundary_data's ghost ring, grid b a field of its own with the sentinel in
    its interior (same_ghosts: a's ring), the source grid NaN but for its
    interior (uniform in [-1, 1), or `source`).  Returns (engine, dense a,
    dense source)."""
    nx, ny, nz = size
    e = make_engine(gpu, dtype, size)
    start = bd.poison_and_fill(e, seed, True, same_ghosts=same_ghosts)
    p = sr.problem(dtype, nx, ny, nz)
    inner = ob.interior(p, ob.init(p, "random", seed)) if field is None else field
    set_interior(e, e.a, start, inner.astype(NP[dtype]))
    e.interior(e.b).fill_(SENTINEL)
    e.source = torch.empty_like(e.a)
    bd.ibits(e.source).fill_(bd.nan_pattern(e.source.dtype))
    src = np.full_like(start, np.nan)
    vals = np.random.default_rng(seed + 7).uniform(-1, 1, (nz, ny, nx)) if source is None else source
    set_interior(e, e.source, src, vals.astype(NP[dtype]))
    torch.cuda.synchronize()
    return e, start, src


def check_launch(e, start, src, steps, ranges):
    """One source launch a -> b per range: the helper's planes on the range, the
    sentinel on the other planes, every other element of b's allocation as it
    was; a and the source grid untouched."""
    nx, ny, nz = int(e.prob.nx), int(e.prob.ny), int(e.prob.nz)
    p = sr.problem(e.spec.dtype, nx, ny, nz)
    full = sr.sweeps(p, start, src, steps)[1:-1, 1:-1, 1:-1]
    a0, s0, b0 = e.a.clone(), e.source.clone(), e.b.clone()
    for b, en in ranges:
        e.b.copy_(b0)
        e.sweepk_source(e.a, e.b, b, en, steps)
        got = e.interior(e.b).cpu().numpy()
        sv.assert_same_values(got[b:en], full[b:en], f"{steps} source sweeps on [{b}, {en})")
        rest = np.delete(got, np.s_[b:en], axis=0)
        assert (rest == NP[e.spec.dtype](SENTINEL)).all(), "a plane outside the range was written"
        bd.assert_only_wrote(e, b0, e.b, b, en)
        bd.assert_untouched(e, a0, e.a, "input grid")
        bd.assert_untouched(e, s0, e.source, "source grid")


def ranges_of(nz):
    return [r for r in ((0, nz), (0, 1), (2, 7), (nz - 1, nz)) if r[1] <= nz and r[0] < r[1]]


# ---------------------------------------------------------------- launches
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_seams_and_ragged_ends(gpu, dtype, steps):
    size = seam_size(dtype, steps)
    e, start, src = setup(gpu, dtype, size, 301)
    tx, ty = sr.tile(dtype, strip_k(steps))
    assert -(-size[0] // tx) == 2 and -(-size[1] // ty) == 2
    check_launch(e, start, src, steps, ranges_of(size[2]))


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_interior_fast_path(gpu, dtype, steps):
    """3 x 3 tiles: the middle one lies inside the grid and runs without ghost-cell selects."""
    k = strip_k(steps)
    tx, ty = sr.tile(dtype, k)
    size = (3 * tx, 3 * ty, 2 * k + 3)
    e, start, src = setup(gpu, dtype, size, 302)
    check_launch(e, start, src, steps, [(0, size[2]), (2, 7)])


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_planes_than_steps(gpu, dtype, steps):
    nx, ny, _ = seam_size(dtype, steps)
    e, start, src = setup(gpu, dtype, (nx, ny, 2), 303)
    check_launch(e, start, src, steps, [(0, 2), (0, 1), (1, 2)])


@pytest.mark.parametrize("chunk", ["2K", "2K+1"])
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forced_z_chunks(gpu, monkeypatch, dtype, steps, chunk):
    """nz = 4K + 1 in chunks of 2K and 2K + 1 planes (the debug library's
    STENCIL_TK_ZCHUNK): chunk seams, a one-plane last chunk."""
    k = strip_k(steps)
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", str(2 * k + (chunk == "2K+1")))
    nx, ny, _ = seam_size(dtype, steps)
    nz = 4 * k + 1
    e, start, src = setup(gpu, dtype, (nx, ny, nz), 304)
    assert e.lib.stencil_debug_knobs() == 1
    check_launch(e, start, src, steps, [(0, nz), (2, nz - 1)])


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_source_is_the_plain_sweep(gpu, dtype, steps):
    """src = +0 everywhere: bitwise stencil_sweepk on a field without negative zeros."""
    size = seam_size(dtype, steps)
    nx, ny, nz = size
    e = make_engine(gpu, dtype, size)
    e.reset("random", 305)
    assert not bool(torch.signbit(e.interior(e.a)).any())
    e.set_source(np.zeros((nz, ny, nx), dtype=NP[dtype]))
    plain = e.b.clone()
    e.sweepk(e.a, plain, 0, nz, steps)
    e.sweepk_source(e.a, e.b, 0, nz, steps)
    torch.cuda.synchronize()
    assert torch.equal(bd.ibits(e.b), bd.ibits(plain))


def special_cells(dtype, shape, seed):
    """Uniform values with subnormal, huge, infinite and NaN cells among them:
    at the corners, on both sides of the middle, and scattered."""
    fi = np.finfo(NP[dtype])
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1, 1, shape)
    special = [float(fi.smallest_subnormal), -float(fi.smallest_subnormal), float(fi.tiny) / 3, float(fi.max) * 0.75,
               -float(fi.max), np.inf, -np.inf, np.nan]
    nz, ny, nx = shape
    sites = [(0, 0, 0), (nz - 1, ny - 1, nx - 1), (0, ny - 1, 0), (nz // 2, ny // 2, nx // 2), (nz // 2, ny // 2, nx // 2 - 1),
             (1, 3, nx - 1), (nz - 2, 0, 7), (2, ny - 1, 11)]
    for i, at in enumerate(sites):
        f[at] = special[i % len(special)]
    hit = rng.random(shape) < 0.03
    f[hit] = rng.choice(special, size=int(hit.sum()))
    return f.astype(NP[dtype])


@pytest.mark.parametrize("where", ["source", "field"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(gpu, dtype, where):
    size = (20, 12, 6)
    cells = special_cells(dtype, (6, 12, 20), 306)
    assert np.isnan(cells).any() and np.isinf(cells).any()
    e, start, src = setup(gpu, dtype, size, 306, **{where: cells})
    for steps in STEPS:
        check_launch(e, start, src, steps, [(0, 6), (2, 5)])
    want = sr.sweeps(sr.problem(dtype, *size), start, src, K)[1:-1, 1:-1, 1:-1]
    assert np.isnan(want).any() and np.isfinite(want).any()


# -------------------------------------------------------------------- jobs
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_jobs(gpu, dtype):
    size = seam_size(dtype, K)
    nx, ny, nz = size
    p = sr.problem(dtype, nx, ny, nz)
    e, start, src = setup(gpu, dtype, size, 307, same_ghosts=True)
    b_start = bd.dense_of(e, e.b)
    a0, b0, s0 = e.a.clone(), e.b.clone(), e.source.clone()
    want, done = start, 0
    for n in (0, 1, K - 1, K, K + 1, 2 * K + 3, 23):
        e.a.copy_(a0)
        e.b.copy_(b0)
        fin, _ = e.iterate_source(n)
        want = sr.sweeps(p, start, src, n)
        sv.assert_same_values(bd.dense_of(e, fin)[1:-1, 1:-1, 1:-1], want[1:-1, 1:-1, 1:-1], f"{n} sweeps")
        assert e.source_plan(n) == {"launches": -(-n // K), "steps": K}
        assert (fin is e.a) == (-(-n // K) % 2 == 0)
        # ghosts, padding and tail of both grids as they were; the source grid untouched
        bd.assert_only_wrote(e, a0, e.a, 0, nz)
        bd.assert_only_wrote(e, b0, e.b, 0, nz)
        bd.assert_untouched(e, s0, e.source, "source grid")
        done = n
    # a second call continues from the first
    if fin is e.b:
        e.a, e.b = e.b, e.a
    fin2, ms = e.iterate_source(5, timed=True)
    assert ms is not None and ms > 0
    sv.assert_same_values(bd.dense_of(e, fin2)[1:-1, 1:-1, 1:-1], sr.sweeps(p, want, src, 5)[1:-1, 1:-1, 1:-1],
                          f"{done} + 5 sweeps")
    assert b_start.shape == want.shape


# ------------------------------------------------------------- convergence
CONV = {"fp64": ((24, 20, 12), 2e-3), "fp32": ((30, 14, 10), 2e-3)}


@functools.lru_cache(maxsize=None)
def helper_until(dtype, tol, cap, every, nan_source=False):
    size, _ = CONV[dtype]
    p = sr.problem(dtype, *size)
    u = ob.init(p)
    src = np.full_like(u, 1e-3)
    if nan_source:
        src[3, 4, 5] = np.nan
    grid, done, conv, last = sr.until(p, u, src, tol, cap, every)
    grid.setflags(write=False)
    return grid, done, conv, last


def until_engine(gpu, dtype, nan_source=False):
    size, _ = CONV[dtype]
    e = make_engine(gpu, dtype, size)
    e.reset("reference")
    g = np.full((size[2], size[1], size[0]), 1e-3, dtype=NP[dtype])
    if nan_source:
        g[2, 3, 4] = np.nan
    e.set_source(g)
    return e


def check_until(e, dtype, tol, cap, every, nan_source=False):
    grid, done, conv, last = helper_until(dtype, tol, cap, every, nan_source)
    r = e.iterate_until_source(tol, cap, check_every=every)
    print(f"{dtype} tol {tol} cap {cap} every {every}: {r.iterations} sweeps, converged {r.converged}, norm {r.norm!r}; "
          f"helper {done}, {conv}, {last!r}")
    assert (r.iterations, r.converged) == (done, conv)
    assert r.norm == last or (r.norm != r.norm and last != last)
    sv.assert_same_values(bd.dense_of(e, r.grid)[1:-1, 1:-1, 1:-1], np.asarray(grid)[1:-1, 1:-1, 1:-1], "final grid")
    return r


@pytest.mark.parametrize("every", [1, 7, 100])
@pytest.mark.parametrize("dtype", DTYPES)
def test_convergence(gpu, dtype, every):
    _, tol = CONV[dtype]
    _, done, conv, _ = helper_until(dtype, tol, 400, every)
    assert conv and every <= done < 400 and done % every == 0
    check_until(until_engine(gpu, dtype), dtype, tol, 400, every)


@pytest.mark.parametrize("dtype", DTYPES)
def test_convergence_edges(gpu, dtype):
    e = until_engine(gpu, dtype)
    # the cap: a shorter last block, not converged
    r = check_until(e, dtype, 1e-12, 17, 7)
    assert (r.iterations, r.converged) == (17, False)
    # nothing to do
    e.reset("reference")
    r = e.iterate_until_source(1.0, 0, check_every=7)
    assert (r.iterations, r.converged, r.norm) == (0, False, float("inf")) and r.grid is e.a
    # a NaN in the source stops the run at the first check, unconverged
    e = until_engine(gpu, dtype, nan_source=True)
    r = check_until(e, dtype, 1e300, 50, 3, nan_source=True)
    assert (r.iterations, r.converged) == (3, False) and r.norm != r.norm


# -------------------------------------------------------- engine and CLI
def test_engine_methods(gpu):
    size = (37, 19, 9)
    nx, ny, nz = size
    p = sr.problem("fp64", nx, ny, nz)
    e = make_engine(gpu, "fp64", size)
    e.reset("random", 308)
    with pytest.raises(ValueError):
        e.iterate_source(3)  # no source yet
    u = ob.init(p, "random", 308)
    rng = np.random.default_rng(309)
    padded = rng.uniform(-1, 1, u.shape)
    e.set_source(padded)  # the ghost-padded form: its ghost cells are ignored
    src = np.full_like(u, np.nan)
    src[1:-1, 1:-1, 1:-1] = padded[1:-1, 1:-1, 1:-1]
    fin, _ = e.iterate_source(7)
    bd.assert_bitwise(bd.dense_of(e, fin)[1:-1, 1:-1, 1:-1], sr.sweeps(p, u, src, 7)[1:-1, 1:-1, 1:-1], "iterate_source")
    e.reset("random", 308)
    e.set_source(torch.from_numpy(padded[1:-1, 1:-1, 1:-1].copy()))  # the interior form, a tensor
    grid, done, conv, last = sr.until(p, u, src, 0.05, 60, 4)
    r = e.iterate_until_source(0.05, 60, check_every=4)
    assert (r.iterations, r.converged, r.norm) == (done, conv, last)
    bd.assert_bitwise(bd.dense_of(e, r.grid)[1:-1, 1:-1, 1:-1], grid[1:-1, 1:-1, 1:-1], "iterate_until_source")
    with pytest.raises(ValueError):
        e.set_source(np.zeros((nz, ny, nx + 1)))
    e.set_source(None)
    with pytest.raises(ValueError):
        e.sweepk_source(e.a, e.b, 0, nz, 1)


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_cli_hip_source(gpu):
    """stencil_main --dims 3 -s 24 -i 30 -m HIP --source 0.001 -c (with the
    required -b) passes its own check and ends on the helper's grid; with --tol
    it stops where the helper does."""
    p = sr.problem("fp32", 24, 24, 24)
    u = ob.init(p)
    src = np.full_like(u, np.float32(0.001))
    out = cli("--dims", "3", "-s", "24", "-b", "4", "-i", "30", "-m", "HIP", "--source", "0.001", "-c")
    assert out.returncode == 0, out.stdout + out.stderr
    assert "The results of method HIP is correct." in out.stdout
    sums = re.findall(r"^\[stencil-amd\] HIP: source 0\.001, 30 sweeps, interior sum = (\S+)$", out.stdout, flags=re.M)
    assert len(sums) == 2 and all(float(v) == sr.interior_sum(sr.sweeps(p, u, src, 30)) for v in sums), sums
    grid, done, conv, _ = sr.until(p, u, src, 2e-3, 400, 7)
    assert conv and 7 < done < 400
    out = cli("--dims", "3", "-s", "24", "-b", "4", "-i", "400", "-m", "HIP", "--source", "0.001", "--tol", "2e-3",
              "--check-every", "7", "-c")
    assert out.returncode == 0, out.stdout + out.stderr
    counts = re.findall(r"^\[stencil-amd\] HIP: converged after (\d+) sweeps", out.stdout, flags=re.M)
    assert len(counts) == 2 and all(int(n) == done for n in counts), (counts, done)
    sums = re.findall(r"interior sum = (\S+)$", out.stdout, flags=re.M)
    assert len(sums) == 2 and all(float(v) == sr.interior_sum(grid) for v in sums)
