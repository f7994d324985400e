"""Source launches (stencil_sweepk_source, K = 2, 3, 4) and checking launches
(stencil_sweepk_update_max, K = 3, 4, 5) on every schedule path of the strip
kernel's host routine (kernels_strip.hip launch_st): the packed z-chunk table,
the per-step and per-segment select-free steps of an interior tile, the first
launch's trial, the XCD-patch orders, and the calls of 256 sweeps or more.

Every comparison is bit for bit against the CPU helpers the other files use
(tests/source_ref.py; the oracle pair of tests/test_gpu_update_max.py), NaNs
compared as NaNs; there are no tolerances.  The setups are those files' too
(sentinel interior and NaN source padding; a field of its own in every ghost
cell and NaN in all padding), so every launch's write footprint is checked:
only the interior cells of [begin, end) change, the input and the source never.

Shapes.  For a launch kind with output tile (TX, TY) and K sweeps: nz =
3 (2K + 1) + 1 planes, which forced table chunks of lc = 2K + 1 planes cut
into a chunk at the low z end, a middle chunk every stage of which stays
inside in z (seg_fast() holds), a chunk that leaves the grid only at the high
z end (K >= 3: the per-step choice mixes both step variants in one segment),
and a one-plane remainder dispatched last.  Planes: `inner` = 3 TX x 3 TY,
whose middle tile alone has its whole region inside the grid; `ragged` = one
more, partly filled tile column and row, nx odd (an fp32 lane vector is cut at
the row's end).  interior_tiles() restates the kernel's region_inner and each
test asserts the tiles it expects.

Which path ran is read from the debug library's STENCIL_TK_VERBOSE lines
(launches_in): the launch line gives the tile grid, the equal chunk and the
workgroups launched, a `pack:` line appears when the process builds a table,
a `schedule trial:` line when the first launch times both schedules.
  * a forced table launches tiles x ceil(planes / lc) workgroups, and its
    `pack:` line (seen when this process built it: TABLES) names that count
    without "-- not used";
  * forced equal chunks launch tiles x ceil(planes / zc) and build no table.
STENCIL_TK_PACK_LC and STENCIL_TK_ZCHUNK are both 2K + 1 in the first two cases,
so their counts are equal by construction there; the launch line's chunk field
(the forced zc, against the model's own chunk beside a table) and the `pack:`
line tell them apart.  The XCD case also runs equal chunks of 3K + 1 planes,
whose counts differ from the table's on both ranges, which it asserts.
"""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import binding as ob
from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, StencilSpec
from tests import boundary_data as bd
from tests import source_ref as sr
from tests import special_values as sv
from tests import test_gpu_boundary_data as tb
from tests import test_gpu_source as sg
from tests import test_gpu_update_max as um

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "fp64")
LAUNCHES = ([("source", dt, k) for dt in DTYPES for k in (2, 3, 4)]
            + [("check", dt, k) for dt in DTYPES for k in (3, 4, 5)])
FP64_LAUNCHES = [c for c in LAUNCHES if c[1] == "fp64"]
SIZES = ("inner", "ragged")
FAST = (None, 0, 1, 4, 5)  # STENCIL_TK_FAST: unset, no select-free step, per step, per segment, both
SUSTAINED = 256            # kSustainedSweeps (common.hpp): a call of that many sweeps orders its tables in XCD patches


def case_id(case):
    return "-".join(str(c) for c in case)


def strip_of(kind, dtype, k):
    """(cells per lane V, rows per wave RY) of the launch's strip shape."""
    return sr.STRIP[dtype, k] if kind == "source" else um.STRIP[dtype, k]


def tile_of(kind, dtype, k):
    return sr.tile(dtype, k) if kind == "source" else um.tile(dtype, k)


def planes_of(k):
    return 3 * (2 * k + 1) + 1


def size_of(kind, dtype, k, which):
    tx, ty = tile_of(kind, dtype, k)
    if which == "inner":
        return 3 * tx, 3 * ty, planes_of(k)
    nx = 3 * tx + 11
    return nx if nx % 2 else nx + 1, 3 * ty + 5, planes_of(k)


def tile_grid(kind, dtype, k, size):
    tx, ty = tile_of(kind, dtype, k)
    return -(-size[0] // tx), -(-size[1] // ty)


def interior_tiles(kind, dtype, k, size):
    """The kernel's region_inner: tile (bx, by)'s region -- x from bx TX -
    ceil(K / V) V, 64 V wide; y from by TY - K, 8 RY high -- lies inside the grid."""
    v, ry = strip_of(kind, dtype, k)
    tx, ty = tile_of(kind, dtype, k)
    ring = -(-k // v) * v
    gx, gy = tile_grid(kind, dtype, k, size)
    return {(bx, by) for bx in range(gx) for by in range(gy)
            if bx * tx - ring >= 0 and bx * tx - ring + 64 * v <= size[0]
            and by * ty - k >= 0 and by * ty - k + 8 * ry <= size[1]}


def assert_shape(kind, dtype, k, size, which):
    """The tile grid and the interior tiles the size was built for."""
    tx, ty = tile_of(kind, dtype, k)
    if which == "inner":
        assert tile_grid(kind, dtype, k, size) == (3, 3) and size[0] % tx == 0 and size[1] % ty == 0
        assert interior_tiles(kind, dtype, k, size) == {(1, 1)}
    else:
        assert tile_grid(kind, dtype, k, size) == (4, 4) and size[0] % 2 == 1
        assert 0 < size[0] - 3 * tx < tx and 0 < size[1] - 3 * ty < ty
        assert interior_tiles(kind, dtype, k, size) == {(1, 1), (2, 1), (1, 2), (2, 2)}
    assert size[2] == 3 * (2 * k + 1) + 1


def test_shapes():
    for kind, dtype, k in LAUNCHES:
        for which in SIZES:
            assert_shape(kind, dtype, k, size_of(kind, dtype, k, which), which)
    assert size_of("source", "fp64", 4, "inner") == (168, 96, 28)
    assert size_of("check", "fp64", 4, "ragged") == (179, 149, 28)
    assert size_of("check", "fp32", 5, "inner") == (348, 90, 34)


# ------------------------------------------------- the library's launch lines
STRIP_LINE = re.compile(r"tkstrip K=(\d+) V=(\d+) RY=(\d+) NW=(\d+): tiles (\d+)x(\d+), zchunk (-?\d+), (\d+) workgroups")
PACK_LINE = re.compile(r"pack: equal chunks -?\d+ steps, packed -?\d+ steps \((\d+) workgroups, XCD patches (-?\d+) wide\)"
                       r"( -- not used)?")
TRIAL_LINE = re.compile(r"schedule trial: .* -> (packed|equal chunks)")


def launches_in(err):
    """The strip launches of a captured stderr, in order: each with the `pack:`
    lines printed just before its launch line (the tables that call built) and
    the `schedule trial:` verdict printed after it."""
    out, packs = [], []
    for line in err.splitlines():
        m = PACK_LINE.match(line)
        if m:
            packs.append(SimpleNamespace(workgroups=int(m[1]), width=int(m[2]), used=m[3] is None))
            continue
        m = STRIP_LINE.match(line)
        if m:
            k, v, ry, _, gx, gy, zc, n = (int(g) for g in m.groups())
            out.append(SimpleNamespace(k=k, v=v, ry=ry, grid=(gx, gy), zc=zc, n=n, packs=packs, trial=None))
            packs = []
            continue
        m = TRIAL_LINE.match(line)
        if m and out:
            out[-1].trial = m[1]
    return out


def read_launches(capfd):
    """The launches since the last read; what the test printed meanwhile goes on to pytest's report."""
    cap = capfd.readouterr()
    print(cap.out, end="")
    return launches_in(cap.err)


def of_shape(launches, kind, dtype, k):
    """The launches of the kind's own strip shape."""
    v, ry = strip_of(kind, dtype, k)
    return [x for x in launches if (x.k, x.v, x.ry) == (k, v, ry)]


# (kind, dtype, k, size, planes, lc, order) -> the `pack:` line of that table.  The library prints it once,
# when the process builds the table.  A call without STENCIL_TK_PACK_XCD builds two: the tile-major table
# ("short") and the XCD-patch one of the calls of >= 256 sweeps ("long"), the other order's first.
TABLES = {}


def note_tables(launch, key, order):
    if order in ("short", "long") and len(launch.packs) == 2:
        TABLES[key + ("long" if order == "short" else "short",)], TABLES[key + (order,)] = launch.packs
    elif order not in ("short", "long") and len(launch.packs) == 1:
        TABLES[key + (order,)] = launch.packs[0]
    else:
        assert not launch.packs, launch.packs


def assert_table(launch, case, size, planes, lc, order="short"):
    """The launch ran the forced table of lc-plane chunks; returns its `pack:` line."""
    gx, gy = tile_grid(*case, size)
    want = gx * gy * -(-planes // lc)
    assert launch.grid == (gx, gy) and launch.n == want, (launch, want)
    key = case + (size, planes, lc)
    note_tables(launch, key, order)
    assert key + (order,) in TABLES, f"no `pack:` line seen for the table of {key}, order {order}"
    line = TABLES[key + (order,)]
    assert line.used and line.workgroups == want, (line, want)
    return line


def assert_equal_chunks(launch, case, size, planes, zc):
    """The launch ran forced equal chunks of zc planes, and built no table."""
    gx, gy = tile_grid(*case, size)
    want = gx * gy * -(-planes // zc)
    assert launch.grid == (gx, gy) and (launch.zc, launch.n) == (zc, want) and not launch.packs, (launch, want)
    return want


def knobs(monkeypatch, **env):
    monkeypatch.setenv("STENCIL_TK_VERBOSE", "1")
    for name, value in env.items():
        if value is None:
            monkeypatch.delenv("STENCIL_TK_" + name, raising=False)
        else:
            monkeypatch.setenv("STENCIL_TK_" + name, str(value))


# ------------------------------------------------------ one checked launch
ORACLE_PAIRS = {}


class SourceRun:
    """test_gpu_source's setup; launch() is its check_launch on one range."""

    def __init__(self, gpu, dtype, k, size, seed):
        self.k = k
        self.e, self.start, self.src = sg.setup(gpu, dtype, size, seed)
        self.b0 = self.e.b.clone()

    def launch(self, b, en):
        self.e.b.copy_(self.b0)
        sg.check_launch(self.e, self.start, self.src, self.k, [(b, en)])
        return self.e.b.clone()


class CheckRun:
    """test_gpu_update_max's random-field setup; launch() is its check() with the footprint."""

    def __init__(self, gpu, dtype, k, size, seed):
        self.k = k
        self.e = um.make_engine(gpu, dtype, size)
        start = bd.poison_and_fill(self.e, seed, True, same_ghosts=False)
        key = (dtype, k, size, seed)
        if key not in ORACLE_PAIRS:
            ORACLE_PAIRS[key] = um.oracle_pair(dtype, size, start, k)
        self.prev, self.cur = ORACLE_PAIRS[key]
        self.a0, self.b0 = self.e.a.clone(), self.e.b.clone()

    def launch(self, b, en):
        self.e.b.copy_(self.b0)
        um.check(self.e, self.prev, self.cur, self.k, b, en)
        bd.assert_only_wrote(self.e, self.b0, self.e.b, b, en)
        bd.assert_untouched(self.e, self.a0, self.e.a)
        return self.e.b.clone()


def make_run(gpu, case, size, seed):
    """The engine is built under the knobs set so far: it loads the debug library."""
    kind, dtype, k = case
    run = (SourceRun if kind == "source" else CheckRun)(gpu, dtype, k, size, seed)
    assert run.e.lib.stencil_debug_knobs() == 1
    return run


def launch_and_read(run, capfd, case, b, en):
    """One checked launch; returns (its launch line, grid b's whole allocation after it)."""
    read_launches(capfd)
    out = run.launch(b, en)
    torch.cuda.synchronize()
    mine = of_shape(read_launches(capfd), *case)
    assert len(mine) == 1, mine
    return mine[0], out


def ranges_of(nz):
    return (0, nz), (2, nz - 1)


def same_allocation(x, y):
    return torch.equal(bd.ibits(x), bd.ibits(y))


# ------------------------------------------------------------ launch cases
@pytest.mark.parametrize("which", SIZES)
@pytest.mark.parametrize("case", LAUNCHES, ids=case_id)
def test_forced_packed_table(gpu, monkeypatch, capfd, case, which):
    """STENCIL_TK_PACK=2 with STENCIL_TK_PACK_LC=2K+1: the table of the module
    docstring, and the sub-range's own.  With the knob STENCIL_TK_FAST unset a
    table launch has both select-free paths on (fp64)."""
    k = case[2]
    lc = 2 * k + 1
    knobs(monkeypatch, PACK=2, PACK_LC=lc)
    size = size_of(*case, which)
    assert_shape(*case, size, which)
    run = make_run(gpu, case, size, 401)
    for b, en in ranges_of(size[2]):
        launch, _ = launch_and_read(run, capfd, case, b, en)
        assert_table(launch, case, size, en - b, lc)


@pytest.mark.parametrize("which", SIZES)
@pytest.mark.parametrize("case", LAUNCHES, ids=case_id)
def test_equal_chunks(gpu, monkeypatch, capfd, case, which):
    """STENCIL_TK_ZCHUNK=2K+1: the same cuts as equal chunks, chunk-major, no table."""
    k = case[2]
    knobs(monkeypatch, ZCHUNK=2 * k + 1)
    size = size_of(*case, which)
    assert_shape(*case, size, which)
    run = make_run(gpu, case, size, 402)
    for b, en in ranges_of(size[2]):
        launch, _ = launch_and_read(run, capfd, case, b, en)
        assert_equal_chunks(launch, case, size, en - b, 2 * k + 1)


@pytest.mark.parametrize("schedule", ["table", "equal"])
@pytest.mark.parametrize("case", FP64_LAUNCHES, ids=case_id)
def test_fast_settings_agree(gpu, monkeypatch, capfd, case, schedule):
    """fp64, the `inner` size (the per-step path is compiled for the fp64
    one-cell-per-lane shapes only): STENCIL_TK_FAST unset, 0, 1, 4 and 5 on the
    forced table and on equal chunks.  Every setting is the reference bit for
    bit (launch()), and the whole allocations of grid b agree with each other.
    1 and 5 turn the per-step choice on for equal chunks too."""
    k = case[2]
    lc = 2 * k + 1
    knobs(monkeypatch, **({"PACK": 2, "PACK_LC": lc} if schedule == "table" else {"ZCHUNK": lc}))
    size = size_of(*case, "inner")
    assert_shape(*case, size, "inner")
    run = make_run(gpu, case, size, 403)
    for b, en in ranges_of(size[2]):
        outs = []
        for fast in FAST:
            knobs(monkeypatch, FAST=fast)
            launch, out = launch_and_read(run, capfd, case, b, en)
            if schedule == "table":
                assert_table(launch, case, size, en - b, lc)
            else:
                assert_equal_chunks(launch, case, size, en - b, lc)
            outs.append(out)
        for fast, out in zip(FAST[1:], outs[1:]):
            assert same_allocation(out, outs[0]), f"STENCIL_TK_FAST={fast} on [{b}, {en}) differs from the knob unset"


@pytest.mark.parametrize("case", LAUNCHES, ids=case_id)
def test_first_launch_trial(gpu, monkeypatch, capfd, case):
    """STENCIL_TK_PACK=1 (the default rule) on a table of 2K+2-plane chunks, a
    length no other test gives this kernel: the table's verdict is untested in
    this process, so the first launch is pick_schedule's -- six launches,
    packed and equal chunks in turn, all into grid b -- and the second runs the
    verdict.  Both are the reference bit for bit with a clean footprint."""
    k = case[2]
    lc = 2 * k + 2
    knobs(monkeypatch, PACK=1, PACK_LC=lc)
    size = size_of(*case, "inner")
    assert_shape(*case, size, "inner")
    nz = size[2]
    run = make_run(gpu, case, size, 404)
    first, _ = launch_and_read(run, capfd, case, 0, nz)
    second, _ = launch_and_read(run, capfd, case, 0, nz)
    print(f"{case_id(case)}: trial -> {first.trial}; first launch {first}, second {second}")
    assert first.trial in ("packed", "equal chunks") and second.trial is None, (first, second)
    table = 9 * -(-nz // lc)
    assert first.n == table and first.grid == (3, 3)
    assert second.n == (table if first.trial == "packed" else 9 * -(-nz // second.zc))


@pytest.mark.parametrize("case", LAUNCHES, ids=case_id)
def test_xcd_patch_orders(gpu, monkeypatch, capfd, case):
    """STENCIL_TK_PACK_XCD=2 on the forced table (generations of 9 tiles, so
    the patch order really permutes them), and STENCIL_TK_XCD=2 on equal
    chunks, whose grid is rounded up to a multiple of 8 workgroups: the surplus
    ones must do nothing.  Equal chunks of 2K+1 planes (the table's cuts) and
    of 3K+1, whose workgroup counts differ from the table's on both ranges."""
    k = case[2]
    lc = 2 * k + 1
    size = size_of(*case, "inner")
    assert_shape(*case, size, "inner")
    knobs(monkeypatch, PACK=2, PACK_LC=lc, PACK_XCD=2)
    run = make_run(gpu, case, size, 405)
    tables = {}
    for b, en in ranges_of(size[2]):
        launch, _ = launch_and_read(run, capfd, case, b, en)
        assert assert_table(launch, case, size, en - b, lc, order="xcd2").width == 2
        tables[b, en] = launch.n
    knobs(monkeypatch, PACK=None, PACK_LC=None, PACK_XCD=None, XCD=2)
    for zc in (lc, 3 * k + 1):
        knobs(monkeypatch, ZCHUNK=zc)
        for b, en in ranges_of(size[2]):
            launch, _ = launch_and_read(run, capfd, case, b, en)
            n = assert_equal_chunks(launch, case, size, en - b, zc)
            assert n % 8 != 0, n  # the launched grid has surplus workgroups
            assert zc == lc or n != tables[b, en], (n, tables)


# ------------------------------------- where the checking launch's maximum sits
def table_spikes(dtype, k, size):
    """Cells (z, y, x) of the `inner` size's interior tile (1, 1): name -> cell."""
    tx, ty = um.tile(dtype, k)
    lc = 2 * k + 1
    cx, cy = tx + tx // 2, ty + ty // 2
    cells = {"seg-fast chunk": (lc + k, cy, cx), "mixed chunk": (2 * lc + k, cy + 1, cx + 1),
             "remainder chunk": (3 * lc, cy, cx)}
    cells.update({f"chunk seam, plane {z}": (z, cy, cx) for z in (lc - 1, lc, 2 * lc - 1, 2 * lc)})
    cells.update({f"x seam, column {x}": (lc + k, cy, x) for x in (tx - 1, tx, 2 * tx - 1, 2 * tx)})
    cells.update({f"y seam, row {y}": (lc + k, y, cx) for y in (ty - 1, ty, 2 * ty - 1, 2 * ty)})
    assert size[2] == 3 * lc + 1 and len(set(cells.values())) == 15
    return cells


@pytest.mark.parametrize("dtype,k", um.CASES)
def test_where_the_maximum_sits_on_the_table(gpu, monkeypatch, capfd, dtype, k):
    """Forced table, zero field with one spike (test_gpu_update_max.spike_start):
    the update's maximum sits at the spike (odd K) or next to it (even K), so a
    cell whose |t_K - t_(K-1)| the launch misses -- in the interior tile's
    select-free steps, at a table chunk's seam, in the remainder chunk, at the
    tile's x and y seams -- changes the word.  Grid b starts as NaN everywhere,
    so the footprint is checked too.  Last, a NaN in the interior tile."""
    case = ("check", dtype, k)
    lc = 2 * k + 1
    knobs(monkeypatch, PACK=2, PACK_LC=lc)
    size = size_of(*case, "inner")
    assert_shape(*case, size, "inner")
    nz = size[2]
    e = um.make_engine(gpu, dtype, size)
    assert e.lib.stencil_debug_knobs() == 1
    cells = table_spikes(dtype, k, size)

    def launch(start, what):
        prev, cur = um.oracle_pair(dtype, size, start, k)
        um.zero_grids(e)
        e.interior(e.a).copy_(torch.from_numpy(start[1:-1, 1:-1, 1:-1]))
        bd.ibits(e.b).fill_(bd.nan_pattern(e.b.dtype))
        a0, b0 = e.a.clone(), e.b.clone()
        torch.cuda.synchronize()
        read_launches(capfd)
        print(what)
        got = um.check(e, prev, cur, k, 0, nz)
        bd.assert_only_wrote(e, b0, e.b, 0, nz)
        bd.assert_untouched(e, a0, e.a)
        mine = of_shape(read_launches(capfd), *case)
        assert len(mine) == 1, mine
        assert_table(mine[0], case, size, nz, lc)
        return got, prev, cur

    for name, cell in cells.items():
        start = um.spike_start(size, cell, dtype, k)
        got, prev, cur = launch(start, f"{name} {cell}")
        d = um.update(prev, cur)
        top = np.argwhere(d == d.max())
        assert d.max() > 0 and np.abs(top - cell).sum(axis=1).max() <= (0 if k % 2 else 1), (name, cell, top.tolist())
    start = um.spike_start(size, cells["seg-fast chunk"], dtype, k)
    z, y, x = cells["mixed chunk"]
    start[1 + z, 1 + y, 1 + x] = np.nan
    got, _, _ = launch(start, "NaN in the interior tile")
    assert got != got


# -------------------------------------------------------------------- jobs
def job_setup(gpu, dtype, size, seed):
    e, start, src = sg.setup(gpu, dtype, size, seed, same_ghosts=True)
    return e, start, src, (e.a.clone(), e.b.clone(), e.source.clone())


def assert_job_footprint(e, before):
    nz = int(e.prob.nz)
    bd.assert_only_wrote(e, before[0], e.a, 0, nz)
    bd.assert_only_wrote(e, before[1], e.b, 0, nz)
    bd.assert_untouched(e, before[2], e.source, "source grid")


def interior_of(dense):
    return dense[1:-1, 1:-1, 1:-1]


THREADS = 16


def _add_planes(out, src, first, last):
    with np.errstate(all="ignore"):
        out[first:last, 1:-1, 1:-1] += src[first:last, 1:-1, 1:-1]


def long_source_sweeps(p, u, src, steps):
    """source_ref.sweeps for the long jobs: the same cells by the same two
    operations -- the oracle's sweep, then numpy's add of the source's interior
    -- without sweep()'s copy per sweep: two buffers that both hold u's ghosts,
    swept in turn on THREADS oracle threads (every cell is computed alone), the
    source added to slabs of planes side by side.  test_long_reference pins it
    on source_ref.sweeps."""
    from concurrent.futures import ThreadPoolExecutor
    a, b = u.copy(), u.copy()
    cuts = np.linspace(1, 1 + p.nz, min(THREADS, p.nz) + 1).astype(int)
    with ThreadPoolExecutor(THREADS) as pool:
        for _ in range(steps):
            ob.sweep(p, a, b, 0, p.nz, THREADS)
            list(pool.map(lambda z: _add_planes(b, src, z[0], z[1]), zip(cuts[:-1], cuts[1:])))
            a, b = b, a
    return a


@pytest.mark.parametrize("dtype,size", [("fp32", (67, 29, 11)), ("fp64", (20, 12, 40))])
def test_long_reference(dtype, size):
    """long_source_sweeps is source_ref.sweeps bit for bit, NaN and infinite cells included."""
    p = sr.problem(dtype, *size)
    u = ob.init(p, "random", 410)
    src = np.random.default_rng(411).uniform(-1, 1, u.shape).astype(u.dtype)
    src[3, 4, 5], src[5, 6, 7], u[2, 3, 4] = np.nan, np.inf, -np.inf
    for steps in (0, 1, 9):
        sv.assert_same_values(long_source_sweeps(p, u, src, steps), sr.sweeps(p, u, src, steps), f"{steps} sweeps")


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_source_call_on_the_forced_table(gpu, monkeypatch, capfd, dtype):
    """iterate_source(257): 64 fused K = 4 launches, each on the forced table
    in the XCD-patch order of a call of >= 256 sweeps, and one single sweep."""
    case = ("source", dtype, sr.K_MAX)
    k, lc = sr.K_MAX, 2 * sr.K_MAX + 1
    knobs(monkeypatch, PACK=2, PACK_LC=lc)
    size = size_of(*case, "inner")
    assert_shape(*case, size, "inner")
    e, start, src, before = job_setup(gpu, dtype, size, 406)
    assert e.lib.stencil_debug_knobs() == 1
    n = SUSTAINED + 1
    assert e.source_plan(n) == {"launches": n // k + 1, "steps": k} and n % k == 1
    read_launches(capfd)
    fin, _ = e.iterate_source(n)
    torch.cuda.synchronize()
    mine = of_shape(read_launches(capfd), *case)
    want = long_source_sweeps(sr.problem(dtype, *size), start, src, n)
    sv.assert_same_values(interior_of(bd.dense_of(e, fin)), interior_of(want), f"{n} source sweeps")
    assert_job_footprint(e, before)
    assert len(mine) == n // k
    for launch in mine:
        line = assert_table(launch, case, size, size[2], lc, order="long")
    print(f"{dtype}: the sustained call's table: {line.workgroups} workgroups, XCD patches {line.width} wide")


PACKED_SOURCE = {}


def smallest_packed_source_shape(gpu, capfd, dtype):
    """The smallest of the project's candidate shapes whose K = 4 source launch
    the model itself packs (debug library, STENCIL_TK_VERBOSE alone): the
    launch's `pack:` line without "-- not used", or, when the table was built
    earlier in the process, a workgroup count that equal chunks do not give.
    None when no candidate packs."""
    if dtype in PACKED_SOURCE:
        return PACKED_SOURCE[dtype]
    case = ("source", dtype, sr.K_MAX)
    found = None
    for size in sorted(tb.PACKED_CANDIDATES, key=lambda s: s[0] * s[1] * s[2]):
        e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=gpu)
        assert e.lib.stencil_debug_knobs() == 1
        e.a.zero_()
        e.source = torch.zeros_like(e.a)
        read_launches(capfd)
        e.sweepk_source(e.a, e.b, 0, size[2], sr.K_MAX)
        torch.cuda.synchronize()
        launch, = of_shape(read_launches(capfd), *case)
        gx, gy = tile_grid(*case, size)
        packed = launch.packs[-1].used if launch.packs else launch.n != gx * gy * -(-size[2] // launch.zc)
        print(f"{dtype} {size}: source launch {launch} -> {'packed' if packed else 'not packed'}")
        del e
        if packed:
            found = size
            break
    PACKED_SOURCE[dtype] = found
    return found


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_source_call_in_the_product_library(gpu, monkeypatch, capfd, dtype):
    """The same 257 sweeps with no experiment knob set: the product library's
    own rule (trial included), at the smallest shape whose source launch the
    model packs -- the `inner` size if no candidate does.  On MI355X that is
    512 x 512 x 96 for fp64 (its reference is the oracle on 16 threads); no
    candidate packs the fp32 source shape."""
    knobs(monkeypatch)
    size = smallest_packed_source_shape(gpu, capfd, dtype)
    print(f"{dtype}: the model packs the source launch at {size}")
    if size is None:
        size = size_of("source", dtype, sr.K_MAX, "inner")
    monkeypatch.delenv("STENCIL_TK_VERBOSE")
    assert not _lib.debug_knobs_requested()
    e, start, src, before = job_setup(gpu, dtype, size, 407)
    assert e.lib.stencil_debug_knobs() == 0
    n = SUSTAINED + 1
    fin, _ = e.iterate_source(n)
    torch.cuda.synchronize()
    want = long_source_sweeps(sr.problem(dtype, *size), start, src, n)
    sv.assert_same_values(interior_of(bd.dense_of(e, fin)), interior_of(want), f"{n} source sweeps")
    assert_job_footprint(e, before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_source_block(gpu, monkeypatch, capfd, dtype):
    """iterate_until_source, one block of 300 sweeps to a tolerance out of
    reach: its first 299 are one stencil_iterate_source call of >= 256 sweeps
    (74 K = 4 launches and one K = 3 launch on the forced tables), then the
    single sweep and the norm."""
    case = ("source", dtype, sr.K_MAX)
    k, lc = sr.K_MAX, 2 * sr.K_MAX + 1
    knobs(monkeypatch, PACK=2, PACK_LC=lc)
    size = size_of(*case, "inner")
    nz = size[2]
    e, start, src, before = job_setup(gpu, dtype, size, 408)
    assert e.lib.stencil_debug_knobs() == 1
    every = cap = 300
    tol = 1e-300
    read_launches(capfd)
    r = e.iterate_until_source(tol, cap, check_every=every)
    torch.cuda.synchronize()
    launches = read_launches(capfd)
    # source_ref.until of the block: its first 299 sweeps are source_ref.sweeps' (long_source_sweeps), its
    # last sweep and the check the helper's own
    p = sr.problem(dtype, *size)
    grid, done, conv, last = sr.until(p, long_source_sweeps(p, start, src, every - 1), src, tol, 1, 1)
    done += every - 1
    print(f"{dtype}: {r.iterations} sweeps, converged {r.converged}, norm {r.norm!r}; helper {done}, {conv}, {last!r}")
    assert (done, conv) == (cap, False) and last > tol
    assert (r.iterations, r.converged) == (done, conv)
    assert np.float64(r.norm).view(np.uint64) == np.float64(last).view(np.uint64)
    sv.assert_same_values(interior_of(bd.dense_of(e, r.grid)), interior_of(grid), "final grid")
    assert_job_footprint(e, before)
    fused = of_shape(launches, *case)
    assert len(fused) == (every - 1) // k, fused
    for launch in fused:
        assert_table(launch, case, size, nz, lc, order="long")
    rest = of_shape(launches, "source", dtype, (every - 1) % k)
    gx, gy = tile_grid("source", dtype, (every - 1) % k, size)
    assert (every - 1) % k == 3 and len(rest) == 1 and rest[0].n == gx * gy * -(-nz // lc), rest


PLAIN_BLOCKS = [("fp64", 4, 260), ("fp32", 5, 260), ("fp32", 5, 261)]


@pytest.mark.parametrize("dtype,k,every", PLAIN_BLOCKS)
def test_long_plain_block_with_a_fused_check(gpu, monkeypatch, capfd, dtype, k, every):
    """iterate_until (max norm), one block of `every` sweeps to a tolerance out
    of reach: every - K sweeps as one stencil_iterate call, then the checking
    launch on the forced table.  260 - 4 = 256 sweeps make the fp64 call a
    sustained one; fp32 runs K = 5 on planes this small only with
    STENCIL_TK_STEPS=5 (a documented variable of both libraries), and its
    260 - 5 = 255 sweeps stay below kSustainedSweeps, so it also runs 261."""
    case = ("check", dtype, k)
    lc = 2 * k + 1
    knobs(monkeypatch, PACK=2, PACK_LC=lc)
    if dtype == "fp32":
        monkeypatch.setenv("STENCIL_TK_STEPS", str(k))
    size = size_of(*case, "inner")
    assert_shape(*case, size, "inner")
    nx, ny, nz = size
    e = um.make_engine(gpu, dtype, size)
    assert e.lib.stencil_debug_knobs() == 1 and e.fuse_steps == k
    assert e.until_plan(every)["fused_check"]
    assert um.PLAIN_RY[dtype, k] == um.STRIP[dtype, k][1]  # the plain launches print the checking launch's shape
    start = bd.poison_and_fill(e, 409, True)
    a0, b0 = e.a.clone(), e.b.clone()
    read_launches(capfd)
    tol = 1e-300
    r = e.iterate_until(tol, every, check_every=every)
    torch.cuda.synchronize()
    mine = of_shape(read_launches(capfd), *case)
    p = ob.problem(3, dtype, "star", 1, "naive", nx, ny, nz)
    old = bd.oracle_steps(p, start, every - 1, nz, threads=THREADS)
    cur = old.copy()
    ob.sweep(p, old, cur, 0, nz, THREADS)
    want = float(um.update(interior_of(old), interior_of(cur)).max())
    print(f"{dtype} K={k}: {r.iterations} sweeps, converged {r.converged}, norm {r.norm!r}; the oracle's {want!r}")
    assert want > tol and (r.iterations, r.converged) == (every, False)
    assert np.float64(r.norm).view(np.uint64) == np.float64(want).view(np.uint64)
    bd.assert_bitwise(e.interior(r.grid).cpu().numpy(), interior_of(cur), f"after {every} sweeps")
    bd.assert_only_wrote(e, a0, e.a, 0, nz)
    bd.assert_only_wrote(e, b0, e.b, 0, nz)
    # the K-step launches of the sweeps before the check, then the checking launch: the table, every one
    assert len(mine) == (every - k) // k + 1, mine
    assert all(x.n == 9 * -(-nz // lc) and x.grid == (3, 3) for x in mine), mine
    assert (every - k >= SUSTAINED) == ((dtype, every) != ("fp32", 260))
