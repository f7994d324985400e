"""The fp64 K = 4 strip's sliver mode on the GPU (kernels_strip.hip SLIVER;
DESIGN.md §5.2): grids whose last tile column is at most 8 columns wide run it
as sliver workgroups, four tile rows side by side in the 16-lane groups of a
region row.

Shapes: nx = 57, 64, 120 leave 1, 8 and 8 ragged columns beside one or two
main tile columns; ny = 48, 50, 100, 200 give one lane group in use, two,
three, and two sliver workgroups of 4 + 1 tile rows; nz = 3, 9, 23 planes.
Every case runs the packed table forced, equal chunks forced, the model's own
table and the mode switched off; all must agree with one another and
with the oracle bit for bit, and nothing but interior cells may change in
allocations that hold NaN everywhere else (tests/boundary_data.py)."""
import math

import numpy as np
import pytest
import torch

from oracle import binding as ob
from tests import boundary_data as bd
from tests import special_values as sv
from tests import test_gpu_boundary_data as tb

pytestmark = pytest.mark.gpu

TX, TY, K = 56, 48, 4                    # the fp64 K = 4 strip's output tile
PACK_LC = {3: 2, 9: 4, 23: 8}            # forced packed chunks: 2 + 1, 4 + 4 + 1, 8 + 8 + 7 planes
ZCHUNK = 5
# the mode is on in calls of >= 256 sweeps; STENCIL_TK_SLIVER=1 (debug library) turns it on in every launch
WAYS = {"packed": {"STENCIL_TK_SLIVER": "1", "STENCIL_TK_PACK": "2"},   # + STENCIL_TK_PACK_LC per case
        "equal": {"STENCIL_TK_SLIVER": "1", "STENCIL_TK_ZCHUNK": str(ZCHUNK)},
        "model": {"STENCIL_TK_SLIVER": "1"},   # the model's own table (none under 2K planes: equal chunks)
        "off": {"STENCIL_TK_SLIVER": "0"}}
# long calls only: the default rule -- the sliver table where one exists, timed against the plain launch by
# the first launch's trial, the plain launch otherwise -- in the debug and in the product library
LONG_WAYS = {"auto": {"STENCIL_TK_SLIVER": "-1"}, "product": {}}


@pytest.fixture(scope="module", autouse=True)
def drop_references():
    """The shared oracle grids of this file are released when it is done."""
    yield
    for key in [k for k in tb._STATES if k[-1] == "sliver"]:
        del tb._STATES[key]


def sliver_tiles(nx, ny):
    gx, gy = math.ceil(nx / TX), math.ceil(ny / TY)
    assert gx >= 2 and nx - (gx - 1) * TX <= 8
    return (gx - 1) * gy + math.ceil(gy / 4), gx * gy


def environment(m, way, nz):
    for k, v in {**WAYS, **LONG_WAYS}[way].items():
        m.setenv(k, v)
    if way == "packed":
        m.setenv("STENCIL_TK_PACK_LC", str(PACK_LC.get(nz, 4)))


def check_geometry(e, way, size):
    """The launch is the one the case is about: the forced grids count the
    sliver mode's tiles, the switched-off launch the plain tile grid's."""
    nx, ny, nz = size
    on, plain = sliver_tiles(nx, ny)
    geo = e.sweepk_geometry(K)
    if way != "product":
        assert e.lib.stencil_debug_knobs() == 1
    if way == "packed":  # the sliver workgroups take half-length chunks (pack_search)
        lc, main = PACK_LC.get(nz, 4), (math.ceil(nx / TX) - 1) * math.ceil(ny / TY)
        want = main * math.ceil(nz / lc) + (on - main) * math.ceil(nz / math.ceil(lc / 2))
        assert geo["packed"] and geo["workgroups"] == want, geo
    elif way == "equal":
        assert geo["zchunk"] == ZCHUNK and geo["workgroups"] == on * math.ceil(nz / ZCHUNK), geo
    elif way == "model":
        assert bool(geo["packed"]) == (nz >= 2 * K), geo
    elif way == "off" and not geo["packed"]:
        assert geo["workgroups"] % plain == 0, geo


@pytest.mark.parametrize("nz", [3, 9, 23])
@pytest.mark.parametrize("ny", [48, 50, 100, 200])
@pytest.mark.parametrize("nx", [57, 64, 120])
def test_sliver_launch_and_job(gpu, monkeypatch, nx, ny, nz):
    """One stencil_sweepk launch a -> b (grid b holds another field) and a
    9-sweep stencil_iterate job (two K = 4 launches and a single sweep)."""
    size = (nx, ny, nz)
    launched, jobs = {}, {}
    for way in WAYS:
        with monkeypatch.context() as m:
            environment(m, way, nz)
            e, p, start, tall, key = tb.setup_single(gpu, "fp64", "star", "temporalk", size, 701)
            check_geometry(e, way, size)
            tb.check_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, K), p, start, K, [(0, nz)], key + ("sliver",))
            launched[way] = e.b.clone()
            e, p, start, key = tb.setup_job(gpu, 3, "fp64", "star", 1, "naive", "auto", size, 702)
            assert e.fuse_steps == K
            tb.check_job(e, p, start, 2 * K + 1, nz, key + ("sliver",))
            jobs[way] = (e.a.clone(), e.b.clone())
    for way in WAYS:  # whole allocations, bit for bit
        assert torch.equal(bd.ibits(launched[way]), bd.ibits(launched["off"])), way
        assert all(torch.equal(bd.ibits(x), bd.ibits(y)) for x, y in zip(jobs[way], jobs["off"])), way


@pytest.mark.parametrize("way", list(WAYS))
def test_thirteen_sweeps(gpu, monkeypatch, way):
    """4 + 4 + 4 + 1 sweeps: the grids swap roles between sliver launches."""
    size = (120, 200, 23)
    environment(monkeypatch, way, size[2])
    e, p, start, key = tb.setup_job(gpu, 3, "fp64", "star", 1, "naive", "auto", size, 703)
    assert e.plan(13)[0] == 4
    tb.check_job(e, p, start, 13, size[2], key + ("sliver",))


@pytest.mark.parametrize("nz", [9, 3])
@pytest.mark.parametrize("way", ["packed", "off", "auto", "product"])
def test_long_job_takes_the_patch_table(gpu, monkeypatch, way, nz):
    """257 sweeps in one call: the packed table in XCD-patch order, the sliver
    entries behind each generation's main tiles.  `auto` / `product`: the
    default rule, which turns the mode on for a call this long where it has a
    table (9 planes: the first launch times it against the plain launch) and
    runs the plain launch where it has none (3 planes)."""
    size = (64, 100, nz)
    if way in ("packed", "off"):
        environment(monkeypatch, "packed", nz)
        if way == "off":
            monkeypatch.setenv("STENCIL_TK_SLIVER", "0")
    else:
        environment(monkeypatch, way, nz)
    e, p, start, key = tb.setup_job(gpu, 3, "fp64", "star", 1, "naive", "auto", size, 704)
    assert way in LONG_WAYS or e.sweepk_geometry(K)["packed"]
    assert (e.lib.stencil_debug_knobs() == 1) == (way != "product")
    tb.check_job(e, p, start, 257, nz, key + ("sliver",))


GHOSTS = np.array([-0.0, 5e-324, -5e-324, np.inf, 2.5e-310, -np.inf, 2.2250738585072014e-308, -0.0])


@pytest.mark.parametrize("kind", list(sv.KINDS))
def test_special_values(gpu, monkeypatch, kind):
    """The value classes of tests/special_values.py, and a ghost column x = nx
    -- the column every sliver tile keeps beside its output columns -- of
    -0.0, subnormals and infinities: it is read at every stage, never computed,
    and has its bits after the job."""
    size = (64, 100, 9)
    nx, ny, nz = size
    for way in WAYS:
        with monkeypatch.context() as m:
            environment(m, way, nz)
            e = tb.make_engine(gpu, 3, "fp64", "star", 1, "naive", "auto", size)
            sv.poison_and_fill(e, 705, True, kind=kind, q=0.002, limit=12)
            column = np.resize(GHOSTS, (nz, ny))
            for grid in (e.a, e.b):
                bd.box_view(e, grid)[1:-1, 1:-1, -1] = torch.from_numpy(column).to(grid.device)
            start = bd.dense_of(e, e.a)
            assert bd.same_bits(start[1:-1, 1:-1, -1], column)
            p = ob.problem(3, "fp64", "star", 1, "naive", nx, ny, nz)
            key = ("fp64", size, 705, kind, "sliver")
            want = tb.oracle_interiors(key, p, start, 2 * K + 1, nz)
            assert np.isfinite(want).any() and not np.isfinite(want).all()  # the infinite ghosts reach the interior
            with sv.comparing(sv.assert_same_values):
                tb.check_job(e, p, start, 2 * K + 1, nz, key)
            for grid in (e.a, e.b):
                assert bd.same_bits(bd.dense_of(e, grid)[1:-1, 1:-1, -1], column), (way, "the ghost column changed")
