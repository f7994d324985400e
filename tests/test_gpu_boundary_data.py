"""Every kernel family on fields whose boundary data varies by plane and row.

All other GPU parity tests start from ghosts that are the same in every row
and plane (x-ghosts 1, the rest 0, which is also what fresh padding holds).
Here (tests/boundary_data.py) every ghost cell has a value of its own, the
destination of a single launch has ghosts different from the source's, a
star's ring edges and corners are NaN, and all padding -- row padding, unused
ghost planes, the 256-B tail -- is NaN.  Every comparison is bitwise against
`ob.sweep` applied step by step to the dense start array, and every one also
checks, over the whole allocation, that the launch stored nothing outside the
interior cells of its own planes (`assert_only_wrote`) and left its source
alone.  tests/test_oracle_boundary_data.py shows on the CPU that the oracle
is a sound judge of such fields and that the old fields could not see what
these see.

Each parametrised shape asserts the launch regime it was chosen for: more
than one tile in x and y with a ragged last tile, more than one z-chunk, a
packed schedule, one workgroup, one persistent launch.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import binding as ob
from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, SlabJob, StencilSpec
from tests import boundary_data as bd

pytestmark = pytest.mark.gpu

HALO = _lib.HALO_LO | _lib.HALO_HI
# The default regions of the K-step kernels: 64 V x 56 cells for the 3D strip kernels
# (V = 1 fp64, 2 fp32), 128 x 64 for the 2D strip.  A grid wider and taller than a region has a ragged last
# tile and, at those shapes, more than one tile in x and in y (an output tile is a region less its ring);
# where the library reports its launch (stencil_sweepk_geometry, the face-signal count) the tests ask it.
REGION3 = {"fp64": (64, 56), "fp32": (128, 56)}
REGION2 = (128, 64)


def make_engine(gpu, dims, dtype, shape, r, order, kernel, size, halo=0, flags=0):
    nx, ny, nz = size
    bd.require_bounded(dims, dtype, shape, r, order)
    spec = StencilSpec(dims=dims, dtype=dtype, shape=shape, radius=r, order=order, kernel=kernel, halo=halo)
    return JacobiEngine(spec, nx, ny, nz, device=gpu, flags=flags)


_STATES: dict = {}


def oracle_interiors(key, p, start, steps, slow, threads=1):
    """Interior of the oracle's grid after `steps` sweeps of `start`, computed
    once per `key` and extended sweep by sweep (cases share their reference).
    Small grids keep every sweep's interior, large ones only those asked for."""
    r = p.radius
    inner = tuple(slice(r, -r) for _ in range(start.ndim))
    st = _STATES.get(key)
    if st is None or (steps < st["done"] and steps not in st["at"]):
        st = _STATES[key] = {"done": 0, "a": start.copy(), "b": start.copy(), "at": {0: start[inner].copy()}}
    keep_all = start.nbytes <= 32 << 20
    while st["done"] < steps:
        ob.sweep(p, st["a"], st["b"], 0, slow, threads)
        st["a"], st["b"] = st["b"], st["a"]
        st["done"] += 1
        if keep_all or st["done"] == steps:
            st["at"][st["done"]] = st["a"][inner].copy()
    return st["at"][steps]


def subrange(n, chunk=0):
    """An interior range [b, e), 0 < b, e < n, whose length is no multiple of the forced z-chunk."""
    if n < 8:
        return 1, n - 1
    b, e = 3, n - 4
    if chunk and (e - b) % chunk == 0:
        b = 2
    assert 0 < b < e < n and not (chunk and (e - b) % chunk == 0)
    return b, e


def check_launch(e, launch, p, start, steps, ranges, key, tall=0):
    """Run `launch(src, dst, b, e)` a -> b for every range: the interior of
    [b, e) is the oracle's after `steps` sweeps, every other element of the
    destination's allocation keeps its bits, the source is untouched."""
    nz = int(e.prob.nz)
    want = oracle_interiors(key, p, start, steps, nz + 2 * tall)
    src0 = e.a.clone()
    dst0 = e.b.clone()
    for b, en in ranges:
        e.b.copy_(dst0)
        launch(e.a, e.b, b, en)
        torch.cuda.synchronize()
        bd.assert_only_wrote(e, dst0, e.b, b, en)
        bd.assert_untouched(e, src0, e.a)
        got = e.interior(e.b)[b:en].cpu().numpy()
        bd.assert_bitwise(got, want[tall + b:tall + en], f"planes [{b}, {en}) after {steps} sweeps")


def setup_single(gpu, dtype, shape, kernel, size, seed, r=1, halo=0, flags=0):
    """Engine, oracle problem, dense start (grid b holds a different field) and
    the depth by which the oracle's grid is taller per side (halo layouts)."""
    e = make_engine(gpu, 3, dtype, shape, r, "naive", kernel, size, halo=halo, flags=flags)
    start = bd.poison_and_fill(e, seed, shape == "star", same_ghosts=False)
    tall = int(e.layout.zghost) if flags else 0
    nx, ny, nz = size
    p = ob.problem(3, dtype, shape, r, "naive", nx, ny, nz + 2 * tall)
    key = (dtype, shape, r, size, seed, tall)
    return e, p, start, tall, key


def multi_tile(dtype, size):
    w, h = REGION3[dtype]
    return size[0] > w and size[1] > h


# ------------------------------------------------------------ single launches
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("steps", [3, 4, 5])
@pytest.mark.parametrize("zchunk", [0, 7])
@pytest.mark.parametrize("size", [(131, 61, 29), (64, 7, 9)])
def test_tkstrip_single_launch(gpu, monkeypatch, dtype, steps, zchunk, size):
    """tkstrip_7pt (stencil_sweepk, K = 3..5): several ragged tiles and
    z-chunks, and a grid shorter than one region; full range and a sub-range."""
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", str(zchunk))
    e, p, start, tall, key = setup_single(gpu, dtype, "star", "temporalk", size, 101)
    nz = size[2]
    ranges = [(0, nz), subrange(nz, zchunk)]
    for b, en in ranges:
        geo = e.sweepk_geometry(steps, b, en)
        chunks = -(-(en - b) // zchunk) if zchunk else 1
        if zchunk:
            assert geo["zchunk"] == zchunk and geo["workgroups"] % chunks == 0, geo
        if multi_tile(dtype, size):
            assert geo["workgroups"] // chunks > 1, geo  # more than one tile
            assert not zchunk or chunks > 1
        else:
            assert geo["workgroups"] >= 1, geo
    check_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, ranges, key)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("steps", [4, 5])
@pytest.mark.parametrize("fast", [0, 1, 4, 5])
def test_tkstrip_interior_tiles(gpu, monkeypatch, dtype, steps, fast):
    """Tiles that touch no x or y ghost and take the interior fast paths
    (STENCIL_TK_FAST bits) beside edge tiles that must not: a fast path on a
    region that still holds a ghost cell would compute that ghost at the
    intermediate stages instead of keeping it."""
    monkeypatch.setenv("STENCIL_TK_FAST", str(fast))
    size = (300, 250, 40)
    w, h = REGION3[dtype]
    assert size[0] > 2 * w and size[1] > 2 * h  # at least 3 x 3 tiles: one with no edge
    e, p, start, tall, key = setup_single(gpu, dtype, "star", "temporalk", size, 102)
    ranges = [(0, 40), subrange(40)]
    assert e.sweepk_geometry(steps)["workgroups"] >= 9
    check_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, ranges, key)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape,steps", [("star", 3), ("star", 4), ("star", 5), ("box", 2), ("box", 3), ("box", 4)])
@pytest.mark.parametrize("flags", [0, HALO])
def test_sweepk_halo_layouts(gpu, dtype, shape, steps, flags):
    """Grids with K ghost planes per z side.  HALO_LO|HALO_HI: the K planes
    are a neighbour's interior, advanced in registers and never stored; the
    oracle sweeps a grid taller by K planes per side and the middle nz planes
    are compared.  Without the flags only the first ghost plane is read: the
    deeper ones hold NaN."""
    size = (131, 61, 29)
    assert multi_tile(dtype, size)
    e, p, start, tall, key = setup_single(gpu, dtype, shape, "auto", size, 103, halo=steps, flags=flags)
    assert int(e.layout.zghost) == steps and tall == (steps if flags else 0)
    if shape == "star":
        assert e.sweepk_geometry(steps)["workgroups"] > 1
    check_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, [(0, 29), subrange(29)], key,
                 tall=tall)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape,steps", [("star", 3), ("star", 4), ("star", 5), ("box", 2), ("box", 3), ("box", 4)])
@pytest.mark.parametrize("flags", [0, HALO])
@pytest.mark.parametrize("zchunk", [0, 9])
def test_sweepk_signal_launch(gpu, monkeypatch, dtype, shape, steps, flags, zchunk):
    """stencil_sweepk_signal (the last z-chunk marches down, faces first):
    what stencil_sweepk gives, over the full range and an interior sub-range
    (its faces are then the sub-range's first and last K planes), and after a
    normal wait both face counters read the returned adds per face (one per
    tile), the timeout flag 0."""
    monkeypatch.setenv("STENCIL_TK_ZCHUNK" if shape == "star" else "STENCIL_BOXK_ZCHUNK", str(zchunk))
    size = (131, 61, 29)
    e, p, start, tall, key = setup_single(gpu, dtype, shape, "auto", size, 103, halo=steps if flags else 0,
                                          flags=flags)
    sig = torch.zeros(4, dtype=torch.int32, device=e.a.device)
    seen = []

    def launch(s, d, b, en):
        sig.zero_()
        nsig = e.sweepk_signal(s, d, b, en, steps, sig)
        e.wait_counters(sig, nsig, nsig)
        torch.cuda.synchronize()
        seen.append((nsig, sig.tolist()))

    check_launch(e, launch, p, start, steps, [(0, 29), subrange(29, zchunk)], key, tall=tall)
    assert len(seen) == 2
    for nsig, counters in seen:
        assert nsig > 1, nsig  # one add per tile and face: more than one tile
        assert counters == [nsig, nsig, 0, 0], counters


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("steps", [1, 2, 3, 4])
@pytest.mark.parametrize("size", [(131, 61, 29), (7, 5, 3), (250, 119, 12)])
@pytest.mark.parametrize("zchunk", [0, 5])
def test_box_strip_single_launch(gpu, monkeypatch, dtype, steps, size, zchunk):
    """The 27-point box through AUTO's launches (box27_strip and its K = 1
    instance): ragged tiles, one tiny tile, forced short z-chunks.  The box
    reads ring edges and corners, so those hold values too.

    Regime: the library has no geometry query for the box; the one tile count
    it reports is the face-signalled launch's adds per face (one per tile), so
    that launch is asked about the same grid under the same knobs: more than
    one tile at the two large shapes, exactly one at (7, 5, 3).  Whether
    STENCIL_BOXK_ZCHUNK was honoured is not observable from outside; the
    forced chunk is shorter than nz at the large shapes, so there it cuts
    each tile's march into several chunks if it is read at all (it is a knob
    of the debug library, which the engine is checked to have loaded)."""
    monkeypatch.setenv("STENCIL_BOXK_ZCHUNK", str(zchunk))
    e, p, start, tall, key = setup_single(gpu, dtype, "box", "auto", size, 104)
    assert e.lib.stencil_debug_knobs() == 1
    nz = size[2]
    small = size == (7, 5, 3)
    assert small or not zchunk or nz > 2 * zchunk  # at least three forced chunks
    check_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, [(0, nz), subrange(nz, zchunk)],
                 key)
    tiles = box_tiles(e, 2)
    assert (tiles == 1) if small else (tiles > 1), tiles


def box_tiles(e, steps):
    """Tiles of the box's face-signalled launch over the whole grid (its adds
    per face), from a launch a -> b whose counters are waited for.  A face is
    the range's first / last `steps` planes, so the grid must have at least
    `steps` planes: on a shorter range a face counter never reaches its
    target and the wait runs into its timeout."""
    assert int(e.prob.nz) >= steps
    sig = torch.zeros(4, dtype=torch.int32, device=e.a.device)
    nsig = e.sweepk_signal(e.a, e.b, 0, int(e.prob.nz), steps, sig)
    e.wait_counters(sig, nsig, nsig)
    torch.cuda.synchronize()
    assert sig.tolist() == [nsig, nsig, 0, 0]
    return nsig


# "temporalk-rows": the family's interleaved-row layout (kernels_temporalk.hip, STENCIL_TK_STRIP=0)
FAMILIES = [("star", "direct", 1), ("star", "zmarch", 1), ("star", "temporal2", 2), ("star", "temporalk", 3),
            ("star", "temporalk-rows", 3), ("star", "temporalk-rows", 4),
            ("box", "direct", 1), ("box", "zmarch", 1), ("box", "temporal2", 2)]


# Output tile (x, y) of each forced family's launch, from its source: sweep_direct's block is kBX x kBY =
# 64 x 4 cells (kernels_direct.hip); zmarch7's tile is 64 V x 4 RY with V = 16 B / sizeof(T) and RY <= 4
# (kernels_zmarch.hip ZTile, launch_zmarch); temporal2's default is T2Tile<T, V, 2, 16>: (64 V - 2 V) x 28
# (kernels_temporal.hip).  The library reports no launch geometry for these, so the tile counts below are
# arithmetic on those constants; what the library does report is asserted beside them: the family
# stencil_plan resolves the engine to, the strip kernel's geometry, and that there is none under
# STENCIL_TK_STRIP=0 (the interleaved-row kernel has no dry mode, api.hip stencil_sweepk_geometry).
def family_tile(kernel, dtype):
    v = 4 if dtype == "fp32" else 2
    return {"direct": (64, 4), "zmarch": (64 * v, 16), "temporal2": (62 * v, 28)}[kernel]


def tiles_of(size, tile):
    return -(-size[0] // tile[0]), -(-size[1] // tile[1])


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape,kernel,steps", FAMILIES)
@pytest.mark.parametrize("size", [(65, 17, 3), (130, 37, 29)])
def test_forced_families_single_launch(gpu, monkeypatch, dtype, shape, kernel, steps, size):
    """The forced kernel families (direct, zmarch, temporal2, temporalk in
    both its layouts), one launch each of as many sweeps as the family fuses.
    (130, 37, 29): several tiles with a ragged last one in every family;
    (65, 17, 3): one cell past a 64-wide block, one row past 16, fewer planes
    than any pipeline fill."""
    rows = kernel == "temporalk-rows"
    if rows:
        monkeypatch.setenv("STENCIL_TK_STRIP", "0")
        kernel = "temporalk"
    e, p, start, tall, key = setup_single(gpu, dtype, shape, kernel, size, 105)
    nz = size[2]
    ranges = [(0, nz), subrange(nz)]
    # the family the library resolves this engine to
    assert e.plan(steps)[1] == _lib.KERNEL_NAMES[kernel]
    big = size == (130, 37, 29)
    if kernel == "temporalk":
        if rows:
            assert e.lib.stencil_debug_knobs() == 1  # the knob is read
            with pytest.raises(_lib.StencilError, match="not the strip kernel"):
                e.sweepk_geometry(steps)
        else:
            geo = e.sweepk_geometry(steps)
            assert geo["workgroups"] > 1 if big else geo["workgroups"] >= 1, geo
    elif shape == "star" or kernel == "direct":
        tx, ty = tiles_of(size, family_tile(kernel, dtype))
        assert size[0] % family_tile(kernel, dtype)[0] and size[1] % family_tile(kernel, dtype)[1]  # ragged
        if big:
            assert ty > 1 and tx * ty > 1, (tx, ty)
        if kernel == "direct":
            assert tx > 1 and ty > 1, (tx, ty)
    check_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, ranges, key)
    if shape == "box" and kernel != "direct":  # the box's z-march kernels: the library's own tile count
        tiles = box_tiles(e, 2)  # the face-signalled box launch of the same grid (kernels_boxk.hip)
        assert tiles > 1 if big else tiles >= 1, tiles


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape,r", [("star", 2), ("star", 3), ("box", 2)])
def test_direct_wider_stencils(gpu, dtype, shape, r):
    """sweep_direct for the 3D star r = 2, 3 and the box r = 2: a partial
    block in x (45 of 64 lanes), six blocks of 4 rows in y with a ragged last
    one, one plane per block in z."""
    size = (45, 23, 17)
    e, p, start, tall, key = setup_single(gpu, dtype, shape, "direct", size, 106, r=r)
    assert e.plan(1) == (1, _lib.KERNEL_DIRECT)  # the family the library resolves the engine to
    tx, ty = tiles_of(size, family_tile("direct", dtype))
    assert (tx, ty) == (1, 6) and size[0] % 64 and size[1] % 4
    check_launch(e, lambda s, d, b, en: e.sweep(s, d, b, en), p, start, 1, [(0, 17), subrange(17)], key)


# ----------------------------------------------------------------- whole jobs
def check_job(e, p, start, it, slow, key, threads=1, run=None):
    """stencil_iterate from grid a (both grids hold the same field): the final
    grid's interior is the oracle's, and over the whole allocation of BOTH
    grids nothing but interior cells changed."""
    want = oracle_interiors(key, p, start, it, slow, threads)
    a0, b0 = e.a.clone(), e.b.clone()
    fin = run() if run else e.iterate(it)[0]
    torch.cuda.synchronize()
    bd.assert_only_wrote(e, a0, e.a, 0, slow)
    bd.assert_only_wrote(e, b0, e.b, 0, slow)
    bd.assert_bitwise(e.interior(fin).cpu().numpy(), want, f"after {it} sweeps")


def setup_job(gpu, dims, dtype, shape, r, order, kernel, size, seed):
    e = make_engine(gpu, dims, dtype, shape, r, order, kernel, size)
    start = bd.poison_and_fill(e, seed, shape == "star")
    nx, ny, nz = size
    p = ob.problem(dims, dtype, shape, r, order, nx, ny, nz)
    return e, p, start, (dims, dtype, shape, r, order, size, seed)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("order", ["naive", "dma"])
@pytest.mark.parametrize("cfg", ["default", "92808"])
def test_2d_star_jobs(gpu, monkeypatch, dtype, r, order, cfg):
    """2D stars through AUTO (the register-strip regions for r <= 2, the LDS
    regions to r = 4, sweep_direct beyond), 23 sweeps over several ragged
    tiles: ghost rows and columns kept through every intermediate stage."""
    if cfg != "default":
        monkeypatch.setenv("STENCIL_TB2D_CFG", cfg)
    size = (301, 170, 1)
    assert size[0] > 2 * REGION2[0] and size[1] > 2 * REGION2[1]
    e, p, start, key = setup_job(gpu, 2, dtype, "star", r, order, "auto", size, 201)
    if r <= 4:
        assert e.plan(23)[0] < 23  # K-step launches, not single sweeps
    check_job(e, p, start, 23, 170, key)


@pytest.mark.parametrize("size", [(20, 9, 1), (64, 64, 1)])
@pytest.mark.parametrize("r,order", [(1, "naive"), (1, "dma"), (2, "naive"), (2, "dma"), (3, "naive"), (3, "dma"),
                                     (4, "naive"), (4, "dma")])
def test_2d_single_workgroup_jobs(gpu, size, r, order):
    """Grids one workgroup holds in LDS: the whole job is one launch."""
    for dtype in ("fp32", "fp64"):
        e, p, start, key = setup_job(gpu, 2, dtype, "star", r, order, "auto", size, 202)
        assert e.plan(7)[0] == 1
        check_job(e, p, start, 7, size[1], key)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("order", ["naive", "dma"])
def test_2d_persistent_jobs(gpu, dtype, r, order):
    """The persistent kernel: one cooperative launch for the whole job."""
    size = (64, 64, 1)
    e, p, start, key = setup_job(gpu, 2, dtype, "star", r, order, "persistent", size, 203)
    assert e.plan(12) == (1, _lib.KERNEL_PERSISTENT)
    check_job(e, p, start, 12, 64, key)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", ["star", "box"])
def test_3d_jobs(gpu, dtype, shape):
    """AUTO's 3D jobs: two K-step launches and a single sweep."""
    size = (131, 61, 29)
    assert multi_tile(dtype, size)
    e, p, start, key = setup_job(gpu, 3, dtype, shape, 1, "naive", "auto", size, 204)
    k = e.fuse_steps
    assert k >= 3 and e.plan(2 * k + 1)[0] == 3
    check_job(e, p, start, 2 * k + 1, 29, key)


PACKED_CANDIDATES = [(131, 61, 29), (200, 200, 200), (300, 200, 150), (512, 512, 96), (600, 100, 64), (64, 7, 90)]


@functools.lru_cache(maxsize=None)
def smallest_packed_shape(gpu, dtype):
    for size in sorted(PACKED_CANDIDATES, key=lambda s: s[0] * s[1] * s[2]):
        e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=gpu, allocate=False)
        if e.sweepk_geometry(e.fuse_steps)["packed"]:
            return size
    raise AssertionError("none of the candidate shapes takes the packed schedule")


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("pack", ["1", "2"])
def test_long_job_xcd_patch_tables(gpu, monkeypatch, dtype, pack):
    """A call of >= 256 sweeps launches the packed tables in XCD-patch order
    (DESIGN.md §5.2): 257 sweeps at the smallest shape the model packs.
    STENCIL_TK_PACK=1 keeps whichever of packed / equal chunks the first launch
    measures faster; 2 launches the model's choice, the packed tables, for
    certain."""
    monkeypatch.setenv("STENCIL_TK_PACK", pack)
    size = smallest_packed_shape(gpu, dtype)
    e, p, start, key = setup_job(gpu, 3, dtype, "star", 1, "naive", "auto", size, 205)
    assert e.sweepk_geometry(e.fuse_steps)["packed"]
    check_job(e, p, start, 257, size[2], key, threads=16)
    if pack == "2":
        assert e.sweepk_geometry(e.fuse_steps)["packed"]


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_short_job_forced_xcd_patch_tables(gpu, monkeypatch, dtype):
    """The same tables forced on a 9-sweep job (STENCIL_TK_PACK_XCD=-1)."""
    monkeypatch.setenv("STENCIL_TK_PACK", "2")
    monkeypatch.setenv("STENCIL_TK_PACK_XCD", "-1")
    size = smallest_packed_shape(gpu, dtype)
    e, p, start, key = setup_job(gpu, 3, dtype, "star", 1, "naive", "auto", size, 205)
    assert e.lib.stencil_debug_knobs() == 1 and e.sweepk_geometry(e.fuse_steps)["packed"]
    check_job(e, p, start, 9, size[2], key, threads=16)


@pytest.mark.parametrize("shape", ["star", "box"])
def test_prepare_writes_only_interior_of_b(gpu, shape):
    """stencil_prepare2 (schedule trials and settle launches a -> b): grid a's
    whole allocation is unchanged, grid b's ghosts, padding and tail are; the
    job that follows is the oracle's."""
    size = (200, 180, 96)
    e, p, start, key = setup_job(gpu, 3, "fp64", shape, 1, "naive", "auto", size, 206)
    a0, b0 = e.a.clone(), e.b.clone()
    ran = e.prepare()
    torch.cuda.synchronize()
    assert ran["launches"] >= 1
    bd.assert_untouched(e, a0, e.a, "grid a")
    bd.assert_only_wrote(e, b0, e.b, 0, 96)
    check_job(e, p, start, 2 * e.fuse_steps + 1, 96, key, threads=16)


def test_iterate_until_on_live_rings(gpu):
    """stencil_iterate_until with both job grids holding a varying ring (and
    NaN ring edges): the sweep count, the norm and the grid are the oracle's,
    so stencil_diff_norms sees interior cells only."""
    size = (67, 29, 11)
    nx, ny, nz = size
    check_every, cap = 7, 25
    e, p, start, key = setup_job(gpu, 3, "fp64", "star", 1, "naive", "auto", size, 207)
    norms = {}
    for n in (7, 14, 21, 25):
        d = oracle_interiors(key, p, start, n, nz) - oracle_interiors(key, p, start, n - 1, nz)
        norms[n] = float(np.abs(d).max())
    assert norms[21] < norms[14] < norms[7], norms  # a property of the field, from the oracle alone
    tol = 0.5 * (norms[14] + norms[21])
    for want_done, want_conv, t in ((21, True, tol), (25, False, 0.0)):
        bd.poison_and_fill(e, 207, True)
        a0, b0 = e.a.clone(), e.b.clone()
        res = e.iterate_until(t, cap, check_every=check_every, norm="max")
        torch.cuda.synchronize()
        assert (res.iterations, res.converged) == (want_done, want_conv)
        assert res.norm == norms[want_done]
        bd.assert_only_wrote(e, a0, e.a, 0, nz)
        bd.assert_only_wrote(e, b0, e.b, 0, nz)
        bd.assert_bitwise(e.interior(res.grid).cpu().numpy(), oracle_interiors(key, p, start, want_done, nz),
                          f"after {want_done} sweeps")


# ------------------------------------------------------------------ slab jobs
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("shape", ["star", "box"])
@pytest.mark.parametrize("nslabs", [1, 2, 3])
def test_slab_job_keeps_a_varying_ring(gpu, dtype, shape, nslabs):
    """SlabJob (device-copy halos, slabs sharing the GPU, two grids per slab):
    boundary and interior launches run side by side on disjoint plane ranges
    and the exchange copies whole planes, ghost rings included.  Uploaded
    poisoned-ring grid, 3K + 1 sweeps: the oracle's grid, ghosts included."""
    nx, ny, nz = 70, 45, 41
    p = ob.problem(3, dtype, shape, 1, "naive", nx, ny, nz)
    start = bd.ring_field((nz + 2, ny + 2, nx + 2), 1, 301, np.float64 if dtype == "fp64" else np.float32,
                          shape == "star")
    job = SlabJob(StencilSpec(dims=3, dtype=dtype, shape=shape), nx, ny, nz, devices=[gpu] * nslabs, exchange="copy")
    k = job.info(0)["sweeps_per_round"]
    assert k >= 3 and sum(job.info(i)["planes"] for i in range(nslabs)) == nz
    job.upload(start)
    bd.assert_bitwise(job.download(), start, "upload / download")
    job.run(3 * k + 1)
    bd.assert_bitwise(job.download(), bd.oracle_steps(p, start, 3 * k + 1, nz), f"after {3 * k + 1} sweeps")
    job.close()


@pytest.mark.parametrize("shape", ["star", "box"])
@pytest.mark.parametrize("exchange", ["copy", "rccl"])
def test_slab_job_periodic_ring_with_a_varying_ring(gpu, shape, exchange):
    """A periodic ring of one slab (its faces cross the exchange into its own
    halos): the middle third of three stacked copies swept by the oracle, for
    fewer sweeps than one copy has planes; each plane keeps its own x/y ring."""
    nx, ny, nz, sweeps = 64, 40, 30, 9
    start = bd.ring_field((nz + 2, ny + 2, nx + 2), 1, 302, np.float64, shape == "star")
    job = SlabJob(StencilSpec(dims=3, dtype="fp64", shape=shape), nx, ny, nz, devices=[gpu], exchange=exchange,
                  periodic=True)
    job.upload(start)
    job.run(sweeps)
    got = job.download()
    job.close()
    p3 = ob.problem(3, "fp64", shape, 1, "naive", nx, ny, 3 * nz)
    g3 = np.zeros((3 * nz + 2, ny + 2, nx + 2))
    g3[1:1 + 3 * nz] = np.concatenate([start[1:nz + 1]] * 3)
    want = bd.oracle_steps(p3, g3, sweeps, 3 * nz)
    bd.assert_bitwise(got[1:nz + 1], want[1 + nz:1 + 2 * nz], f"{exchange} ring after {sweeps} sweeps")


# -------------------------------------------------------------- reference ABI
@pytest.mark.parametrize("fn,order", [("stencil_iterate_dma", "dma"), ("stencil_iterate_dma_static_unroll", "naive"),
                                      ("stencil_iterate_dma_slave_pack", "dma"), ("stencil_iterate_rma", "dma")])
@pytest.mark.parametrize("n,r", [(64, 1), (96, 3)])
@pytest.mark.parametrize("it", [6, 7])
def test_reference_abi_with_a_varying_ring(gpu, fn, order, n, r, it):
    """The four reference entry points on host buffers with whole-grid reach
    (block_size n / 8) and an arbitrary ring in both buffers: the
    parity-selected buffer is the oracle's grid in that variant's order, and
    neither buffer's ghosts change.  (With whole-grid reach RMA synthesises no
    face: every ghost it uses is read from the host.)"""
    lib = _lib.load()
    bd.require_bounded(2, "fp32", "star", r, order)
    p = ob.problem(2, "fp32", "star", r, order, n, n)
    start = bd.ring_field((n + 2 * r, n + 2 * r), r, 401, np.float32, True)
    a, b = start.copy(), start.copy()

    def view(arr):
        return _lib.MatrixView(n + 2 * r, n + 2 * r, r, r, n + 2 * r, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    args = _lib.Arguments(n // 8, it, view(a), view(b))
    getattr(lib, fn)(ctypes.byref(args))
    assert lib.stencil_last_error() == 0, lib.stencil_last_error_message()
    bd.assert_bitwise(b if it % 2 else a, bd.oracle_steps(p, start, it, n), fn)
    ring = np.ones(start.shape, dtype=bool)
    ring[r:-r, r:-r] = False
    assert bd.same_bits(a[ring], start[ring]) and bd.same_bits(b[ring], start[ring])
