"""The packed z-chunk tables of the fp64 K = 4 strip's sliver mode
(kernels_strip.hip, exported as stencil_sliver_table) on the CPU: the last
tile column, at most 8 columns wide, runs as sliver workgroups of four tile
rows each.  Every (tile, plane) of the range -- the four tile rows of a sliver
workgroup counted one by one -- lies in exactly one table entry, in the
tile-major order and in XCD patches.  No GPU: the tables are host code."""
import ctypes
import math

import pytest

from stencil_amd import _lib

TX, TY, K, SLOTS = 56, 48, 4, 256  # the fp64 K = 4 strip's output tile; one workgroup per CU


def sliver_table(nx, ny, nz, lc, w, slots=SLOTS):
    lib = _lib.load()
    geo = (ctypes.c_int64 * 4)()
    n = ctypes.c_int64(0)
    assert lib.stencil_sliver_table(nx, ny, nz, slots, lc, w, geo, None, 0, ctypes.byref(n)) == 0
    buf = (ctypes.c_int32 * (3 * max(1, n.value)))()
    assert lib.stencil_sliver_table(nx, ny, nz, slots, lc, w, geo, buf, n.value, ctypes.byref(n)) == 0
    return list(geo), [tuple(buf[3 * i:3 * i + 3]) for i in range(n.value)]


def model_workgroups(main, tiles, nz, lc):
    """pack_search's grid: chunks of lc planes for the main tiles, of
    ceil(lc / 2) for the sliver workgroups."""
    return main * math.ceil(nz / lc) + (tiles - main) * math.ceil(nz / math.ceil(lc / 2))


def test_model_at_c2():
    """512^3: 102 schedule tiles.  The model's table: chunks of 222 planes for
    the 99 main tiles ({222, 222, 68}: 230 plane steps against the 110-tile
    grid's 240), of 111 for the 3 sliver workgroups."""
    (gx, gy, main, tiles), tab = sliver_table(512, 512, 512, 0, 0)
    assert (gx, gy, main, tiles) == (10, 11, 99, 102)
    assert len(tab) == 99 * 3 + 3 * 5
    assert sorted({n for t, _, n in tab if t < main}) == [68, 222]
    assert sorted({n for t, _, n in tab if t >= main}) == [68, 111]
    # longest first: the main tiles' full chunks lead the table, and fit the slots at once
    assert all(t < main and n == 222 for t, _, n in tab[:198]) and 198 <= SLOTS


# chunk lengths: the model's own (0) and forced ones, each leaving a short last chunk; 230 planes at 512^3
# are the chunks of the 110-tile grid's table
@pytest.mark.parametrize("w", [0, -1, 2, 5], ids=["tile-major", "patches-auto", "patches-2", "patches-5"])
@pytest.mark.parametrize("shape,lc", [((512, 512, 512), 0), ((512, 512, 512), 230), ((64, 100, 9), 4),
                                      ((120, 200, 23), 5), ((57, 48, 5), 2), ((120, 200, 23), 23), ((64, 100, 9), 0)])
def test_every_tile_plane_once(shape, lc, w):
    nx, ny, nz = shape
    (gx, gy, main, tiles), tab = sliver_table(nx, ny, nz, lc, w)
    assert (gx, gy) == (math.ceil(nx / TX), math.ceil(ny / TY))
    assert main == (gx - 1) * gy and tiles == main + math.ceil(gy / 4)
    if shape == (512, 512, 512):
        assert (gx, gy, main, tiles) == (10, 11, 99, 102)
    assert tab, "sliver mode always has a table: the first launch's trial settles packed against equal chunks"
    chunk = lc or max(n for _, _, n in tab)
    assert len(tab) == model_workgroups(main, tiles, nz, chunk)
    seen = {}
    for t, z, n in tab:
        assert 0 <= t < tiles and n >= 1 and 0 <= z and z + n <= nz, (t, z, n)
        # the (tile column, tile row) pairs the entry covers
        if t < main:
            cells = [(t % (gx - 1), t // (gx - 1))]
        else:
            cells = [(gx - 1, by) for by in range(4 * (t - main), min(gy, 4 * (t - main) + 4))]
            assert cells, "a sliver workgroup holds at least one tile row"
        for c in cells:
            for p in range(z, z + n):
                assert (c, p) not in seen, (c, p)
                seen[(c, p)] = t
    assert len(seen) == gx * gy * nz
    # the same lengths at the same positions in every order: the same makespan
    _, base = sliver_table(nx, ny, nz, lc, 0)
    assert [(z, n) for _, z, n in tab] == [(z, n) for _, z, n in base]
    assert sorted(tab) == sorted(base)


def test_patches_keep_sliver_entries_behind_the_main_tiles():
    """In every generation (same first plane and length) of the patch order the
    sliver workgroups follow the main tiles, in their own order: the patch
    order deals its tiles to XCD 0's table positions (i % 8 == 0), then XCD
    1's, ..., so the sliver workgroups are the last the last XCD takes."""
    (gx, gy, main, tiles), tab = sliver_table(512, 512, 512, 230, -1)
    assert len(tab) == 312
    gens = {}
    for i, (t, z, n) in enumerate(tab):
        gens.setdefault((z, n), []).append((i % 8, i, t))
    assert (460, 52) in gens  # the last chunk: main tiles and sliver workgroups in one generation
    for g in gens.values():
        dealt = [t for _, _, t in sorted(g)]
        mains = [t for t in dealt if t < main]
        assert sorted(mains) in ([], list(range(main)))
        assert dealt[len(mains):] in ([], list(range(main, tiles)))


@pytest.mark.parametrize("nx,why", [(2048, "32 columns left"), (56, "one tile column"), (121, "9 columns left")])
def test_mode_off(nx, why):
    (gx, gy, main, tiles), tab = sliver_table(nx, 200, 64, 16, 0)
    assert (main, tiles) == (0, 0) and tab == [], why


def test_mode_off_beyond_the_packed_regime():
    """More than 2 tiles per workgroup slot: equal chunks fill the rounds, no sliver mode."""
    (gx, gy, main, tiles), tab = sliver_table(512, 512, 64, 16, 0, slots=54)
    assert gx * gy == 110 and (main, tiles) == (0, 0) and tab == []


def test_mode_off_where_no_table_can_exist():
    """The mode runs only with its packed table, whose full chunks must all be
    resident at once: more schedule tiles than slots leave no such table, so the
    mode is off -- 512 x 1536 (10 x 32 tiles: 288 + 8 = 296 on 256 slots, inside
    the packed regime of 2 tiles per slot), and 512^2 on 101 slots."""
    (gx, gy, main, tiles), tab = sliver_table(512, 1536, 512, 0, 0)
    assert (gx, gy) == (10, 32) and gx * gy <= 2 * SLOTS and (main, tiles) == (0, 0) and tab == []
    (gx, gy, main, tiles), tab = sliver_table(512, 512, 64, 0, 0, slots=101)
    assert (main, tiles) == (0, 0) and tab == []
    (gx, gy, main, tiles), tab = sliver_table(512, 512, 64, 0, 0, slots=102)
    assert (main, tiles) == (99, 102) and tab


@pytest.mark.parametrize("nx,ny,nz", [(512, 512, 512), (512, 1200, 64), (64, 100, 9), (120, 200, 23), (57, 48, 8),
                                      (4096, 96, 300), (64, 48, 600)])
def test_mode_on_means_a_table(nx, ny, nz):
    """Wherever the geometry allows the mode and the range is at least one
    pipeline fill (2K planes) long, the model has a table for it.  (Shorter
    ranges have none, here as on the plain grid: the launch then runs the plain
    grid, tests/test_gpu_sliver.py.)"""
    (gx, gy, main, tiles), tab = sliver_table(nx, ny, nz, 0, 0)
    assert tiles > main > 0 and tiles <= SLOTS and tab
    (_, _, _, tiles), tab = sliver_table(nx, ny, 2 * K - 1, 0, 0)
    assert tiles > 0 and tab == []


def test_invalid_arguments():
    lib = _lib.load()
    n = ctypes.c_int64(0)
    for args in [(0, 10, 8, 256, 0, 0), (10, 0, 8, 256, 0, 0), (10, 10, 0, 256, 0, 0), (10, 10, 8, 0, 0, 0),
                 (10, 10, 8, 256, -1, 0), (10, 10, 8, 256, 0, -2)]:
        assert lib.stencil_sliver_table(*args, None, None, 0, ctypes.byref(n)) != 0
        assert b"sliver table" in lib.stencil_last_error_message()
