"""Source launches on slab layouts (stencil_sweepk_source_halo) and their
face-signalled forms (stencil_sweepk_signal_source / _gated) on the GPU,
against tests/source_ref.py.

A halo side's K halo planes are a neighbour slab's planes: the launch advances
them on chip, each advanced cell taking the source of its own plane.  So the
expectation is source_ref.sweeps on the dense grid EXTENDED by K - 1 live
planes per halo side (plane -K / nz + K - 1 is that grid's ghost plane), taken
on the range.  Every comparison is bit for bit.  Field and source give every
cell its own value (tests/boundary_data.py), so a source plane taken from the
wrong z shows -- in particular in the down-marching chunk of a face-signalled
launch; every source cell the definition says is never used holds NaN, and so
does all padding.
"""
import ctypes

import numpy as np
import pytest
import torch

from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, StencilSpec
from tests import boundary_data as bd
from tests import source_ref as sr
from tests import special_values as sv

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "fp64")
NP = {"fp32": np.float32, "fp64": np.float64}
LO, HI = _lib.HALO_LO, _lib.HALO_HI
FLAGS = (LO, HI, LO | HI)
SENTINEL = -777.25
# rows per strip of the face-signalled source shapes (kernels_strip.hip SourceSignalShape), 8 waves each
SIGNAL_ROWS = {3: 6, 4: 4}


def signal_tile(dtype, k):
    v = 2 if dtype == "fp32" else 1
    return 64 * v - 2 * (-(-k // v)) * v, 8 * SIGNAL_ROWS[k] - 2 * k


def seam_size(tile):
    """Two tiles per axis with a ragged end, an odd width."""
    tx, ty = tile
    nx = tx + 11 if (tx + 11) % 2 else tx + 12
    return nx, ty + 5


def test_signal_tiles():
    assert signal_tile("fp64", 4) == (56, 24) and signal_tile("fp32", 4) == (120, 24)
    assert signal_tile("fp64", 3) == (58, 42) and signal_tile("fp32", 3) == (120, 42)


class Case:
    """An engine on a layout with `flags` and halo = K whose grid a, source grid
    and their dense extended images hold boundary_data's fields; grid b holds
    the sentinel in its interior.  Everything else in the three allocations is
    the poison NaN."""

    def __init__(self, gpu, dtype, nx, ny, nz, k, flags, seed):
        bd.require_bounded(3, dtype, "star", 1, "naive")
        self.k, self.nz, self.dtype = k, nz, dtype
        self.e = e = JacobiEngine(StencilSpec(dims=3, dtype=dtype, halo=k), nx, ny, nz, device=gpu, flags=flags)
        assert int(e.layout.zghost) == k
        lo, hi = bool(flags & LO), bool(flags & HI)
        self.off = k if lo else 1                     # extended index of slab plane 0
        nze = nz + (k - 1) * (lo + hi)
        self.p = sr.problem(dtype, nx, ny, nze)
        self.u = bd.ring_field((nze + 2, ny + 2, nx + 2), 1, seed, NP[dtype], star=True)
        self.g = np.full_like(self.u, np.nan)
        self.g[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed + 7).uniform(-1, 1, (nze, ny, nx)).astype(NP[dtype])
        e.source = torch.empty_like(e.a)
        first = (k - self.off)                         # the device view's plane that holds extended plane 0
        for grid, dense in ((e.a, self.u), (e.b, None), (e.source, self.g)):
            bd.ibits(grid).fill_(bd.nan_pattern(grid.dtype))
            if dense is not None:
                bd.box_view(e, grid, k)[first:first + nze + 2].copy_(torch.from_numpy(dense))
        e.interior(e.b).fill_(SENTINEL)
        torch.cuda.synchronize()
        self.b0 = e.b.clone()

    def want(self, steps):
        full = sr.sweeps(self.p, self.u, self.g, steps)
        return full[self.off:self.off + self.nz, 1:-1, 1:-1]

    def check(self, launch, steps, b, en, what):
        """One launch a -> b over [b, en): the extended grid's planes there, the
        sentinel on the slab's other planes, nothing else of b written, a and
        the source grid untouched."""
        e = self.e
        a0, s0 = e.a.clone(), e.source.clone()
        e.b.copy_(self.b0)
        out = launch(b, en)
        torch.cuda.synchronize()
        got = e.interior(e.b).cpu().numpy()
        sv.assert_same_values(got[b:en], self.want(steps)[b:en], f"{what} [{b}, {en})")
        assert (np.delete(got, np.s_[b:en], axis=0) == NP[self.dtype](SENTINEL)).all(), "a plane outside the range was written"
        bd.assert_only_wrote(e, self.b0, e.b, b, en)
        bd.assert_untouched(e, a0, e.a, "input grid")
        bd.assert_untouched(e, s0, e.source, "source grid")
        return out


def ranges_of(nz, k):
    r = [(0, nz), (0, min(k, nz)), (max(0, nz - k), nz), (k, nz - k)]
    return sorted({(b, en) for b, en in r if 0 <= b < en <= nz})


# ------------------------------------------------------ stencil_sweepk_source_halo
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("steps", (1, 2, 3, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_source_halo_launch(gpu, dtype, steps, flags):
    nx, ny = seam_size(sr.tile(dtype, steps if steps >= 2 else sr.K_MAX))
    for nz in (2 * steps + 1, max(1, steps - 1)):  # the second: fewer planes than steps
        c = Case(gpu, dtype, nx, ny, nz, steps, flags, 400 + steps)
        for b, en in ranges_of(nz, steps):
            c.check(lambda b, en: c.e.sweepk_source_halo(c.e.a, c.e.b, b, en, steps), steps, b, en,
                    f"{dtype} {steps} source sweeps, flags {flags}, nz {nz}")


@pytest.mark.parametrize("steps", (2, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_source_halo_interior_tile(gpu, dtype, steps):
    """3 x 3 tiles: the middle one runs the fp64 shapes' select-free segments,
    which must still give a halo side's advanced planes their source."""
    tx, ty = sr.tile(dtype, steps)
    nz = 2 * steps + 3
    c = Case(gpu, dtype, 3 * tx, 3 * ty, nz, steps, LO | HI, 410)
    for b, en in ((0, nz), (0, steps), (nz - steps, nz)):
        c.check(lambda b, en: c.e.sweepk_source_halo(c.e.a, c.e.b, b, en, steps), steps, b, en, f"{dtype} K={steps}")


@pytest.mark.parametrize("steps", (1, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_flags_it_is_sweepk_source(gpu, dtype, steps):
    nx, ny = seam_size(sr.tile(dtype, sr.K_MAX))
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), nx, ny, 9, device=gpu)
    e.reset("random", 420)
    e.set_source(np.random.default_rng(421).uniform(-1, 1, (9, ny, nx)))
    ref = e.b.clone()
    e.sweepk_source(e.a, ref, 0, 9, steps)
    e.sweepk_source_halo(e.a, e.b, 0, 9, steps)
    torch.cuda.synchronize()
    assert torch.equal(bd.ibits(e.b), bd.ibits(ref))


def test_halo_shallower_than_the_steps(gpu):
    e = JacobiEngine(StencilSpec(dims=3, dtype="fp64", halo=3), 40, 30, 12, device=gpu, flags=LO | HI)
    e.reset("random", 1)
    e.source = torch.zeros_like(e.a)
    with pytest.raises(_lib.StencilError) as err:
        e.sweepk_source_halo(e.a, e.b, 0, 12, 4)
    assert err.value.code == -1 and "halo" in str(err.value)
    e.sweepk_source_halo(e.a, e.b, 0, 12, 3)
    torch.cuda.synchronize()


# ------------------------------------------------- stencil_sweepk_signal_source*
def signal_launch(c, steps, gated):
    """The launch under test; returns (adds per face, the counters after it)."""
    def run(b, en):
        sig = torch.zeros(4, dtype=torch.int32, device=c.e.device)
        if gated:
            sig[3] = 3  # the exchange-completion word has reached the launch's need: the gate is released
        n = c.e.sweepk_signal_source(c.e.a, c.e.b, b, en, steps, sig, gated=gated, gate_need=3)
        c.e.wait_counters(sig, n, n)
        torch.cuda.synchronize()
        return n, sig.cpu().numpy()
    return run


def check_signal(c, steps, ranges):
    e = c.e
    for b, en in ranges:
        halo = e.b.clone()
        e.b.copy_(c.b0)
        e.sweepk_source_halo(e.a, e.b, b, en, steps)
        torch.cuda.synchronize()
        halo.copy_(e.b)
        for gated in (False, True):
            n, sig = c.check(signal_launch(c, steps, gated), steps, b, en, f"{c.dtype} K={steps} signalled (gated {gated})")
            assert torch.equal(bd.ibits(e.b), bd.ibits(halo)), "not the halo launch's grid"
            tiles = -(-int(e.prob.nx) // signal_tile(c.dtype, steps)[0]) * -(-int(e.prob.ny) // signal_tile(c.dtype, steps)[1])
            assert n == tiles and sig[0] == n and sig[1] == n and sig[2] == 0, (n, tiles, sig)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("steps", (3, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_signalled_source_launch(gpu, dtype, steps, flags):
    nx, ny = seam_size(signal_tile(dtype, steps))
    nz = 2 * steps + 1
    c = Case(gpu, dtype, nx, ny, nz, steps, flags, 430 + steps)
    check_signal(c, steps, [(0, nz), (0, steps), (nz - steps, nz), (1, nz - 1)])


@pytest.mark.parametrize("steps", (3, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_signalled_forced_z_chunks(gpu, monkeypatch, dtype, steps):
    """nz = 4K + 1 with STENCIL_TK_ZCHUNK = 2K (the debug library): every tile
    has an up-marching chunk of 2K + 1 planes and a down-marching one of 2K, so
    the source ring is walked both ways; 3 x 3 tiles, the middle one inside the
    grid (the fp64 shapes' select-free segments, both marches)."""
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", str(2 * steps))
    tx, ty = signal_tile(dtype, steps)
    nz = 4 * steps + 1
    c = Case(gpu, dtype, 2 * tx + 9, 2 * ty + 5, nz, steps, LO | HI, 440 + steps)
    assert c.e.lib.stencil_debug_knobs() == 1
    check_signal(c, steps, [(0, nz), (1, nz - 2)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_signalled_many_chunks(gpu, monkeypatch, dtype):
    """Three chunks per tile and more: the face chunks are dispatched first, the middle ones march up."""
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", "9")
    tx, ty = signal_tile(dtype, 4)
    c = Case(gpu, dtype, tx + 7, ty + 3, 31, 4, LO | HI, 450)
    check_signal(c, 4, [(0, 31)])


def test_signalled_rejections(gpu):
    e = JacobiEngine(StencilSpec(dims=3, dtype="fp64", halo=4), 40, 30, 12, device=gpu, flags=LO | HI)
    e.reset("random", 2)
    e.source = torch.zeros_like(e.a)
    sig = torch.zeros(4, dtype=torch.int32, device=e.device)
    for args in ((0, 3, 4), (5, 7, 3), (0, 12, 2), (0, 12, 5)):  # short ranges, steps other than 3 and 4
        for gated in (False, True):
            with pytest.raises(_lib.StencilError) as err:
                e.sweepk_signal_source(e.a, e.b, *args, sig, gated=gated)
            assert err.value.code == -1
    torch.cuda.synchronize()
    assert int(sig.abs().sum()) == 0
    n = ctypes.c_int32(0)
    lay = ctypes.byref(e.layout)
    a, b, s = (ctypes.c_void_p(t.data_ptr()) for t in (e.a, e.b, e.source))
    assert e.lib.stencil_sweepk_signal_source(lay, a, b, s, 0, 12, 4, None, None, ctypes.byref(n), None) == -1
    assert e.lib.stencil_sweepk_signal_source(lay, a, b, None, 0, 12, 4, ctypes.c_void_p(sig.data_ptr()), None,
                                              ctypes.byref(n), None) == -1
