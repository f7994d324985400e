"""Relaxed launches on slab layouts (stencil_sweepk_relax_halo) and their
face-signalled forms (stencil_sweepk_signal_relax / _gated) on the GPU, against
tests/relax_ref.py.

The expectation is tests/test_gpu_source_halo.py's, with relaxed sweeps: a halo
side's K halo planes are a neighbour slab's planes, the launch advances them on
chip, each advanced cell taking the source of its own plane and the stage's
weight.  So the launch must equal relax_ref.sweeps on the dense grid EXTENDED
by K - 1 live planes per halo side, taken on the range.  Every comparison is
bit for bit.  Field and source give every cell its own value, every source cell
the definition never reads holds NaN and so does all padding (Case, from that
file); the weights are distinct and non-dyadic, so a stage that took another
stage's weight -- in particular in the down-marching chunk of a face-signalled
launch -- shows in every cell.
"""
import ctypes

import numpy as np
import pytest
import torch

from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, StencilSpec
from tests import boundary_data as bd
from tests import relax_ref as rr
from tests.test_gpu_source_halo import FLAGS, HI, LO, Case, ranges_of, seam_size, signal_tile

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "fp64")
W = (0.8, 1.7, 0.6, 1.25, 0.9)
# rows per strip of the face-signalled relaxed shapes (kernels_strip.hip RelaxSignalShape): the signalled
# source shapes', so signal_tile() serves both
RELAX_SIGNAL_ROWS = {3: 6, 4: 4}


class RelaxCase(Case):
    """Case whose expectation is `steps` relaxed sweeps with the weights W[:steps]."""

    def want(self, steps):
        full = rr.sweeps(self.p, self.u, self.g, steps, W[:steps])
        return full[self.off:self.off + self.nz, 1:-1, 1:-1]


def test_relax_signal_rows_are_the_signalled_source_rows():
    from tests.test_gpu_source_halo import SIGNAL_ROWS
    assert RELAX_SIGNAL_ROWS == SIGNAL_ROWS


# ------------------------------------------------------ stencil_sweepk_relax_halo
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("steps", (1, 2, 3, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_relax_halo_launch(gpu, dtype, steps, flags):
    nx, ny = seam_size(rr.tile(dtype, steps if steps >= 2 else rr.K_MAX))
    for nz in (2 * steps + 1, max(1, steps - 1)):  # the second: fewer planes than steps
        c = RelaxCase(gpu, dtype, nx, ny, nz, steps, flags, 500 + steps)
        for b, en in ranges_of(nz, steps):
            c.check(lambda b, en: c.e.sweepk_relax_halo(c.e.a, c.e.b, b, en, W[:steps]), steps, b, en,
                    f"{dtype} {steps} relaxed sweeps, flags {flags}, nz {nz}")


@pytest.mark.parametrize("steps", (2, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_relax_halo_interior_tile(gpu, dtype, steps):
    """3 x 3 tiles: the middle one runs the fp64 shapes' select-free segments,
    which must still give a halo side's advanced planes their source and weight."""
    tx, ty = rr.tile(dtype, steps)
    nz = 2 * steps + 3
    c = RelaxCase(gpu, dtype, 3 * tx, 3 * ty, nz, steps, LO | HI, 510)
    for b, en in ((0, nz), (0, steps), (nz - steps, nz)):
        c.check(lambda b, en: c.e.sweepk_relax_halo(c.e.a, c.e.b, b, en, W[:steps]), steps, b, en, f"{dtype} K={steps}")


@pytest.mark.parametrize("steps", (1, 2, 3, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_flags_it_is_sweepk_relax(gpu, dtype, steps):
    nx, ny = seam_size(rr.tile(dtype, rr.K_MAX))
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), nx, ny, 9, device=gpu)
    e.reset("random", 520)
    e.set_source(np.random.default_rng(521).uniform(-1, 1, (9, ny, nx)))
    ref = e.b.clone()
    e.sweepk_relax(e.a, ref, 0, 9, W[:steps])
    e.sweepk_relax_halo(e.a, e.b, 0, 9, W[:steps])
    torch.cuda.synchronize()
    assert torch.equal(bd.ibits(e.b), bd.ibits(ref))


def test_halo_shallower_than_the_steps(gpu):
    e = JacobiEngine(StencilSpec(dims=3, dtype="fp64", halo=3), 40, 30, 12, device=gpu, flags=LO | HI)
    e.reset("random", 1)
    e.source = torch.zeros_like(e.a)
    with pytest.raises(_lib.StencilError) as err:
        e.sweepk_relax_halo(e.a, e.b, 0, 12, W[:4])
    assert err.value.code == -1 and "halo" in str(err.value)
    e.sweepk_relax_halo(e.a, e.b, 0, 12, W[:3])
    torch.cuda.synchronize()
    # the single-grid entry keeps refusing halo layouts
    with pytest.raises(_lib.StencilError) as err:
        e.sweepk_relax(e.a, e.b, 0, 12, W[:3])
    assert err.value.code == -5 and "halo" in str(err.value)


# -------------------------------------------------- stencil_sweepk_signal_relax*
def signal_launch(c, steps, gated):
    """The launch under test; returns (adds per face, the counters after it)."""
    def run(b, en):
        sig = torch.zeros(4, dtype=torch.int32, device=c.e.device)
        if gated:
            sig[3] = 3  # the exchange-completion word has reached the launch's need: the gate is released
        n = c.e.sweepk_signal_relax(c.e.a, c.e.b, b, en, W[:steps], sig, gated=gated, gate_need=3)
        c.e.wait_counters(sig, n, n)
        torch.cuda.synchronize()
        return n, sig.cpu().numpy()
    return run


def check_signal(c, steps, ranges):
    e = c.e
    for b, en in ranges:
        halo = e.b.clone()
        e.b.copy_(c.b0)
        e.sweepk_relax_halo(e.a, e.b, b, en, W[:steps])
        torch.cuda.synchronize()
        halo.copy_(e.b)
        for gated in (False, True):
            n, sig = c.check(signal_launch(c, steps, gated), steps, b, en, f"{c.dtype} K={steps} signalled (gated {gated})")
            assert torch.equal(bd.ibits(e.b), bd.ibits(halo)), "not the halo launch's grid"
            tx, ty = signal_tile(c.dtype, steps)
            tiles = -(-int(e.prob.nx) // tx) * -(-int(e.prob.ny) // ty)
            assert n == tiles and sig[0] == n and sig[1] == n and sig[2] == 0, (n, tiles, sig)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("steps", (3, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_signalled_relax_launch(gpu, dtype, steps, flags):
    nx, ny = seam_size(signal_tile(dtype, steps))
    nz = 2 * steps + 1
    c = RelaxCase(gpu, dtype, nx, ny, nz, steps, flags, 530 + steps)
    check_signal(c, steps, [(0, nz), (0, steps), (nz - steps, nz), (1, nz - 1)])


@pytest.mark.parametrize("steps", (3, 4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_signalled_forced_z_chunks(gpu, monkeypatch, dtype, steps):
    """nz = 4K + 1 with STENCIL_TK_ZCHUNK = 2K (the debug library): every tile
    has an up-marching chunk of 2K + 1 planes and a down-marching one of 2K, and
    both must apply w[s - 1] at stage s; 2 x 2 + ragged tiles."""
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", str(2 * steps))
    tx, ty = signal_tile(dtype, steps)
    nz = 4 * steps + 1
    c = RelaxCase(gpu, dtype, 2 * tx + 9, 2 * ty + 5, nz, steps, LO | HI, 540 + steps)
    assert c.e.lib.stencil_debug_knobs() == 1
    check_signal(c, steps, [(0, nz), (1, nz - 2)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_signalled_many_chunks(gpu, monkeypatch, dtype):
    """Three chunks per tile and more: the face chunks are dispatched first, the middle ones march up."""
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", "9")
    tx, ty = signal_tile(dtype, 4)
    c = RelaxCase(gpu, dtype, tx + 7, ty + 3, 31, 4, LO | HI, 550)
    check_signal(c, 4, [(0, 31)])


def test_signalled_rejections(gpu):
    e = JacobiEngine(StencilSpec(dims=3, dtype="fp64", halo=4), 40, 30, 12, device=gpu, flags=LO | HI)
    e.reset("random", 2)
    e.source = torch.zeros_like(e.a)
    sig = torch.zeros(4, dtype=torch.int32, device=e.device)
    # short ranges, steps other than 3 and 4 (2 and 5 weights), a NaN and an infinite weight
    for b, en, w in ((0, 3, W[:4]), (5, 7, W[:3]), (0, 12, W[:2]), (0, 12, W[:5]), (0, 12, (0.8, float("nan"), 0.6)),
                     (0, 12, (0.8, 1.7, 0.6, float("inf")))):
        for gated in (False, True):
            with pytest.raises(_lib.StencilError) as err:
                e.sweepk_signal_relax(e.a, e.b, b, en, w, sig, gated=gated)
            assert err.value.code == -1
    with pytest.raises(_lib.StencilError) as err:
        e.sweepk_relax_halo(e.a, e.b, 0, 12, (0.8, float("nan")))
    assert err.value.code == -1 and "weight 1" in str(err.value)
    torch.cuda.synchronize()
    assert int(sig.abs().sum()) == 0
    n = ctypes.c_int32(0)
    lay = ctypes.byref(e.layout)
    a, b, s, c = (ctypes.c_void_p(t.data_ptr()) for t in (e.a, e.b, e.source, sig))
    w = (ctypes.c_double * 4)(*W[:4])
    f = e.lib.stencil_sweepk_signal_relax
    assert f(lay, a, b, s, 0, 12, 4, w, None, None, ctypes.byref(n), None) == -1      # NULL counters
    assert f(lay, a, b, None, 0, 12, 4, w, c, None, ctypes.byref(n), None) == -1      # NULL source
    assert f(lay, a, b, s, 0, 12, 4, None, c, None, ctypes.byref(n), None) == -1      # NULL weights
    assert "omegas" in e.lib.stencil_last_error_message().decode()
    assert e.lib.stencil_sweepk_signal_relax_gated(lay, a, b, s, 0, 12, 4, None, c, None, 0, None, ctypes.byref(n),
                                                   None) == -1
    assert e.lib.stencil_sweepk_relax_halo(lay, a, b, s, 0, 12, 4, None, None) == -1
    torch.cuda.synchronize()
    assert int(sig.abs().sum()) == 0
