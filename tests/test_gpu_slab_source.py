"""Source terms in slab jobs on the GPU (stencil_slab_set_source, run_source,
run_until_source, source_round_form; SlabJob's methods): bit for bit the
single-grid source job (JacobiEngine.iterate_source / iterate_until_source) or
tests/source_ref.py.  No tolerances.

Fields and sources give every cell its own value, varying by plane and by row
(tests/boundary_data.py); the source array's ghost cells hold NaN.
"""
import functools
import struct

import numpy as np
import pytest
import torch

from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, SlabJob, StencilSpec
from tests import boundary_data as bd
from tests import source_ref as sr

pytestmark = pytest.mark.gpu

NP = {"fp32": np.float32, "fp64": np.float64}
KS = sr.K_MAX
SIZE = (70, 45, 41)


def bits(x):
    return struct.pack("<d", x)


@functools.lru_cache(maxsize=None)
def fields(dtype, size, seed=3):
    nx, ny, nz = size
    u = bd.ring_field((nz + 2, ny + 2, nx + 2), 1, seed, NP[dtype], star=True)
    g = np.full_like(u, np.nan)
    g[1:-1, 1:-1, 1:-1] = (0.01 * np.random.default_rng(seed + 7).standard_normal((nz, ny, nx))).astype(NP[dtype])
    u.setflags(write=False)
    g.setflags(write=False)
    return u, g


def single_engine(gpu, dtype, size, u, g):
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=gpu)
    for grid in (e.a, e.b):
        grid.zero_()
        bd.box_view(e, grid).copy_(torch.from_numpy(np.array(u)))
    e.set_source(np.array(np.asarray(g)[1:-1, 1:-1, 1:-1]))
    return e


def advance(e, steps):
    """steps = [("source" | "plain", n), ...] on the engine's grids, a holding the result."""
    for kind, n in steps:
        fin, _ = e.iterate_source(n) if kind == "source" else e.iterate(n)
        if fin is e.b:
            e.a, e.b = e.b, e.a
    return e.a


@functools.lru_cache(maxsize=None)
def single_grid(gpu, dtype, size, steps):
    """The single-grid job's final grid (dense) and plane sums, computed once."""
    u, g = fields(dtype, size)
    e = single_engine(gpu, dtype, size, u, g)
    fin = advance(e, steps)
    out = bd.dense_of(e, fin)
    out.setflags(write=False)
    return out, e.plane_sums(fin)


def make_job(gpu, dtype, size, world, **kw):
    kw.setdefault("exchange", "copy")
    job = SlabJob(StencilSpec(dims=3, dtype=dtype), *size, [gpu] * world, **kw)
    u, g = fields(dtype, size)
    job.upload(np.asarray(u))
    job.set_source(np.asarray(g))
    return job


def inner(a):
    return np.asarray(a)[1:-1, 1:-1, 1:-1]


# ------------------------------------------------------ slabs sharing the GPU
@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_slabs_sharing_the_gpu(gpu, dtype, world):
    sweeps = 3 * KS + 1
    want, sums = single_grid(gpu, dtype, SIZE, (("source", sweeps),))
    job = make_job(gpu, dtype, SIZE, world)
    try:
        assert job.info(0)["sweeps_per_round"] == 4
        assert job.source_plan(sweeps) == {"rounds": 4, "steps": KS}
        assert job.source_round_form() == (1 if world == 1 else 0)  # slabs sharing a GPU: boundary + interior
        ms = job.run_source(sweeps)
        assert ms >= 0
        bd.assert_bitwise(inner(job.download()), inner(want), f"{dtype} world {world}")
        assert np.array_equal(job.plane_sums(), sums)
    finally:
        job.close()


def test_against_the_helper(gpu):
    size = (37, 19, 17)
    u, g = fields("fp64", size, seed=11)
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), *size, [gpu] * 2, exchange="copy")
    try:
        job.upload(np.asarray(u))
        job.set_source(inner(g))  # the interior alone
        job.run_source(2 * KS + 3)
        got = job.download()
        want = sr.sweeps(sr.problem("fp64", *size), np.asarray(u), np.asarray(g), 2 * KS + 3)
        bd.assert_bitwise(inner(got), inner(want))
        bd.assert_bitwise(got[0], np.asarray(u)[0])  # the global ghost planes as uploaded
        # a second set_source replaces the values
        g2 = np.asarray(g).copy()
        g2[1:-1, 1:-1, 1:-1] *= -3.0
        job.set_source(g2)
        job.run_source(5)
        bd.assert_bitwise(inner(job.download()), inner(sr.sweeps(sr.problem("fp64", *size), want, g2, 5)))
    finally:
        job.close()


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_alternating_run_and_run_source(gpu, dtype, world):
    steps = (("source", KS + 1), ("plain", 5), ("source", 2), ("plain", 4), ("source", 2 * KS))
    want, _ = single_grid(gpu, dtype, SIZE, steps)
    job = make_job(gpu, dtype, SIZE, world)
    try:
        for kind, n in steps:
            job.run_source(n) if kind == "source" else job.run(n)
        bd.assert_bitwise(inner(job.download()), inner(want))
    finally:
        job.close()


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_zero_source_equals_run(gpu, dtype):
    got = []
    for source in (True, False):
        job = SlabJob(StencilSpec(dims=3, dtype=dtype), *SIZE, [gpu] * 2, exchange="copy")
        try:
            job.fill_initial("random", 9)
            start = job.download()
            assert not np.signbit(inner(start)).any()
            if source:
                job.set_source(np.zeros((SIZE[2], SIZE[1], SIZE[0]), dtype=NP[dtype]))
                job.run_source(2 * KS + 1)
            else:
                job.run(2 * KS + 1)
            got.append(job.download())
        finally:
            job.close()
    bd.assert_bitwise(got[0], got[1])


# ---------------------------------------------- face-signalled source rounds
def tripled(u, g, nz):
    def three(a, fill):
        out = np.empty((3 * nz + 2,) + a.shape[1:], dtype=a.dtype)
        out[0], out[-1] = fill, fill
        out[1:-1] = np.concatenate([np.asarray(a)[1:-1]] * 3)
        return out
    return three(u, np.asarray(u)[0]), three(g, np.nan)


def ring_run(gpu, monkeypatch, dtype, size, exchange, env, sweeps):
    with monkeypatch.context() as m:
        m.setenv("STENCIL_SLAB_STAGED", "0")
        for name, value in env.items():
            m.setenv(name, value)
        job = make_job(gpu, dtype, size, 1, exchange=exchange, periodic=True)
        try:
            info = dict(job.round_info(), source_form=job.source_round_form(), k=job.info(0)["sweeps_per_round"])
            for n in sweeps:
                job.run_source(n)
            return info, job.download()
        finally:
            job.close()


@pytest.mark.parametrize("exchange", ["copy", "rccl"])
@pytest.mark.parametrize("dtype,k", [("fp64", 4), ("fp32", 4), ("fp64", 3), ("fp32", 3)])
def test_signalled_ring_matches_boundary_interior(gpu, monkeypatch, dtype, k, exchange):
    """A one-slab periodic ring (the rehearsal of an interior rank): full source
    rounds as one face-signalled launch against STENCIL_SLAB_SOURCE_SIGNAL=0,
    and both against the helper on the ring unrolled three times.  130 x 64
    planes: two tile rows and more; 4 K + 1 planes: two chunks of at least 2 K
    planes per tile, one marching up and one down."""
    size = (130, 64, 4 * k + 1)
    sweeps = (k, 1, k, k, 1)  # 3 K + 2 <= 4 K + 1 planes: the unrolled ring's ends stay out of the middle copy
    env = {"STENCIL_TK_STEPS": str(k)}
    info, got = ring_run(gpu, monkeypatch, dtype, size, exchange, env, sweeps)
    assert info["k"] == k and info["form"] == 1 and info["source_form"] == 1, info
    info0, got0 = ring_run(gpu, monkeypatch, dtype, size, exchange, dict(env, STENCIL_SLAB_SOURCE_SIGNAL="0"), sweeps)
    assert info0["form"] == 1 and info0["source_form"] == 0, info0
    bd.assert_bitwise(inner(got), inner(got0), "signalled against boundary + interior")
    u, g = fields(dtype, size)
    u3, g3 = tripled(u, g, size[2])
    want = sr.sweeps(sr.problem(dtype, size[0], size[1], 3 * size[2]), u3, g3, sum(sweeps))
    bd.assert_bitwise(inner(got), want[1 + size[2]:1 + 2 * size[2], 1:-1, 1:-1], "against the helper")


def test_ungated_source_rounds_on_a_gated_job(gpu, monkeypatch):
    """560 x 300 fp64 planes: the job's own launch has 10 x 7 tiles and is halo
    gated, the signalled source launch 10 x 13 -- too many for the gate's rule,
    so its rounds wait for the exchange's event between gated plain rounds."""
    size = (560, 300, 12)
    steps = (("plain", 4), ("source", 8), ("plain", 8), ("source", 4))
    out = []
    for env in ({}, {"STENCIL_SLAB_SOURCE_SIGNAL": "0"}):
        with monkeypatch.context() as m:
            m.setenv("STENCIL_SLAB_STAGED", "0")
            for name, value in env.items():
                m.setenv(name, value)
            job = make_job(gpu, "fp64", size, 1, periodic=True)
            try:
                info = job.round_info()
                assert info["form"] == 1 and info["gated"] and not info["confined"], info
                assert job.source_round_form() == (0 if env else 1)
                for kind, n in steps:
                    job.run_source(n) if kind == "source" else job.run(n)
                out.append(job.download())
            finally:
                job.close()
    bd.assert_bitwise(out[0], out[1])


def test_serial_knob(gpu, monkeypatch):
    monkeypatch.setenv("STENCIL_SLAB_SERIAL", "1")
    want, _ = single_grid(gpu, "fp64", SIZE, (("source", 3 * KS + 1),))
    job = make_job(gpu, "fp64", SIZE, 2)
    try:
        assert job.source_round_form() == 3
        job.run_source(3 * KS + 1)
        bd.assert_bitwise(inner(job.download()), inner(want))
    finally:
        job.close()


# ------------------------------------------------------------------ rank mode
def test_rank_mode_single_rank(gpu):
    sweeps = 2 * KS + 1
    want, _ = single_grid(gpu, "fp64", SIZE, (("source", sweeps),))
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), *SIZE, [gpu], exchange="rccl", rank=(1, 0, SlabJob.unique_id()))
    try:
        u, g = fields("fp64", SIZE)
        job.upload(np.asarray(u))
        job.set_source(np.asarray(g))
        job.run_source(sweeps)
        bd.assert_bitwise(inner(job.download()), inner(want))
        with pytest.raises(_lib.StencilError) as err:
            job.run_until_source(1e-3, 20, check_every=5)
        assert err.value.code == -5 and "rank" in str(err.value)
    finally:
        job.close()


# ---------------------------------------------------------------- convergence
CONV = {"fp64": (24, 20, 12), "fp32": (30, 14, 10)}


@functools.lru_cache(maxsize=None)
def single_until(gpu, dtype, tol, cap, every, norm):
    size = CONV[dtype]
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=gpu)
    e.reset("reference")
    e.set_source(np.full((size[2], size[1], size[0]), 1e-3, dtype=NP[dtype]))
    r = e.iterate_until_source(tol, cap, check_every=every, norm=norm)
    grid = bd.dense_of(e, r.grid)
    grid.setflags(write=False)
    return r.iterations, r.converged, r.norm, grid


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("norm,tol", [("max", 2e-3), ("l2", 5e-2)])
@pytest.mark.parametrize("every", [1, 7, 100])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_run_until_source(gpu, dtype, every, norm, tol, world):
    size = CONV[dtype]
    done, conv, last, grid = single_until(gpu, dtype, tol, 400, every, norm)
    assert conv and every <= done < 400 and done % every == 0  # the single grid's run converges inside the cap
    job = SlabJob(StencilSpec(dims=3, dtype=dtype), *size, [gpu] * world, exchange="copy")
    try:
        job.fill_initial("reference")
        job.set_source(np.full((size[2], size[1], size[0]), 1e-3, dtype=NP[dtype]))
        r = job.run_until_source(tol, 400, check_every=every, norm=norm)
        print(f"{dtype} {norm} every {every} world {world}: slabs ({r.iterations}, {r.converged}, {r.norm!r}), "
              f"single grid ({done}, {conv}, {last!r})")
        assert (r.iterations, r.converged) == (done, conv)
        assert bits(r.norm) == bits(last)
        assert r.grid is None and r.ms is not None and r.ms >= 0
        bd.assert_bitwise(inner(job.download()), inner(grid))
    finally:
        job.close()


def test_run_until_source_edges(gpu):
    size = CONV["fp64"]
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), *size, [gpu] * 2, exchange="copy")
    try:
        job.fill_initial("reference")
        job.set_source(np.full((size[2], size[1], size[0]), 1e-3))
        # the cap: a shorter last block, not converged
        done, conv, last, grid = single_until(gpu, "fp64", 1e-12, 17, 7, "max")
        assert (done, conv) == (17, False)
        r = job.run_until_source(1e-12, 17, check_every=7)
        assert (r.iterations, r.converged) == (17, False) and bits(r.norm) == bits(last)
        bd.assert_bitwise(inner(job.download()), inner(grid))
        # nothing to do
        r = job.run_until_source(1.0, 0, check_every=7)
        assert (r.iterations, r.converged, r.norm) == (0, False, float("inf"))
        # the argument errors of run_until
        f = job.lib.stencil_slab_run_until_source
        assert f(None, 5, 1, 0, 1e-3, None, None, None, None) == -1
        assert f(job.job, 5, 0, 0, 1e-3, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, -1.0, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, float("nan"), None, None, None, None) == -1
        assert f(job.job, 5, 1, 2, 1e-3, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, 1e-3, None, None, None, None) == 0  # every output pointer may be NULL
    finally:
        job.close()


# ------------------------------------------------------------------ rejections
def test_rejections(gpu):
    size = (37, 19, 20)
    u, g = fields("fp64", size)
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), *size, [gpu] * 2, exchange="copy")
    try:
        job.upload(np.asarray(u))
        for call in (lambda: job.run_source(4), lambda: job.run_until_source(1e-3, 8, check_every=4)):
            with pytest.raises(_lib.StencilError) as err:
                call()
            assert err.value.code == -1 and "set_source" in str(err.value)
        arr = np.asarray(g)
        assert job.lib.stencil_slab_set_source(job.job, None, arr.shape[2], arr.shape[1]) == -1
        assert job.lib.stencil_slab_set_source(job.job, arr.ctypes.data, arr.shape[2] - 1, arr.shape[1]) == -1
        job.run(3)  # the job is not failed by the refusals
    finally:
        job.close()
    rolling = SlabJob(StencilSpec(dims=3, dtype="fp64"), *size, [gpu] * 2, exchange="copy", rolling=True, margin=8)
    try:
        for call in (lambda: rolling.set_source(np.asarray(g)), lambda: rolling.run_source(4), rolling.source_round_form):
            with pytest.raises(_lib.StencilError) as err:
                call()
            assert err.value.code == -5 and "rolling" in str(err.value)
    finally:
        rolling.close()
    box = SlabJob(StencilSpec(dims=3, dtype="fp64", shape="box"), *size, [gpu] * 2, exchange="copy")
    try:
        for call in (lambda: box.set_source(np.asarray(g)), lambda: box.run_source(4)):
            with pytest.raises(_lib.StencilError) as err:
                call()
            assert err.value.code == -5 and "box" in str(err.value)
    finally:
        box.close()
