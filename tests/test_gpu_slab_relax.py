"""Relaxed sweeps in slab jobs on the GPU (stencil_slab_run_relax,
run_until_relax, relax_plan, relax_round_form; SlabJob's methods): bit for bit
the single-grid relaxed job (JacobiEngine.iterate_relax / iterate_until_relax)
or tests/relax_ref.py.  No tolerances.

Fields and sources give every cell its own value, varying by plane and by row
(tests/boundary_data.py); the source array's ghost cells hold NaN.  The weights
are distinct and non-dyadic, so a round, a slab or a stage that took another's
weight shows in every cell.
"""
import functools
import struct

import numpy as np
import pytest
import torch

from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, SlabJob, StencilSpec, chebyshev_weights
from tests import boundary_data as bd
from tests import relax_ref as rr

pytestmark = pytest.mark.gpu

NP = {"fp32": np.float32, "fp64": np.float64}
KS = rr.K_MAX
SIZE = (70, 45, 41)
W = (0.8, 1.7, 0.6, 1.25, 0.9)
W3, PHASE = W[:3], 2  # a period of 3 entered at its last weight


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
    """steps = [("relax", n, omegas, phase) | ("source", n) | ("plain", n), ...] on the engine's grids, a holding
    the result."""
    for kind, n, *rest in steps:
        if kind == "relax":
            fin, _ = e.iterate_relax(n, rest[0], phase=rest[1])
        else:
            fin, _ = e.iterate_source(n) if kind == "source" else e.iterate(n)
        if fin is e.b:
            e.a, e.b = e.b, e.a
    return e.a


def run_steps(job, steps):
    for kind, n, *rest in steps:
        if kind == "relax":
            job.run_relax(n, rest[0], phase=rest[1])
        else:
            job.run_source(n) if kind == "source" else job.run(n)


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
    want, sums = single_grid(gpu, dtype, SIZE, (("relax", sweeps, W3, PHASE),))
    job = make_job(gpu, dtype, SIZE, world)
    try:
        assert job.info(0)["sweeps_per_round"] == 4
        assert job.relax_plan(sweeps) == {"rounds": 4, "steps": KS}
        assert job.relax_round_form() == (1 if world == 1 else 0)  # slabs sharing a GPU: boundary + interior
        ms = job.run_relax(sweeps, W3, phase=PHASE)
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
        job.run_relax(2 * KS + 3, W, phase=1)
        got = job.download()
        want = rr.sweeps(rr.problem("fp64", *size), np.asarray(u), np.asarray(g), 2 * KS + 3, W, 1)
        bd.assert_bitwise(inner(got), inner(want))
        bd.assert_bitwise(got[0], np.asarray(u)[0])  # the global ghost planes as uploaded
    finally:
        job.close()


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_continuation_with_phase(gpu, dtype):
    """run_relax(5) then run_relax(6, phase=5) is run_relax(11): other rounds, the same weight per sweep."""
    want, _ = single_grid(gpu, dtype, SIZE, (("relax", 11, W, 0),))
    job = make_job(gpu, dtype, SIZE, 3)
    try:
        job.run_relax(5, W, phase=0)
        job.run_relax(6, W, phase=5)
        bd.assert_bitwise(inner(job.download()), inner(want))
    finally:
        job.close()


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_alternating_run_run_source_and_run_relax(gpu, dtype, world):
    steps = (("relax", KS + 1, W3, 0), ("plain", 5), ("source", 2), ("relax", 2, W3, KS + 1), ("plain", 4),
             ("relax", 2 * KS, W, 3), ("source", KS))
    want, _ = single_grid(gpu, dtype, SIZE, steps)
    job = make_job(gpu, dtype, SIZE, world)
    try:
        run_steps(job, steps)
        bd.assert_bitwise(inner(job.download()), inner(want))
    finally:
        job.close()


def test_serial_knob(gpu, monkeypatch):
    monkeypatch.setenv("STENCIL_SLAB_SERIAL", "1")
    want, _ = single_grid(gpu, "fp64", SIZE, (("relax", 3 * KS + 1, W3, PHASE),))
    job = make_job(gpu, "fp64", SIZE, 2)
    try:
        assert job.relax_round_form() == 3
        job.run_relax(3 * KS + 1, W3, phase=PHASE)
        bd.assert_bitwise(inner(job.download()), inner(want))
    finally:
        job.close()


# ------------------------------------------------------------------ rank mode
def test_rank_mode_single_rank(gpu):
    sweeps = 2 * KS + 1
    want, _ = single_grid(gpu, "fp64", SIZE, (("relax", sweeps, W3, PHASE),))
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), *SIZE, [gpu], exchange="rccl", rank=(1, 0, SlabJob.unique_id()))
    try:
        u, g = fields("fp64", SIZE)
        job.upload(np.asarray(u))
        job.set_source(np.asarray(g))
        job.run_relax(sweeps, W3, phase=PHASE)
        bd.assert_bitwise(inner(job.download()), inner(want))
        with pytest.raises(_lib.StencilError) as err:
            job.run_until_relax(1e-3, 20, W3, check_every=5)
        assert err.value.code == -5 and "rank" in str(err.value)
        job.run_relax(1, W3)  # the refusal left the job usable
    finally:
        job.close()


# --------------------------------------------- face-signalled relaxed rounds
def tripled(u, g, nz):
    def three(a, fill):
        out = np.empty((3 * nz + 2,) + a.shape[1:], dtype=a.dtype)
        out[0], out[-1] = fill, fill
        out[1:-1] = np.concatenate([np.asarray(a)[1:-1]] * 3)
        return out
    return three(u, np.asarray(u)[0]), three(g, np.nan)


def ring_run(gpu, monkeypatch, dtype, size, exchange, env, sweeps):
    """A one-slab periodic ring; the schedule index runs on across the calls."""
    with monkeypatch.context() as m:
        m.setenv("STENCIL_SLAB_STAGED", "0")
        for name, value in env.items():
            m.setenv(name, value)
        job = make_job(gpu, dtype, size, 1, exchange=exchange, periodic=True)
        try:
            info = dict(job.round_info(), relax_form=job.relax_round_form(), k=job.info(0)["sweeps_per_round"])
            at = 0
            for n in sweeps:
                job.run_relax(n, W, phase=at)
                at += n
            return info, job.download()
        finally:
            job.close()


@pytest.mark.parametrize("exchange", ["copy", "rccl"])
@pytest.mark.parametrize("dtype,k", [("fp64", 4), ("fp32", 4), ("fp64", 3), ("fp32", 3)])
def test_signalled_ring_matches_boundary_interior(gpu, monkeypatch, dtype, k, exchange):
    """A one-slab periodic ring (the rehearsal of an interior rank): full relaxed
    rounds as one face-signalled launch against STENCIL_SLAB_SOURCE_SIGNAL=0,
    and both against the helper on the ring unrolled three times.  130 x 64
    planes: two tile rows and more; 4 K + 1 planes: two chunks of at least 2 K
    planes per tile, one marching up and one down."""
    size = (130, 64, 4 * k + 1)
    sweeps = (k, 1, k, k, 1)  # 3 K + 2 <= 4 K + 1 planes: the unrolled ring's ends stay out of the middle copy
    env = {"STENCIL_TK_STEPS": str(k)}
    info, got = ring_run(gpu, monkeypatch, dtype, size, exchange, env, sweeps)
    assert info["k"] == k and info["form"] == 1 and info["relax_form"] == 1, info
    info0, got0 = ring_run(gpu, monkeypatch, dtype, size, exchange, dict(env, STENCIL_SLAB_SOURCE_SIGNAL="0"), sweeps)
    assert info0["form"] == 1 and info0["relax_form"] == 0, info0
    bd.assert_bitwise(inner(got), inner(got0), "signalled against boundary + interior")
    u, g = fields(dtype, size)
    u3, g3 = tripled(u, g, size[2])
    want = rr.sweeps(rr.problem(dtype, size[0], size[1], 3 * size[2]), u3, g3, sum(sweeps), W)
    bd.assert_bitwise(inner(got), want[1 + size[2]:1 + 2 * size[2], 1:-1, 1:-1], "against the helper")


def test_relaxed_rounds_on_a_gated_job(gpu, monkeypatch):
    """560 x 300 fp64 planes: the job's own launch has 10 x 7 tiles and is halo
    gated, the signalled relaxed launch 10 x 13 -- too many for the gate's rule,
    so its rounds wait for the exchange's event between gated plain rounds."""
    size = (560, 300, 12)
    steps = (("plain", 4), ("relax", 8, W, 0), ("plain", 8), ("relax", 4, W, 8), ("source", 4), ("relax", 4, W, 12))
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
                assert job.relax_round_form() == (0 if env else 1)
                run_steps(job, steps)
                out.append(job.download())
            finally:
                job.close()
    bd.assert_bitwise(out[0], out[1])


# ---------------------------------------------------------------- convergence
CONV = {"fp64": ((24, 20, 12), 1e-7), "fp32": ((30, 14, 10), 1e-5)}
# sweeps to the tolerance with the P = 8 Chebyshev schedule, from tests/relax_ref.py's until() on the CPU
# (reference initial field, g = 1e-3, cap 600); plain Jacobi (omega = 1) does not converge in 600 sweeps at
# the fp64 size
COUNTS = {("fp64", 8): 136, ("fp64", 16): 144, ("fp32", 8): 72, ("fp32", 16): 80}
CAP = 600


def cheby(dtype):
    return tuple(chebyshev_weights(StencilSpec(dims=3, dtype=dtype), *CONV[dtype][0], 8))


def source_of(dtype):
    size = CONV[dtype][0]
    return np.full((size[2], size[1], size[0]), 1e-3, dtype=NP[dtype])


@functools.lru_cache(maxsize=None)
def single_until(gpu, dtype, tol, cap, every, norm):
    size = CONV[dtype][0]
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=gpu)
    e.reset("reference")
    e.set_source(source_of(dtype))
    r = e.iterate_until_relax(tol, cap, cheby(dtype), check_every=every, norm=norm)
    grid = bd.dense_of(e, r.grid)
    grid.setflags(write=False)
    return r.iterations, r.converged, r.norm, grid


def until_job(gpu, dtype, world):
    job = SlabJob(StencilSpec(dims=3, dtype=dtype), *CONV[dtype][0], [gpu] * world, exchange="copy")
    job.fill_initial("reference")
    job.set_source(source_of(dtype))
    return job


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("every", [8, 16])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_run_until_relax(gpu, monkeypatch, dtype, every, world):
    tol = CONV[dtype][1]
    done, conv, last, grid = single_until(gpu, dtype, tol, CAP, every, "max")
    if CONV[dtype][0][2] < 4 * world:
        # the fp32 grid's 10 planes over 3 slabs leave 3 planes to a slab, fewer than a K = 4 job's halo: that
        # world runs as a K = 3 job (rounds of 3 sweeps; counts, norms and grid do not depend on K)
        monkeypatch.setenv("STENCIL_TK_STEPS", "3")
    job = until_job(gpu, dtype, world)
    try:
        assert job.info(0)["sweeps_per_round"] == (3 if CONV[dtype][0][2] < 4 * world else 4)
        r = job.run_until_relax(tol, CAP, cheby(dtype), check_every=every)
        print(f"{dtype} every {every} world {world}: slabs ({r.iterations}, {r.converged}, {r.norm!r}), "
              f"single grid ({done}, {conv}, {last!r}), recorded {COUNTS[dtype, every]}")
        assert (r.iterations, r.converged) == (done, conv)
        assert r.converged and r.iterations == COUNTS[dtype, every]  # a run that stopped at the cap cannot pass
        assert bits(r.norm) == bits(last)
        assert r.grid is None and r.ms is not None and r.ms >= 0
        bd.assert_bitwise(inner(job.download()), inner(grid))
    finally:
        job.close()


def test_run_until_relax_edges(gpu):
    job = until_job(gpu, "fp64", 2)
    w = cheby("fp64")
    try:
        # the L2 norm, against the single grid only
        done, conv, last, grid = single_until(gpu, "fp64", 1e-5, CAP, 8, "l2")
        r = job.run_until_relax(1e-5, CAP, w, check_every=8, norm="l2")
        print(f"l2: slabs ({r.iterations}, {r.converged}, {r.norm!r}), single grid ({done}, {conv}, {last!r})")
        assert (r.iterations, r.converged) == (done, conv) and bits(r.norm) == bits(last)
        bd.assert_bitwise(inner(job.download()), inner(grid))
    finally:
        job.close()
    job = until_job(gpu, "fp64", 2)
    try:
        # the cap: a shorter last block, not converged; the schedule index runs on across the blocks
        done, conv, last, grid = single_until(gpu, "fp64", 1e-12, 17, 7, "max")
        assert (done, conv) == (17, False)
        r = job.run_until_relax(1e-12, 17, w, check_every=7)
        assert (r.iterations, r.converged) == (17, False) and bits(r.norm) == bits(last)
        bd.assert_bitwise(inner(job.download()), inner(grid))
        # nothing to do
        r = job.run_until_relax(1.0, 0, w, check_every=7)
        assert (r.iterations, r.converged, r.norm) == (0, False, float("inf"))
        # the argument errors of run_until, and those of the weights
        import ctypes
        f = job.lib.stencil_slab_run_until_relax
        om = (ctypes.c_double * 8)(*w)
        nan = (ctypes.c_double * 2)(1.0, float("nan"))
        assert f(None, 5, 1, 0, 1e-3, om, 8, 0, None, None, None, None) == -1
        assert f(job.job, 5, 0, 0, 1e-3, om, 8, 0, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, -1.0, om, 8, 0, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, float("nan"), om, 8, 0, None, None, None, None) == -1
        assert f(job.job, 5, 1, 2, 1e-3, om, 8, 0, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, 1e-3, None, 8, 0, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, 1e-3, om, 0, 0, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, 1e-3, nan, 2, 0, None, None, None, None) == -1
        assert f(job.job, 5, 1, 0, 1e-3, om, 8, 0, None, None, None, None) == 0  # every output pointer may be NULL
    finally:
        job.close()


# ------------------------------------------------------------------ rejections
def test_rejections(gpu):
    import ctypes
    size = (37, 19, 20)
    u, g = fields("fp64", size)
    w = (ctypes.c_double * 5)(*W)
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), *size, [gpu] * 2, exchange="copy")
    try:
        job.upload(np.asarray(u))
        for call in (lambda: job.run_relax(4, W), lambda: job.run_until_relax(1e-3, 8, W, check_every=4)):
            with pytest.raises(_lib.StencilError) as err:
                call()
            assert err.value.code == -1 and "set_source" in str(err.value)
        job.set_source(np.asarray(g))
        run = job.lib.stencil_slab_run_relax
        assert run(None, 4, w, 5, 0, None) == -1
        assert run(job.job, 4, None, 5, 0, None) == -1
        assert run(job.job, 4, w, 0, 0, None) == -1
        for bad in (float("nan"), float("inf")):
            with pytest.raises(_lib.StencilError) as err:
                job.run_relax(4, (0.8, bad))
            assert err.value.code == -1 and "weight 1" in str(err.value)
        job.run(3)  # the job is not failed by the refusals
        job.run_relax(3, W)
        want = rr.sweeps(rr.problem("fp64", *size), bd.oracle_steps(rr.problem("fp64", *size), np.asarray(u), 3, size[2]),
                         np.asarray(g), 3, W)
        bd.assert_bitwise(inner(job.download()), inner(want))
    finally:
        job.close()
    rolling = SlabJob(StencilSpec(dims=3, dtype="fp64"), *size, [gpu] * 2, exchange="copy", rolling=True, margin=8)
    try:
        for call in (lambda: rolling.run_relax(4, W), lambda: rolling.run_until_relax(1e-3, 8, W, check_every=4),
                     rolling.relax_round_form):
            with pytest.raises(_lib.StencilError) as err:
                call()
            assert err.value.code == -5 and "rolling" in str(err.value)
        rolling.run(3)
    finally:
        rolling.close()
    box = SlabJob(StencilSpec(dims=3, dtype="fp64", shape="box"), *size, [gpu] * 2, exchange="copy")
    try:
        for call in (lambda: box.run_relax(4, W), lambda: box.run_until_relax(1e-3, 8, W, check_every=4)):
            with pytest.raises(_lib.StencilError) as err:
                call()
            assert err.value.code == -5 and "box" in str(err.value)
        box.run(3)
    finally:
        box.close()
