"""Relaxed sweeps in slab jobs, without a GPU: the new C-ABI names, the
rejections that need no device, and csrc/slab_core.hpp's relaxed rounds on the
CPU fake device of tests/cpu_slab_relax/ (real send / recv between slabs at
world 1, 2 and 3).  Everything is compared bit for bit with tests/relax_ref.py
on the whole grid.  The weights are distinct and non-dyadic, so a round that
took another round's weights, or a slab that took another slab's, shows in
every cell."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

from stencil_amd import _lib
from stencil_amd.engine import SlabJob, StencilSpec, slab_source_plan
from tests import boundary_data as bd
from tests import relax_ref as rr
from tests import source_ref as sr
from tests.cpu_slab_relax import binding as frb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -5
W = (0.8, 1.7, 0.6, 1.25, 0.9)
NEW_PLAIN = ("stencil_sweepk_relax_halo", "stencil_sweepk_signal_relax", "stencil_sweepk_signal_relax_gated")
NEW_SLAB = ("stencil_slab_run_relax", "stencil_slab_run_until_relax", "stencil_slab_relax_plan",
            "stencil_slab_relax_round_form")


# ---- names -------------------------------------------------------------------
def test_new_names_everywhere():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stencil_hip.h")).read(), flags=re.S)
    lib, dbg = _lib.load(debug=False), _lib.load(debug=True)
    for name in NEW_PLAIN + NEW_SLAB:
        assert re.search(r"^int " + name + r"\(", src, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name) and hasattr(dbg, name), name
    assert set(NEW_PLAIN) <= set(_lib.signatures())
    assert set(_lib.slab_relax_signatures()) == set(NEW_SLAB)
    for other in (_lib.signatures(), _lib.slab_until_signatures(), _lib.slab_source_signatures()):
        assert not set(_lib.slab_relax_signatures()) & set(other)
    assert not [n for n in _lib.signatures() if n.startswith("stencil_slab_") and "relax" in n]


def test_fake_relax_library_binds_the_relaxed_names():
    lib = frb.load()
    for short in frb.PLAIN + frb.SOURCE + frb.RELAX:
        assert callable(getattr(lib, "stencil_slab_" + short))


def test_the_other_fake_libraries_have_no_relaxed_rounds():
    """slab_core.hpp's relaxed section is instantiated by tests/cpu_slab_relax/ alone."""
    from tests.cpu_slab import binding as fb
    from tests.cpu_slab_source import binding as fsb
    for path in (fb.PATH, fsb.PATH):
        cdll = ctypes.CDLL(path)
        assert not hasattr(cdll, "fake_relax_run_relax"), path


# ---- the plan (host only) ----------------------------------------------------
@pytest.mark.parametrize("dtype,n", [("fp64", (70, 45, 41)), ("fp32", (1024, 1024, 64))])
def test_slab_relax_plan_is_the_source_plan(dtype, n):
    spec = StencilSpec(dims=3, dtype=dtype)
    lib = _lib.load()
    prob = spec.problem(*n)
    for it in (0, 1, 4, 5, 100):
        rounds, steps = ctypes.c_int64(-1), ctypes.c_int32(-1)
        assert lib.stencil_slab_relax_plan(ctypes.byref(prob), it, ctypes.byref(rounds), ctypes.byref(steps)) == 0
        assert {"rounds": rounds.value, "steps": steps.value} == slab_source_plan(spec, *n, it)
    assert lib.stencil_slab_relax_plan(None, 4, None, None) == EINVAL
    box = StencilSpec(dims=3, shape="box").problem(32, 32, 32)
    assert lib.stencil_slab_relax_plan(ctypes.byref(box), 4, None, None) == EUNSUPPORTED
    assert "box" in lib.stencil_last_error_message().decode()


# ---- launch rejections that fire before any device call -----------------------
def _layout(flags=0, halo=0, **kw):
    return _lib.make_layout(_lib.make_problem(dims=3, nx=40, ny=30, nz=12, halo=halo, flags=flags, **kw))


def test_launch_rejections_need_no_device():
    lib = _lib.load()
    lay = _layout(_lib.HALO_LO | _lib.HALO_HI, 4)
    a, b, s, c = (ctypes.c_void_p(0x1000 * i) for i in (1, 2, 3, 4))
    n = ctypes.c_int32(0)
    L = ctypes.byref(lay)
    w = (ctypes.c_double * 5)(*W)
    nan = (ctypes.c_double * 4)(0.8, 1.7, float("nan"), 1.25)
    inf = (ctypes.c_double * 4)(0.8, 1.7, 0.6, float("inf"))
    halo = lib.stencil_sweepk_relax_halo
    assert halo(L, None, b, s, 0, 12, 4, w, None) == EINVAL
    assert halo(L, a, b, None, 0, 12, 4, w, None) == EINVAL
    assert halo(L, a, a, s, 0, 12, 4, w, None) == EINVAL
    assert halo(L, a, b, a, 0, 12, 4, w, None) == EINVAL
    assert halo(L, a, b, s, 0, 12, 0, w, None) == EINVAL
    assert halo(L, a, b, s, 0, 12, 5, w, None) == EINVAL
    assert halo(L, a, b, s, 0, 13, 4, w, None) == EINVAL
    assert halo(L, a, b, s, 5, 4, 4, w, None) == EINVAL
    assert halo(L, a, b, s, 0, 12, 4, None, None) == EINVAL
    assert "omegas" in lib.stencil_last_error_message().decode()
    assert halo(L, a, b, s, 0, 12, 4, nan, None) == EINVAL
    assert "weight 2" in lib.stencil_last_error_message().decode()
    sig = lib.stencil_sweepk_signal_relax
    assert sig(L, a, b, s, 0, 12, 2, w, c, None, ctypes.byref(n), None) == EINVAL       # steps 3 or 4
    assert sig(L, a, b, s, 0, 12, 5, w, c, None, ctypes.byref(n), None) == EINVAL
    assert sig(L, a, b, s, 0, 12, 4, w, None, None, ctypes.byref(n), None) == EINVAL    # null counters
    assert sig(L, a, b, None, 0, 12, 4, w, c, None, ctypes.byref(n), None) == EINVAL    # null source
    assert sig(L, a, b, s, 0, 3, 4, w, c, None, ctypes.byref(n), None) == EINVAL        # a range shorter than steps
    assert "at least 4 planes" in lib.stencil_last_error_message().decode()
    assert sig(L, a, b, s, 0, 12, 4, None, c, None, ctypes.byref(n), None) == EINVAL    # null weights
    assert sig(L, a, b, s, 0, 12, 4, inf, c, None, ctypes.byref(n), None) == EINVAL
    assert sig(L, a, b, s, 0, 12, 3, nan, c, None, ctypes.byref(n), None) == EINVAL
    gated = lib.stencil_sweepk_signal_relax_gated
    assert gated(L, a, b, s, 4, 6, 3, w, c, None, 0, None, ctypes.byref(n), None) == EINVAL
    assert gated(L, a, b, s, 0, 12, 4, nan, c, None, 0, None, ctypes.byref(n), None) == EINVAL
    for kw, word in ((dict(shape=_lib.BOX), "box"), (dict(radius=2), "radius"), (dict(kernel=_lib.KERNEL_ZMARCH), "kernel")):
        bad = _layout(**kw)
        assert halo(ctypes.byref(bad), a, b, s, 0, 12, 4, w, None) == EUNSUPPORTED
        assert word in lib.stencil_last_error_message().decode()
        assert sig(ctypes.byref(bad), a, b, s, 0, 12, 4, w, c, None, ctypes.byref(n), None) == EUNSUPPORTED
    # the single-grid entry keeps refusing halo layouts
    assert lib.stencil_sweepk_relax(L, a, b, s, 0, 12, 4, w, None) == EUNSUPPORTED
    assert "halo" in lib.stencil_last_error_message().decode()


# ---- slab_core's relaxed rounds on the fake device ----------------------------
pytestmark_fake = pytest.mark.skipif(not frb.available(), reason="tests/cpu_slab_relax/libslab_fake_relax.so not built")


@pytest.fixture()
def fake():
    lib = frb.load()

    def reset():
        lib.set_k(0)
        lib.set_signal(True)
        lib.set_source_signal(True)
        lib.stats(reset=True)
    reset()
    yield lib
    reset()


def fields(dtype, nx, ny, nz, seed=3):
    """A start grid whose every ghost cell has its own value, and a source whose
    every interior cell has its own value and whose ghost cells are all NaN."""
    npdt = np.float64 if dtype == "fp64" else np.float32
    u = bd.ring_field((nz + 2, ny + 2, nx + 2), 1, seed, npdt, star=True)
    g = np.full((nz + 2, ny + 2, nx + 2), np.nan, dtype=npdt)
    g[1:-1, 1:-1, 1:-1] = (0.01 * np.random.default_rng(seed + 7).standard_normal((nz, ny, nx))).astype(npdt)
    return u, g


def plain_sweeps(p, u, n):
    return bd.oracle_steps(p, u, n, p.nz)


def unrolled(u, g, nz, copies):
    """`copies` (odd) copies of the interior planes stacked in z: a periodic ring's
    unrolled neighbourhood.  The middle copy equals the ring for as many sweeps as
    the copies on either side of it have planes."""
    def many(a, fill):
        out = np.empty((copies * nz + 2,) + a.shape[1:], dtype=a.dtype)
        out[0], out[-1] = fill, fill
        out[1:-1] = np.concatenate([a[1:-1]] * copies)
        return out
    return many(u, u[0]), many(g, np.nan)


class Global:
    """The global grid a job is compared with: the Dirichlet grid itself, or a periodic ring unrolled."""

    def __init__(self, dtype, nx, ny, nz, periodic, total_sweeps, seed=3):
        self.nz = nz
        self.u0, self.g0 = fields(dtype, nx, ny, nz, seed)
        self.copies = 1
        if periodic:
            side = -(-total_sweeps // nz)
            self.copies = 2 * side + 1
        self.u, self.g = unrolled(self.u0, self.g0, nz, self.copies) if periodic else (self.u0, self.g0)
        self.p = sr.problem(dtype, nx, ny, self.u.shape[0] - 2)

    def relax(self, n, omegas, phase=0):
        self.u = rr.sweeps(self.p, self.u, self.g, n, omegas, phase)

    def source(self, n):
        self.u = sr.sweeps(self.p, self.u, self.g, n)

    def plain(self, n):
        self.u = plain_sweeps(self.p, self.u, n)

    def interior(self):
        first = 1 + (self.copies // 2) * self.nz
        return self.u[first:first + self.nz, 1:-1, 1:-1]


def inner(a):
    return a[1:-1, 1:-1, 1:-1]


@pytestmark_fake
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("signal", [True, False])
@pytest.mark.parametrize("k", [3, 4, 5])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_relaxed_rounds_equal_one_grid(fake, world, dtype, k, signal, periodic):
    """3 Ks + 2 sweeps with a schedule of period 5 entered at phase 2: three full
    rounds and a remainder of two, each with its own weights."""
    fake.set_k(k)
    fake.set_signal(signal)
    ks = min(k, rr.K_MAX)
    nx, ny, nz = 9, 7, world * (k + 1) + 1
    sweeps = 3 * ks + 2
    job = SlabJob(StencilSpec(dims=3, dtype=dtype), nx, ny, nz, list(range(world)), exchange="rccl", periodic=periodic,
                  lib=fake)
    try:
        ref = Global(dtype, nx, ny, nz, periodic, sweeps)
        job.upload(ref.u0)
        job.set_source(ref.g0)
        assert job.info(0)["sweeps_per_round"] == k
        assert job.relax_plan(sweeps) == {"rounds": 4, "steps": ks} == job.source_plan(sweeps)
        signalled = signal and k in (3, 4)
        assert job.relax_round_form() == (1 if signalled else 0) == job.source_round_form()
        fake.stats(reset=True)
        ms = job.run_relax(sweeps, W, phase=2)
        assert ms >= 0
        st = fake.stats()
        assert st["relax_signal_sweeps"] == (3 * world if signalled else 0), st
        assert st["relax_sweeps"] >= 4 * world and st["source_sweeps"] == 0 and st["plain_sweeps"] == 0, st
        assert st["gate_violations"] == 0, st
        ref.relax(sweeps, W, 2)
        bd.assert_bitwise(inner(job.download()), ref.interior(), f"world {world} {dtype} K={k}")
    finally:
        job.close()


@pytestmark_fake
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("k", [4, 5])
def test_continuation_with_phase(fake, world, k):
    """run_relax(5, phase 0) then run_relax(6, phase 5) is run_relax(11): the
    rounds are cut differently, the weights per sweep are the same."""
    fake.set_k(k)
    nx, ny, nz = 9, 7, world * (k + 1) + 1
    u, g = fields("fp64", nx, ny, nz)
    got = []
    for calls in (((5, 0), (6, 5)), ((11, 0),)):
        job = SlabJob(StencilSpec(dims=3, dtype="fp64"), nx, ny, nz, list(range(world)), exchange="rccl", lib=fake)
        try:
            job.upload(u)
            job.set_source(g)
            for n, phase in calls:
                job.run_relax(n, W, phase=phase)
            got.append(job.download())
        finally:
            job.close()
    bd.assert_bitwise(got[0], got[1])
    want = rr.sweeps(sr.problem("fp64", nx, ny, nz), u, g, 11, W)
    bd.assert_bitwise(inner(got[0]), inner(want))


@pytestmark_fake
@pytest.mark.parametrize("exchange,devices", [("rccl", "distinct"), ("copy", "shared")])
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_run_run_source_and_run_relax_alternate(fake, world, periodic, exchange, devices):
    k = 4
    fake.set_k(k)
    nx, ny, nz = 9, 7, world * (k + 1) + 1
    steps = (("relax", 2 * k + 1, 0), ("plain", k - 1, 0), ("source", k, 0), ("relax", 1, 3), ("plain", 1, 0),
             ("relax", k, 4), ("source", 2, 0))
    devs = list(range(world)) if devices == "distinct" else [0] * world
    job = SlabJob(StencilSpec(dims=3, dtype="fp32"), nx, ny, nz, devs, exchange=exchange, periodic=periodic, lib=fake)
    try:
        ref = Global("fp32", nx, ny, nz, periodic, sum(s[1] for s in steps))
        job.upload(ref.u0)
        job.set_source(ref.g0)
        signalled = len(set(devs)) == len(devs)  # one slab per device
        for kind, n, phase in steps:
            fake.stats(reset=True)
            if kind == "relax":
                job.run_relax(n, W, phase=phase)
                ref.relax(n, W, phase)
                st = fake.stats()
                assert st["relax_signal_sweeps"] == (n // k * world if signalled else 0), st
                assert st["source_sweeps"] == 0 and st["plain_sweeps"] == 0, st
            elif kind == "source":
                job.run_source(n)
                ref.source(n)
                assert fake.stats()["relax_sweeps"] == 0
            else:
                job.run(n)
                ref.plain(n)
                assert fake.stats()["relax_sweeps"] == 0 and fake.stats()["source_sweeps"] == 0
            assert fake.stats()["gate_violations"] == 0
            bd.assert_bitwise(inner(job.download()), ref.interior(), f"after {kind} x {n}")
    finally:
        job.close()


@pytestmark_fake
@pytest.mark.parametrize("case,form", [("default", 1), ("knob", 0), ("serial", 3), ("nosignal", 0), ("shared", 0),
                                       ("k5", 0)])
def test_relax_round_form(fake, monkeypatch, case, form):
    """Full rounds of a signalled job with Ks == K are signalled relaxed launches;
    K = 5 jobs, the knob, slabs sharing a GPU and unsignalled jobs take boundary +
    interior launches (or the serial one)."""
    fake.set_k(5 if case == "k5" else 4)
    if case == "knob":
        fake.set_source_signal(False)  # the one knob governs source and relaxed rounds
    if case == "serial":
        monkeypatch.setenv("STENCIL_SLAB_SERIAL", "1")
    if case == "nosignal":
        fake.set_signal(False)
    devs = [0, 0] if case == "shared" else [0, 1]
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), 9, 5, 30, devs, exchange="copy", lib=fake)
    try:
        assert job.relax_round_form() == form == job.source_round_form()
        u, g = fields("fp64", 9, 5, 30)
        job.upload(u)
        job.set_source(g)
        fake.stats(reset=True)
        job.run_relax(8, W, phase=1)
        st = fake.stats()
        assert st["relax_signal_sweeps"] == (4 if form == 1 else 0), st
        # one launch per slab and round (signalled, serial), or its interior and two boundary launches
        assert st["relax_sweeps"] == (4 if form in (1, 3) else 12), st
        assert st["source_sweeps"] == 0 and st["source_signal_sweeps"] == 0, st
        bd.assert_bitwise(inner(job.download()), inner(rr.sweeps(sr.problem("fp64", 9, 5, 30), u, g, 8, W, 1)))
    finally:
        job.close()


@pytestmark_fake
@pytest.mark.parametrize("relax_gate", ["1", "0"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_relaxed_rounds_on_a_gated_job(fake, monkeypatch, world, relax_gate):
    """A gated job runs its relaxed rounds gated (the relaxed launch's tiles meet
    the rule) or ungated (they do not) between gated plain rounds and source
    rounds that decide for themselves: no gate numbering violation, the same grid."""
    monkeypatch.setenv("FAKE_SLAB_RELAX_GATE", relax_gate)
    monkeypatch.setenv("FAKE_SLAB_SOURCE_GATE", "1" if relax_gate == "0" else "0")  # the two decisions are apart
    fake.set_k(4)
    nx, ny, nz = 9, 5, 12 * world + 1
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), nx, ny, nz, list(range(world)), exchange="rccl", lib=fake)
    try:
        f, gated = ctypes.c_int32(), ctypes.c_int32()
        assert fake.stencil_slab_round_info(job.job, ctypes.byref(f), ctypes.byref(gated), None) == 0
        assert f.value == 1 and gated.value == 1
        u, g = fields("fp64", nx, ny, nz)
        p = sr.problem("fp64", nx, ny, nz)
        job.upload(u)
        job.set_source(g)
        fake.stats(reset=True)
        at = 0
        for kind, it in (("plain", 8), ("relax", 8), ("plain", 4), ("relax", 5), ("source", 4), ("relax", 4), ("plain", 9)):
            if kind == "relax":
                job.run_relax(it, W, phase=at)
                u = rr.sweeps(p, u, g, it, W, at)
                at += it
            elif kind == "source":
                job.run_source(it)
                u = sr.sweeps(p, u, g, it)
            else:
                job.run(it)
                u = plain_sweeps(p, u, it)
        st = fake.stats()
        assert st["gate_violations"] == 0 and st["relax_signal_sweeps"] == 4 * world, st
        # gated launches: the plain full rounds (2 + 1 + 2), and either the relaxed (4) or the source (1) full rounds
        assert st["gated"] == (5 + (4 if relax_gate == "1" else 1)) * world, st
        bd.assert_bitwise(inner(job.download()), inner(u))
    finally:
        job.close()


@pytestmark_fake
@pytest.mark.parametrize("nranks", [2])
def test_rank_mode_relaxed_rounds(fake, nranks):
    """One process (here: thread) per slab; every rank passes the same schedule."""
    fake.set_k(4)
    spec = StencilSpec(dims=3, dtype="fp64")
    nx, ny, nz = 9, 6, 9 * nranks + 1
    u, g = fields("fp64", nx, ny, nz)
    p = sr.problem("fp64", nx, ny, nz)
    uid = SlabJob.unique_id(lib=fake)
    out, errs = [None] * nranks, []

    def rank(r):
        try:
            job = SlabJob(spec, nx, ny, nz, [r], exchange="rccl", rank=(nranks, r, uid), lib=fake)
            job.upload(u)
            job.set_source(g)
            job.run_relax(9, W, phase=2)
            job.run(3)
            job.run_source(2)
            job.run_relax(2, W, phase=11)
            i = job.info(0)
            out[r] = (i["first"], i["planes"], job.download())
            job.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=rank, args=(r,)) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not errs, errs
    want = rr.sweeps(p, sr.sweeps(p, plain_sweeps(p, rr.sweeps(p, u, g, 9, W, 2), 3), g, 2), g, 2, W, 11)
    for first, planes, got in out:
        bd.assert_bitwise(got[1 + first:1 + first + planes, 1:-1, 1:-1], want[1 + first:1 + first + planes, 1:-1, 1:-1])


@pytestmark_fake
def test_relax_rejections(fake):
    fake.set_k(4)
    spec = StencilSpec(dims=3, dtype="fp64")
    u, g = fields("fp64", 9, 5, 20)
    w = (ctypes.c_double * 5)(*W)
    job = SlabJob(spec, 9, 5, 20, [0, 1], exchange="copy", lib=fake)
    try:
        job.upload(u)
        with pytest.raises(_lib.StencilError) as e:
            job.run_relax(4, W)
        assert e.value.code == EINVAL and "set_source" in str(e.value)
        job.set_source(g)
        run = fake.stencil_slab_run_relax
        assert run(None, 4, w, 5, 0, None) == EINVAL
        assert run(job.job, 4, None, 5, 0, None) == EINVAL
        assert "omegas" in fake.stencil_last_error_message().decode()
        assert run(job.job, 4, w, 0, 0, None) == EINVAL
        assert "period" in fake.stencil_last_error_message().decode()
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(_lib.StencilError) as e:
                job.run_relax(4, (0.8, bad, 0.6))
            assert e.value.code == EINVAL and "weight 1" in str(e.value)
        # a weight outside the sweeps' reach is still part of the schedule
        with pytest.raises(_lib.StencilError) as e:
            job.run_relax(1, (0.8, 1.7, 0.6, 1.25, float("nan")))
        assert e.value.code == EINVAL
        assert fake.stencil_slab_relax_round_form(job.job, None) == EINVAL
        assert fake.stencil_slab_relax_round_form(None, ctypes.byref(ctypes.c_int32())) == EINVAL
        # the refusals left the job usable
        job.run(3)
        job.run_relax(4, W, phase=1)
        p = sr.problem("fp64", 9, 5, 20)
        bd.assert_bitwise(inner(job.download()), inner(rr.sweeps(p, plain_sweeps(p, u, 3), g, 4, W, 1)))
    finally:
        job.close()
    rolling = SlabJob(spec, 9, 5, 20, [0, 1], exchange="copy", rolling=True, margin=8, lib=fake)
    try:
        for call in (lambda: rolling.run_relax(4, W), rolling.relax_round_form):
            with pytest.raises(_lib.StencilError) as e:
                call()
            assert e.value.code == EUNSUPPORTED and "rolling" in str(e.value)
        rolling.run(3)
    finally:
        rolling.close()
    fake.set_k(3)
    box = SlabJob(StencilSpec(dims=3, dtype="fp64", shape="box"), 9, 5, 20, [0, 1], exchange="copy", lib=fake)
    try:
        for call in (lambda: box.run_relax(4, W), box.relax_round_form):
            with pytest.raises(_lib.StencilError) as e:
                call()
            assert e.value.code == EUNSUPPORTED and "box" in str(e.value)
        box.run(3)
    finally:
        box.close()
