"""Source terms in slab jobs, without a GPU: the new C-ABI names, the host-only
plan, the rejections that need no device, and csrc/slab_core.hpp's source
rounds on the CPU fake device of tests/cpu_slab_source/ (real send / recv
between slabs at world 1, 2 and 3).  Everything is compared bit for bit with
tests/source_ref.py on the whole grid."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

from stencil_amd import _lib
from stencil_amd.engine import SlabJob, StencilSpec, slab_source_plan
from tests import boundary_data as bd
from tests import source_ref as sr
from tests.cpu_slab_source import binding as fsb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -5
NEW_PLAIN = ("stencil_sweepk_source_halo", "stencil_sweepk_signal_source", "stencil_sweepk_signal_source_gated")
NEW_SLAB = ("stencil_slab_set_source", "stencil_slab_run_source", "stencil_slab_run_until_source",
            "stencil_slab_source_plan", "stencil_slab_source_round_form")


# ---- names -------------------------------------------------------------------
def test_new_names_everywhere():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stencil_hip.h")).read(), flags=re.S)
    lib, dbg = _lib.load(debug=False), _lib.load(debug=True)
    for name in NEW_PLAIN + NEW_SLAB:
        assert re.search(r"^int " + name + r"\(", src, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name) and hasattr(dbg, name), name
    assert set(NEW_PLAIN) <= set(_lib.signatures())
    assert set(_lib.slab_source_signatures()) == set(NEW_SLAB)
    assert not set(_lib.slab_source_signatures()) & set(_lib.signatures())
    assert not set(_lib.slab_source_signatures()) & set(_lib.slab_until_signatures())
    assert not [n for n in _lib.signatures() if n.startswith("stencil_slab_") and "source" in n]
    # the knob is documented in the header's list and read by the product library
    assert "STENCIL_SLAB_SOURCE_SIGNAL" in _lib.API_KNOBS
    assert "STENCIL_SLAB_SOURCE_SIGNAL=0" in open(os.path.join(ROOT, "include", "stencil_hip.h")).read()


def test_fake_source_library_binds_the_source_names():
    lib = fsb.load()
    for short in fsb.SOURCE:
        assert callable(getattr(lib, "stencil_slab_" + short))


# ---- the plan (host only) ----------------------------------------------------
@pytest.mark.parametrize("dtype,n,k,ks", [("fp64", (70, 45, 41), 4, 4), ("fp32", (70, 45, 41), 4, 4),
                                          ("fp32", (1024, 1024, 64), 5, 4)])
def test_slab_source_plan(dtype, n, k, ks):
    spec = StencilSpec(dims=3, dtype=dtype)
    # K as stencil_plan resolves it for the global problem
    lay = _lib.make_layout(spec.problem(*n))
    launches, kernel = ctypes.c_int64(), ctypes.c_int32()
    assert _lib.load().stencil_plan(ctypes.byref(lay), k, ctypes.byref(launches), ctypes.byref(kernel)) == 0
    assert launches.value == 1
    assert _lib.load().stencil_plan(ctypes.byref(lay), k + 1, ctypes.byref(launches), ctypes.byref(kernel)) == 0
    assert launches.value == 2
    for it in (0, 1, 4, 5, 100):
        assert slab_source_plan(spec, *n, it) == {"rounds": -(-it // ks), "steps": ks}, it


def test_slab_source_plan_rejections():
    lib = _lib.load()
    rounds, steps = ctypes.c_int64(), ctypes.c_int32()
    assert lib.stencil_slab_source_plan(None, 4, ctypes.byref(rounds), ctypes.byref(steps)) == EINVAL
    for spec, word in ((StencilSpec(dims=3, shape="box"), "box"), (StencilSpec(dims=3, radius=2), "7-point")):
        with pytest.raises(_lib.StencilError) as e:
            slab_source_plan(spec, 32, 32, 32, 8)
        assert e.value.code == EUNSUPPORTED and word in str(e.value)
    with pytest.raises(_lib.StencilError) as e:
        slab_source_plan(StencilSpec(dims=2), 32, 32, 1, 8)
    assert e.value.code == EUNSUPPORTED


# ---- launch rejections that fire before any device call -----------------------
def _layout(flags=0, halo=0, **kw):
    return _lib.make_layout(_lib.make_problem(dims=3, nx=40, ny=30, nz=12, halo=halo, flags=flags, **kw))


def test_launch_rejections_need_no_device():
    lib = _lib.load()
    lay = _layout(_lib.HALO_LO | _lib.HALO_HI, 4)
    a, b, s, c = (ctypes.c_void_p(0x1000 * i) for i in (1, 2, 3, 4))
    n = ctypes.c_int32(0)
    L = ctypes.byref(lay)
    halo = lib.stencil_sweepk_source_halo
    assert halo(L, None, b, s, 0, 12, 4, None) == EINVAL
    assert halo(L, a, b, None, 0, 12, 4, None) == EINVAL
    assert halo(L, a, a, s, 0, 12, 4, None) == EINVAL
    assert halo(L, a, b, a, 0, 12, 4, None) == EINVAL
    assert halo(L, a, b, s, 0, 12, 0, None) == EINVAL
    assert halo(L, a, b, s, 0, 12, 5, None) == EINVAL
    assert halo(L, a, b, s, 0, 13, 4, None) == EINVAL
    assert halo(L, a, b, s, 5, 4, 4, None) == EINVAL
    sig = lib.stencil_sweepk_signal_source
    assert sig(L, a, b, s, 0, 12, 2, c, None, ctypes.byref(n), None) == EINVAL       # steps 3 or 4
    assert sig(L, a, b, s, 0, 12, 5, c, None, ctypes.byref(n), None) == EINVAL
    assert sig(L, a, b, s, 0, 12, 4, None, None, ctypes.byref(n), None) == EINVAL    # null counters
    assert sig(L, a, b, s, 0, 3, 4, c, None, ctypes.byref(n), None) == EINVAL        # a range shorter than steps
    assert "at least 4 planes" in lib.stencil_last_error_message().decode()
    assert lib.stencil_sweepk_signal_source_gated(L, a, b, s, 4, 6, 3, c, None, 0, None, ctypes.byref(n), None) == EINVAL
    for kw, word in ((dict(shape=_lib.BOX), "box"), (dict(radius=2), "radius"), (dict(kernel=_lib.KERNEL_ZMARCH), "kernel")):
        bad = _layout(**kw)
        assert halo(ctypes.byref(bad), a, b, s, 0, 12, 4, None) == EUNSUPPORTED
        assert word in lib.stencil_last_error_message().decode()
        assert sig(ctypes.byref(bad), a, b, s, 0, 12, 4, c, None, ctypes.byref(n), None) == EUNSUPPORTED
    # the single-grid entry keeps refusing halo layouts
    assert lib.stencil_sweepk_source(L, a, b, s, 0, 12, 4, None) == EUNSUPPORTED
    assert "halo" in lib.stencil_last_error_message().decode()


# ---- slab_core's source rounds on the fake device ----------------------------
pytestmark_fake = pytest.mark.skipif(not fsb.available(), reason="tests/cpu_slab_source/libslab_fake_source.so not built")


@pytest.fixture()
def fake():
    lib = fsb.load()

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


def tripled(u, g, nz):
    """Three copies of the interior planes stacked in z (a periodic ring's unrolled neighbourhood)."""
    def three(a, fill):
        out = np.empty((3 * nz + 2,) + a.shape[1:], dtype=a.dtype)
        out[0], out[-1] = fill, fill
        out[1:-1] = np.concatenate([a[1:-1]] * 3)
        return out
    return three(u, u[0]), three(g, np.nan)


@pytestmark_fake
@pytest.mark.parametrize("k", [2, 3, 4, 5])
@pytest.mark.parametrize("nslabs", [1, 2, 3])
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("exchange,devices", [("rccl", "distinct"), ("copy", "shared")])
def test_source_rounds_equal_one_grid(fake, k, nslabs, periodic, exchange, devices):
    """run_source / run alternating, full and remainder rounds, every round
    form the device assignment selects; K = 5 jobs run rounds of Ks = 4."""
    fake.set_k(k)
    ks = min(k, sr.K_MAX)
    dtype = "fp64" if k % 2 == 0 else "fp32"
    spec = StencilSpec(dims=3, dtype=dtype)
    nx, ny, nz = 11, 6, 5 * k * nslabs + (0 if periodic else 2)
    devs = list(range(nslabs)) if devices == "distinct" else [0] * nslabs
    job = SlabJob(spec, nx, ny, nz, devs, exchange=exchange, periodic=periodic, lib=fake)
    u, g = fields(dtype, nx, ny, nz)
    job.upload(u)
    job.set_source(g)
    assert job.source_plan(2 * ks + 1) == {"rounds": 3, "steps": ks}
    signalled = len(set(devs)) == len(devs) and k in (3, 4)  # one slab per device
    assert job.source_round_form() == (1 if signalled else 0)
    if periodic:
        u, g = tripled(u, g, nz)
    p = sr.problem(dtype, nx, ny, u.shape[0] - 2)
    for kind, it in (("source", 2 * ks + 1), ("plain", k - 1), ("source", ks), ("source", 1), ("plain", 1)):
        fake.stats(reset=True)
        if kind == "source":
            job.run_source(it)
            u = sr.sweeps(p, u, g, it)
            st = fake.stats()
            assert st["source_signal_sweeps"] == (it // ks * nslabs if signalled else 0), st
            assert st["source_sweeps"] >= (it // ks + (1 if it % ks else 0)) * nslabs and st["plain_sweeps"] == 0, st
        else:
            job.run(it)
            u = plain_sweeps(p, u, it)
            assert fake.stats()["source_sweeps"] == 0
        assert fake.stats()["gate_violations"] == 0
        got = job.download()
        want = u[nz:2 * nz + 2] if periodic else u
        bd.assert_bitwise(got[1:-1, 1:-1, 1:-1], want[1:-1, 1:-1, 1:-1], f"after {kind} x {it}")
    job.close()


@pytestmark_fake
@pytest.mark.parametrize("nslabs", [1, 2, 3])
def test_ungated_source_rounds_on_a_gated_job(fake, monkeypatch, nslabs):
    """A gated job whose source launch does not meet the gate's rule runs its
    source rounds ungated between gated plain rounds: no gate numbering
    violation, the same grid."""
    monkeypatch.setenv("FAKE_SLAB_SOURCE_GATE", "0")
    fake.set_k(4)
    spec = StencilSpec(dims=3, dtype="fp64")
    nx, ny, nz = 9, 5, 12 * nslabs + 1
    job = SlabJob(spec, nx, ny, nz, list(range(nslabs)), exchange="rccl", lib=fake)
    f, gated, _ = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert fake.stencil_slab_round_info(job.job, ctypes.byref(f), ctypes.byref(gated), None) == 0
    assert f.value == 1 and gated.value == 1
    u, g = fields("fp64", nx, ny, nz)
    p = sr.problem("fp64", nx, ny, nz)
    job.upload(u)
    job.set_source(g)
    fake.stats(reset=True)
    for kind, it in (("plain", 8), ("source", 8), ("plain", 4), ("source", 5), ("plain", 9)):
        if kind == "source":
            job.run_source(it)
            u = sr.sweeps(p, u, g, it)
        else:
            job.run(it)
            u = plain_sweeps(p, u, it)
    st = fake.stats()
    assert st["gate_violations"] == 0 and st["source_signal_sweeps"] == 3 * nslabs, st
    assert st["gated"] == (2 + 1 + 2) * nslabs, st  # the plain full rounds only
    bd.assert_bitwise(job.download()[1:-1, 1:-1, 1:-1], u[1:-1, 1:-1, 1:-1])
    job.close()


@pytestmark_fake
@pytest.mark.parametrize("case,form", [("default", 1), ("knob", 0), ("serial", 3), ("nosignal", 0), ("shared", 0),
                                       ("k5", 0)])
def test_source_round_form(fake, monkeypatch, case, form):
    fake.set_k(5 if case == "k5" else 4)
    if case == "knob":
        fake.set_source_signal(False)
    if case == "serial":
        monkeypatch.setenv("STENCIL_SLAB_SERIAL", "1")
    if case == "nosignal":
        fake.set_signal(False)
    devs = [0, 0] if case == "shared" else [0, 1]
    job = SlabJob(StencilSpec(dims=3, dtype="fp64"), 9, 5, 30, devs, exchange="copy", lib=fake)
    assert job.source_round_form() == form
    u, g = fields("fp64", 9, 5, 30)
    job.upload(u)
    job.set_source(g)
    fake.stats(reset=True)
    job.run_source(8)
    st = fake.stats()
    assert st["source_signal_sweeps"] == (4 if form == 1 else 0), st
    # one launch per slab and round (signalled, serial), or its interior and two boundary launches
    assert st["source_sweeps"] == (4 if form in (1, 3) else 12), st
    bd.assert_bitwise(job.download()[1:-1, 1:-1, 1:-1],
                      sr.sweeps(sr.problem("fp64", 9, 5, 30), u, g, 8)[1:-1, 1:-1, 1:-1])
    job.close()


@pytestmark_fake
def test_second_set_source_replaces_the_values(fake):
    fake.set_k(3)
    spec = StencilSpec(dims=3, dtype="fp32")
    nx, ny, nz = 8, 5, 20
    job = SlabJob(spec, nx, ny, nz, [0, 1], exchange="rccl", lib=fake)
    u, g = fields("fp32", nx, ny, nz)
    p = sr.problem("fp32", nx, ny, nz)
    job.upload(u)
    job.set_source(g)
    job.run_source(4)
    g2 = g.copy()
    g2[1:-1, 1:-1, 1:-1] *= np.float32(-2.5)
    job.set_source(g2[1:-1, 1:-1, 1:-1])  # the interior alone
    job.run_source(7)
    want = sr.sweeps(p, sr.sweeps(p, u, g, 4), g2, 7)
    bd.assert_bitwise(job.download()[1:-1, 1:-1, 1:-1], want[1:-1, 1:-1, 1:-1])
    job.close()


@pytestmark_fake
@pytest.mark.parametrize("nranks", [1, 2, 3])
def test_rank_mode_source_rounds(fake, nranks):
    """One process (here: thread) per slab, each reading only its own planes of
    the source array."""
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
            job.run_source(9)
            job.run(3)
            job.run_source(2)
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
    want = sr.sweeps(p, plain_sweeps(p, sr.sweeps(p, u, g, 9), 3), g, 2)
    for first, planes, got in out:
        bd.assert_bitwise(got[1 + first:1 + first + planes, 1:-1, 1:-1], want[1 + first:1 + first + planes, 1:-1, 1:-1])


@pytestmark_fake
def test_source_rejections(fake):
    fake.set_k(4)
    spec = StencilSpec(dims=3, dtype="fp64")
    u, g = fields("fp64", 9, 5, 20)
    job = SlabJob(spec, 9, 5, 20, [0, 1], exchange="copy", lib=fake)
    job.upload(u)
    with pytest.raises(_lib.StencilError) as e:
        job.run_source(4)
    assert e.value.code == EINVAL and "set_source" in str(e.value)
    assert fake.stencil_slab_set_source(job.job, None, 11, 7) == EINVAL
    assert fake.stencil_slab_set_source(None, ctypes.c_void_p(g.ctypes.data), 11, 7) == EINVAL
    assert fake.stencil_slab_set_source(job.job, ctypes.c_void_p(g.ctypes.data), 10, 7) == EINVAL  # too small
    assert fake.stencil_slab_set_source(job.job, ctypes.c_void_p(g.ctypes.data), 11, 6) == EINVAL
    assert fake.stencil_slab_run_source(None, 4, None) == EINVAL
    assert fake.stencil_slab_source_round_form(job.job, None) == EINVAL
    job.run(4)  # the refusals left the job usable
    job.set_source(g)
    job.run_source(4)
    p = sr.problem("fp64", 9, 5, 20)
    bd.assert_bitwise(job.download()[1:-1, 1:-1, 1:-1], sr.sweeps(p, plain_sweeps(p, u, 4), g, 4)[1:-1, 1:-1, 1:-1])
    job.close()
    rolling = SlabJob(spec, 9, 5, 20, [0, 1], exchange="copy", rolling=True, margin=8, lib=fake)
    for call in (lambda: rolling.set_source(g), lambda: rolling.run_source(4), rolling.source_round_form):
        with pytest.raises(_lib.StencilError) as e:
            call()
        assert e.value.code == EUNSUPPORTED and "rolling" in str(e.value)
    rolling.close()
    fake.set_k(3)
    box = SlabJob(StencilSpec(dims=3, dtype="fp64", shape="box"), 9, 5, 20, [0, 1], exchange="copy", lib=fake)
    for call in (lambda: box.set_source(g), lambda: box.run_source(4)):
        with pytest.raises(_lib.StencilError) as e:
            call()
        assert e.value.code == EUNSUPPORTED and "box" in str(e.value)
    box.close()
