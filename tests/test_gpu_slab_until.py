"""Convergence-controlled slab jobs on the GPU: the face-signalled K-step launch
that also reports its update (stencil_sweepk_signal_update_max) and
stencil_slab_run_until -- iterate_until's stopping rule over the slabs of a
multi-GPU job.

Every kernel is bitwise the naive sweep and a maximum does not depend on the
order it is taken in, so counts, norms (as bit patterns) and grids are compared
for equality: with the CPU oracle stepped from the reference initial condition,
or -- periodic one-slab jobs, which the oracle does not model -- with a second
job advanced one sweep at a time by run(1).
"""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import binding as ob
from stencil_amd import _lib
from stencil_amd.engine import FaceSignal, JacobiEngine, SlabJob, StencilSpec
from tests import boundary_data as bd
from tests import test_gpu_norm as tn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "build", "bin", "stencil_main")
HALO = _lib.HALO_LO | _lib.HALO_HI
CASES = [(dt, k) for dt in ("fp32", "fp64") for k in (3, 4, 5)]
# every (dtype, K) has a checking face-signalled launch (none spills); a shape recorded as
# not built would be listed here and must then return STENCIL_EUNSUPPORTED
NOT_BUILT = set()


def bits(x):
    return int(np.float64(x).view(np.uint64))


# ---------------------------------------------------------------- 1. the kernel
def kernel_engine(gpu, dtype, k, flags, nz=None):
    nz = 2 * k + 3 if nz is None else nz
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype, halo=k), 67, 29, nz, device=gpu, flags=flags)
    assert int(e.layout.zghost) == k
    bd.poison_and_fill(e, 301, True, same_ghosts=False)
    if flags:  # spikes in the slab-halo planes -1 and nz: advanced on the way, never stored
        view = bd.box_view(e, e.a, k)
        view[k - 1, 1 + 6, 1 + 10] = 500.0
        view[k + nz, 1 + 27, 1 + 66] = -700.0
        torch.cuda.synchronize()
    return e


def references(e, dst0, b, en, k):
    """sweepk_signal's grid and adds per face, sweepk_update_max's word, and numpy's
    max |double(S^K) - double(S^(K-1))| over the stored cells, both grids by sweepk."""
    ref, prev, cur, scratch = dst0.clone(), dst0.clone(), dst0.clone(), dst0.clone()
    sig = torch.zeros(4, dtype=torch.int32, device=e.device)
    nsig = e.sweepk_signal(e.a, ref, b, en, k, sig)
    e.sweepk(e.a, prev, b, en, k - 1)
    e.sweepk(e.a, cur, b, en, k)
    word = e.sweepk_update_max(e.a, scratch, b, en, k)
    torch.cuda.synchronize()
    assert sig.tolist() == [nsig, nsig, 0, 0]
    d = e.interior(cur)[b:en].cpu().numpy().astype(np.float64) - e.interior(prev)[b:en].cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ref, nsig, word, float(np.abs(d).max())


@pytest.mark.parametrize("flags", [0, HALO])
@pytest.mark.parametrize("zchunk", ["0", "5", "9"])
@pytest.mark.parametrize("dtype,k", CASES)
def test_signalled_checking_launch(gpu, monkeypatch, dtype, k, zchunk, flags):
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", zchunk)
    e = kernel_engine(gpu, dtype, k, flags)
    nz = e.slow_extent
    ib = torch.int64 if dtype == "fp64" else torch.int32
    dst0, src0 = e.b.clone(), e.a.clone()
    fs = FaceSignal()
    try:
        for b, en in ((0, nz), (1, nz - 1)):
            assert en - b >= k
            ref, nsig_ref, word_ref, word_np = references(e, dst0, b, en, k)
            if (dtype, k) in NOT_BUILT:
                with pytest.raises(_lib.StencilError) as err:
                    e.sweepk_signal_update_max(e.a, e.b, b, en, k, torch.zeros(4, dtype=torch.int32, device=e.device))
                assert err.value.code == -5
                continue
            for gate_need in (None, 0):  # the plain and the halo-gated entry point (a gate every word meets)
                e.b.copy_(dst0)
                fs.reset()
                sig = torch.zeros(4, dtype=torch.int32, device=e.device)
                nsig, word = e.sweepk_signal_update_max(e.a, e.b, b, en, k, sig, face_signal=fs, gate_need=gate_need)
                torch.cuda.synchronize()
                print(f"{dtype} K={k} zchunk {zchunk} flags {flags} [{b}, {en}) gate {gate_need}: word {word!r}, "
                      f"update_max {word_ref!r}, numpy {word_np!r}, adds {nsig} / {nsig_ref}")
                assert torch.equal(e.b.view(ib), ref.view(ib))  # the whole allocation, padding included
                assert nsig == nsig_ref > 0 and sig.tolist() == [nsig, nsig, 0, 0]
                assert fs.value() == 2
                assert bits(word) == bits(word_ref) == bits(word_np) and word > 0
                bd.assert_only_wrote(e, dst0, e.b, b, en)
                bd.assert_untouched(e, src0, e.a)
    finally:
        fs.close()


@pytest.mark.parametrize("dtype,k", CASES)
def test_checking_launch_nan_and_a_word_that_stays(gpu, monkeypatch, dtype, k):
    if (dtype, k) in NOT_BUILT:
        pytest.skip("recorded as not built (DESIGN.md §5.6); test_signalled_checking_launch asserts EUNSUPPORTED")
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", "5")
    e = kernel_engine(gpu, dtype, k, HALO)
    nz = e.slow_extent
    sig = torch.zeros(4, dtype=torch.int32, device=e.device)
    _, _, word_ref, _ = references(e, e.b.clone(), 0, nz, k)
    # a word that starts above the true maximum stays, to the bit; so does +inf
    for preset in (word_ref * 4, math.inf):
        _, word = e.sweepk_signal_update_max(e.a, e.b, 0, nz, k, sig, start_bits=bits(preset))
        assert bits(word) == bits(preset)
    _, word = e.sweepk_signal_update_max(e.a, e.b, 0, nz, k, sig, start_bits=bits(word_ref / 4))
    assert bits(word) == bits(word_ref)
    # an interior NaN: a NaN pattern, in an up-marching and in a down-marching chunk's planes
    for z in (1, nz - 2):
        keep = float(e.interior(e.a)[z, 14, 33])
        e.interior(e.a)[z, 14, 33] = float("nan")
        torch.cuda.synchronize()
        _, word = e.sweepk_signal_update_max(e.a, e.b, 0, nz, k, sig)
        assert math.isnan(word)
        assert math.isnan(e.sweepk_update_max(e.a, e.b, 0, nz, k))
        e.interior(e.a)[z, 14, 33] = keep
    torch.cuda.synchronize()


def test_checking_launch_invalid_arguments(gpu):
    k = 4
    e = JacobiEngine(StencilSpec(dims=3, dtype="fp64", halo=k), 20, 12, 11, device=gpu, flags=HALO)
    e.reset()
    word = torch.zeros(1, dtype=torch.int64, device=e.device)
    sig = torch.zeros(4, dtype=torch.int32, device=e.device)
    lay, a, b = ctypes.byref(e.layout), ctypes.c_void_p(e.a.data_ptr()), ctypes.c_void_p(e.b.data_ptr())
    w, c, n = ctypes.c_void_p(word.data_ptr()), ctypes.c_void_p(sig.data_ptr()), ctypes.c_int32(0)
    f, g = e.lib.stencil_sweepk_signal_update_max, e.lib.stencil_sweepk_signal_update_max_gated
    assert f(lay, a, b, 0, 11, k, c, None, None, ctypes.byref(n), None) == -1  # NULL word
    assert g(lay, a, b, 0, 11, k, c, None, None, 0, None, ctypes.byref(n), None) == -1
    assert e.lib.stencil_last_error_message()
    for steps in (2, 6):
        assert f(lay, a, b, 0, 11, steps, c, None, w, ctypes.byref(n), None) == -1
        assert g(lay, a, b, 0, 11, steps, c, None, w, 0, None, ctypes.byref(n), None) == -1
    assert f(lay, a, b, 0, 11, k, None, None, w, ctypes.byref(n), None) == -1  # NULL counters
    assert f(lay, a, b, -1, 11, k, c, None, w, ctypes.byref(n), None) == -1
    assert f(lay, a, b, 0, 12, k, c, None, w, ctypes.byref(n), None) == -1
    assert f(lay, a, a, 0, 11, k, c, None, w, ctypes.byref(n), None) == -1
    # a range of K - 1 planes would signal one face only: refused by the new entry points
    assert f(lay, a, b, 2, 2 + k - 1, k, c, None, w, ctypes.byref(n), None) == -1
    assert g(lay, a, b, 2, 2 + k - 1, k, c, None, w, 0, None, ctypes.byref(n), None) == -1
    torch.cuda.synchronize()
    assert sig.tolist() == [0, 0, 0, 0] and int(word.item()) == 0  # nothing was launched
    assert f(lay, a, b, 2, 2 + k, k, c, None, w, ctypes.byref(n), None) == 0
    torch.cuda.synchronize()
    assert n.value > 0 and sig.tolist() == [n.value, n.value, 0, 0]
    box = JacobiEngine(StencilSpec(dims=3, dtype="fp64", shape="box", halo=k), 20, 12, 11, device=gpu, flags=HALO)
    box.reset()
    lb = ctypes.byref(box.layout)
    ba, bb = ctypes.c_void_p(box.a.data_ptr()), ctypes.c_void_p(box.b.data_ptr())
    assert box.lib.stencil_sweepk_signal_update_max(lb, ba, bb, 0, 11, 3, c, None, w, ctypes.byref(n), None) == -5
    assert box.lib.stencil_sweepk_signal_update_max_gated(lb, ba, bb, 0, 11, 3, c, None, w, 0, None, ctypes.byref(n),
                                                          None) == -5
    torch.cuda.synchronize()


# ------------------------------------------------- the oracle's update norms
CAP = 400
# name: (nx, ny, nz), dtype, shape
CONFIGS = {
    "star_f64_67x29x22": ((67, 29, 22), "fp64", "star"),
    "star_f32_130x20x18": ((130, 20, 18), "fp32", "star"),
    "box_f32_40x24x12": ((40, 24, 12), "fp32", "box"),
}


def oracle_problem(cfg):
    n, dtype, shape = CONFIGS[cfg]
    return ob.problem(3, dtype, shape, 1, "naive", n[0], n[1], n[2])


@functools.lru_cache(maxsize=None)
def oracle_updates(cfg):
    """tests/test_gpu_norm.py's oracle_updates for this file's grids: the oracle
    stepped CAP sweeps from the reference initial condition, once; max and L2
    norm of u^n - u^(n-1) for n = 1 .. CAP (entry 0 unused)."""
    p = oracle_problem(cfg)
    cur = ob.init(p)
    old = cur.copy()
    maxes, l2s = [math.inf], [math.inf]
    for _ in range(CAP):
        ob.sweep(p, cur, old, 0, p.nz)
        cur, old = old, cur
        d = ob.interior(p, cur).astype(np.float64) - ob.interior(p, old).astype(np.float64)
        maxes.append(float(np.abs(d).max()))
        l2s.append(math.sqrt(math.fsum((d * d).ravel())))
    return maxes, l2s


@functools.lru_cache(maxsize=None)
def oracle_grid(cfg, count):
    return ob.run(oracle_problem(cfg), count)


def first_at_most(norms, tol):
    return next((n for n in range(1, len(norms)) if norms[n] <= tol), None)


def test_oracle_table():
    """The figures the cases below lean on, from the oracle alone."""
    f64, _ = oracle_updates("star_f64_67x29x22")
    f32, _ = oracle_updates("star_f32_130x20x18")
    box, _ = oracle_updates("box_f32_40x24x12")
    assert (first_at_most(f64, 1e-2), first_at_most(f64, 1e-3), first_at_most(f64, 1e-4)) == (25, 166, None)
    assert 1.3e-4 < f64[400] < 1.4e-4
    assert (first_at_most(f32, 1e-2), first_at_most(f32, 1e-3), first_at_most(f32, 1e-4)) == (25, 131, 306)
    assert (first_at_most(box, 1e-2), first_at_most(box, 1e-3), first_at_most(box, 1e-4)) == (21, 68, 133)


def make_job(gpu, cfg, world, **kw):
    n, dtype, shape = CONFIGS[cfg]
    job = SlabJob(StencilSpec(dims=3, dtype=dtype, shape=shape), n[0], n[1], n[2], [gpu] * world, exchange="copy", **kw)
    job.fill_initial("reference")
    return job


def assert_run(job, cfg, res, norms, count, conv, grid_count=None):
    print(f"{cfg}: got ({res.iterations}, {res.converged}, {res.norm!r}), want ({count}, {conv}, {norms[count]!r})")
    assert (res.iterations, res.converged) == (count, conv)
    assert bits(res.norm) == bits(norms[count])
    assert res.grid is None and res.ms is not None and res.ms >= 0
    assert tn.same_bits(job.download(), oracle_grid(cfg, count if grid_count is None else grid_count))


# ------------------------------------------------ 2. slabs sharing the one GPU
EVERY = [4, 5, 7, 10, 100]
RUNS = [(1e-2, CAP), (1e-3, CAP), (1e-12, 23)]
PLANES = {("star_f64_67x29x22", 1): [22], ("star_f64_67x29x22", 2): [11, 11], ("star_f64_67x29x22", 3): [8, 7, 7],
          ("star_f32_130x20x18", 1): [18], ("star_f32_130x20x18", 2): [9, 9], ("star_f32_130x20x18", 3): [6, 6, 6]}


@pytest.mark.parametrize("every", EVERY)
@pytest.mark.parametrize("tol,cap", RUNS)
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("cfg", ["star_f64_67x29x22", "star_f32_130x20x18"])
def test_run_until_stops_where_the_oracle_does(gpu, cfg, world, tol, cap, every):
    maxes, _ = oracle_updates(cfg)
    count, conv = tn.expected_stop(maxes, tol, every, cap)
    job = make_job(gpu, cfg, world)
    try:
        assert [job.info(i)["planes"] for i in range(world)] == PLANES[cfg, world]
        assert job.info(0)["sweeps_per_round"] == 4
        plan = job.until_plan(every)
        assert plan["fused_check"] and plan["rounds"] == -(-(every - 4) // 4) + 1
        assert_run(job, cfg, job.run_until(tol, cap, check_every=every), maxes, count, conv)
    finally:
        job.close()


# ------------------------------------------------------- 3. un-fused families
@pytest.mark.parametrize("every", [7, 10])
@pytest.mark.parametrize("tol,cap", [(1e-2, CAP), (1e-3, CAP), (1e-12, 23)])
@pytest.mark.parametrize("world", [2, 3])
def test_box_run_until(gpu, world, tol, cap, every):
    cfg = "box_f32_40x24x12"
    maxes, _ = oracle_updates(cfg)
    count, conv = tn.expected_stop(maxes, tol, every, cap)
    job = make_job(gpu, cfg, world)
    try:
        assert not job.until_plan(every)["fused_check"]
        assert_run(job, cfg, job.run_until(tol, cap, check_every=every), maxes, count, conv)
    finally:
        job.close()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_l2_is_the_single_grids(gpu, world):
    """The per-plane sums added in ascending global plane order: bit for bit
    JacobiEngine.iterate_until(norm="l2") on the one grid; the count by the
    rule of test_gpu_norm.test_l2_norm_stops_where_the_oracle_does."""
    cfg, every = "star_f64_67x29x22", 7
    n, dtype, _ = CONFIGS[cfg]
    _, l2s = oracle_updates(cfg)
    checks = list(range(every, CAP + 1, every))
    k = next(i for i in checks if l2s[i] < l2s[every] / 3)
    tol = math.sqrt(l2s[k - every] * l2s[k])
    count, conv = tn.expected_stop(l2s, tol, every, CAP)
    assert conv and count == k
    bound = (2 * n[0] * n[1] * n[2] + 8) * 2.0 ** -53
    assert all(abs(l2s[i] - tol) > bound * l2s[i] for i in checks if i <= count)
    single = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *n, device=gpu)
    single.reset()
    want = single.iterate_until(tol, CAP, check_every=every, norm="l2")
    assert (want.iterations, want.converged) == (count, True)
    job = make_job(gpu, cfg, world)
    try:
        assert not job.until_plan(every, "l2")["fused_check"]
        res = job.run_until(tol, CAP, check_every=every, norm="l2")
        print(f"l2 world {world}: slabs {res.norm!r}, single grid {want.norm!r}, oracle {l2s[count]!r}")
        assert (res.iterations, res.converged) == (count, True)
        assert bits(res.norm) == bits(want.norm)
        assert res.norm == pytest.approx(l2s[count], rel=bound, abs=0)
        assert tn.same_bits(job.download(), oracle_grid(cfg, count))
    finally:
        job.close()


@pytest.mark.parametrize("every", [4, 7, 100])
@pytest.mark.parametrize("tol,cap", [(1e-3, CAP), (1e-12, 23)])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cfg", ["star_f64_67x29x22", "star_f32_130x20x18"])
def test_unfused_knob_gives_the_same_run(gpu, monkeypatch, cfg, world, tol, cap, every):
    maxes, _ = oracle_updates(cfg)
    count, conv = tn.expected_stop(maxes, tol, every, cap)
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("STENCIL_UNTIL_FUSED", fused)
        job = make_job(gpu, cfg, world)
        try:
            assert job.until_plan(every)["fused_check"] == (fused == "1")
            res = job.run_until(tol, cap, check_every=every)
            assert_run(job, cfg, res, maxes, count, conv)
            got[fused] = (res.iterations, res.converged, bits(res.norm), job.download().tobytes())
        finally:
            job.close()
    assert got["1"] == got["0"]


# ------------------------------------------- 4. face-signalled checking rounds
def periodic_job(gpu, dtype, shape3):
    job = SlabJob(StencilSpec(dims=3, dtype=dtype), *shape3, [gpu], exchange="copy", periodic=True)
    job.fill_initial("random", 5)
    return job


def stepped_reference(gpu, dtype, shape3, sweeps):
    """A second job advanced by run(1): the grid after every sweep and numpy's
    max |double(u^n) - double(u^(n-1))| over the interior (entry 0 unused)."""
    job = periodic_job(gpu, dtype, shape3)
    try:
        grids, norms = [job.download()], [math.inf]
        for _ in range(sweeps):
            job.run(1)
            grids.append(job.download())
            d = grids[-1][1:-1, 1:-1, 1:-1].astype(np.float64) - grids[-2][1:-1, 1:-1, 1:-1].astype(np.float64)
            norms.append(float(np.abs(d).max()))
    finally:
        job.close()
    return grids, norms


def signalled_case(gpu, monkeypatch, dtype, k, shape3, every):
    monkeypatch.setenv("STENCIL_TK_STEPS", str(k))
    monkeypatch.setenv("STENCIL_SLAB_STAGED", "0")  # as test_gpu_slab._periodic_job: signals, not AUTO's staged rounds
    sweeps = 4 * every
    grids, norms = stepped_reference(gpu, dtype, shape3, sweeps)
    # a tol the third check meets (geometric middle of two checks' norms), and a cap that leaves a remainder
    # block: 2 sweeps (shorter than K: un-fused) after checks every K, K + 1 (a single-sweep round, then the
    # checking round) after checks every 2K + 1
    tol = math.sqrt(norms[2 * every] * norms[3 * every])
    rest = 2 if every == k else k + 1
    runs = [(tol, sweeps), (0.0, 2 * every + rest)]
    want = [tn.expected_stop(norms, t, every, c) for t, c in runs]
    assert want[0][1] and want[0][0] < sweeps and want[1] == (2 * every + rest, False)  # from the reference alone
    variants = [{}, {"STENCIL_SLAB_SIGNAL": "0"}, {"STENCIL_SLAB_GATE": "0"}, {"STENCIL_UNTIL_FUSED": "0"}]
    for env in variants:
        with monkeypatch.context() as m:
            for name, value in env.items():
                m.setenv(name, value)
            job = periodic_job(gpu, dtype, shape3)
            try:
                info = job.round_info()
                assert job.info(0)["sweeps_per_round"] == k
                assert (info["form"] == 1) == ("STENCIL_SLAB_SIGNAL" not in env), info
                if "STENCIL_SLAB_GATE" in env:
                    assert not info["gated"]
                assert job.until_plan(every)["fused_check"] == ("STENCIL_UNTIL_FUSED" not in env)
                for (t, cap), (count, conv) in zip(runs, want):
                    job.fill_initial("random", 5)
                    res = job.run_until(t, cap, check_every=every)
                    print(f"{dtype} K={k} {shape3} every {every} {env}: got ({res.iterations}, {res.converged}, "
                          f"{res.norm!r}), want ({count}, {conv}, {norms[count]!r})")
                    assert (res.iterations, res.converged) == (count, conv)
                    assert bits(res.norm) == bits(norms[count])
                    assert tn.same_bits(job.download(), grids[count])
            finally:
                job.close()


@pytest.mark.parametrize("every_of", ["K", "2K+1"])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("dtype,k", CASES)
def test_signalled_checking_rounds(gpu, monkeypatch, dtype, k, extra, every_of):
    signalled_case(gpu, monkeypatch, dtype, k, (67, 29, 2 * k + extra), k if every_of == "K" else 2 * k + 1)


def test_signalled_checking_rounds_two_tile_rows(gpu, monkeypatch):
    signalled_case(gpu, monkeypatch, "fp64", 4, (130, 64, 20), 4)


def test_command_processor_wait_keeps_boundary_interior_checks(gpu, monkeypatch):
    """STENCIL_SLAB_CPWAIT=1: the exchange waits on a HIP signal word the kernel
    raises by the running count modulo the launch's tiles.  On 67 x 45 planes
    the K = 4 checking launch (6-row strips: 40-row tiles) has 2 x 2 tiles, the
    job's own launches (48-row tiles) 2 x 1, so such a job keeps slab_round's
    form for its checking rounds.  The 20 s deadline turns a face signal that
    never rises into a failure instead of a hang."""
    monkeypatch.setenv("STENCIL_SLAB_TIMEOUT_MS", "20000")
    monkeypatch.setenv("STENCIL_SLAB_STAGED", "0")
    shape3, every, sweeps = (67, 45, 11), 4, 14
    grids, norms = stepped_reference(gpu, "fp64", shape3, sweeps)
    count, conv = tn.expected_stop(norms, 0.0, every, sweeps)
    assert (count, conv) == (sweeps, False)
    monkeypatch.setenv("STENCIL_SLAB_CPWAIT", "1")
    job = periodic_job(gpu, "fp64", shape3)
    try:
        assert job.round_info()["form"] == 1 and job.until_plan(every)["fused_check"]
        res = job.run_until(0.0, sweeps, check_every=every)
        assert (res.iterations, res.converged) == (count, conv) and bits(res.norm) == bits(norms[count])
        assert tn.same_bits(job.download(), grids[count])
        job.run(4)  # a face-signalled round behind the checks: the signal word's count is whole
        res = job.run_until(0.0, 16, check_every=8)  # a face-signalled round, then the checking round, twice
        assert res.iterations == 16 and not res.converged
    finally:
        job.close()


# ------------------------------------------------------------ 5. the job goes on
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cfg", ["star_f64_67x29x22", "box_f32_40x24x12"])
def test_the_job_goes_on(gpu, cfg, world):
    maxes, _ = oracle_updates(cfg)
    every = 7
    count, conv = tn.expected_stop(maxes, 1e-2, every, CAP)
    job = make_job(gpu, cfg, world)
    try:
        assert_run(job, cfg, job.run_until(1e-2, CAP, check_every=every), maxes, count, conv)
        job.run(5)
        assert tn.same_bits(job.download(), oracle_grid(cfg, count + 5))
        sums = job.plane_sums()
        assert sums.shape == (CONFIGS[cfg][0][2],) and np.isfinite(sums).all()
        # a second run_until from there, with a smaller tol: its blocks count from count + 5
        off = count + 5
        later = [math.inf] + maxes[off + 1:]
        more, conv2 = tn.expected_stop(later, 3e-3, every, 200)
        assert conv2 and more > every
        res = job.run_until(3e-3, 200, check_every=every)
        assert (res.iterations, res.converged) == (more, True) and bits(res.norm) == bits(later[more])
        assert tn.same_bits(job.download(), oracle_grid(cfg, off + more))
    finally:
        job.close()


# ------------------------------------------------------------------- 6. edges
def test_zero_iterations(gpu):
    cfg = "star_f64_67x29x22"
    job = make_job(gpu, cfg, 2)
    try:
        res = job.run_until(1e-3, 0, check_every=7)
        assert (res.iterations, res.converged, res.norm) == (0, False, math.inf)
        assert tn.same_bits(job.download(), oracle_grid(cfg, 0))
    finally:
        job.close()


@pytest.mark.parametrize("norm", ["max", "l2"])
@pytest.mark.parametrize("every", [7, 3])
def test_interior_nan_stops_at_the_first_check(gpu, norm, every):
    cfg = "star_f64_67x29x22"
    job = make_job(gpu, cfg, 3)
    try:
        dense = ob.init(oracle_problem(cfg))
        dense[1 + 12, 1 + 14, 1 + 33] = np.nan
        job.upload(dense)
        res = job.run_until(1e-3, 50, check_every=every, norm=norm)
        assert (res.iterations, res.converged) == (every, False) and math.isnan(res.norm)
    finally:
        job.close()


def test_unsupported_and_invalid(gpu):
    n = CONFIGS["star_f64_67x29x22"][0]
    rolling = SlabJob(StencilSpec(dims=3, dtype="fp64"), *n, [gpu, gpu], exchange="copy", rolling=True, margin=8)
    try:
        rolling.fill_initial("reference")
        with pytest.raises(_lib.StencilError) as err:
            rolling.run_until(1e-3, 20, check_every=5)
        assert err.value.code == -5 and "one grid" in str(err.value)
        rolling.run(5)  # the job is not failed by the refusal
    finally:
        rolling.close()
    job = make_job(gpu, "star_f64_67x29x22", 2)
    try:
        f = job.lib.stencil_slab_run_until

        def call(j=job.job, cap=5, every=1, norm=_lib.NORM_MAX, tol=1e-3):
            return f(j, cap, every, norm, tol, None, None, None, None)
        assert call(j=None) == -1
        assert call(every=0) == -1
        assert call(tol=-1e-9) == -1 and call(tol=float("nan")) == -1
        assert call(norm=2) == -1 and call(norm=-1) == -1
        assert job.lib.stencil_last_error_message()
        assert call() == 0  # every output pointer may be NULL
        assert tn.same_bits(job.download(), oracle_grid("star_f64_67x29x22", 5))
    finally:
        job.close()


# --------------------------------------------------------------------- 7. CLI
def cli(*args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("STENCIL_")}
    return subprocess.run([CLI, "--dims", "3", "-s", "24", "-b", "4", "--tol", "1e-3", "--check-every", "7", *args],
                          capture_output=True, text=True, timeout=120, env=env)


def test_cli_multi_gpu_stops_where_cpu_does(gpu):
    multi = ("-m", "HIPMultiGPU", "--gpus", "2", "--share-device", "--exchange", "copy")

    def count(p, method):
        assert p.returncode == 0, p.stdout + p.stderr
        assert f"The results of method {method} is correct." in p.stdout
        found = re.findall(rf"^\[stencil-amd\] {method}: converged after (\d+) sweeps, ", p.stdout, flags=re.M)
        assert found and len(set(found)) == 1
        return int(found[0])
    got = count(cli("-i", "400", *multi, "-c"), "HIPMultiGPU")
    want = count(cli("-i", "400", "-m", "CPU", "-c"), "CPU")
    assert got == want and 7 < got < 400 and got % 7 == 0
    p = cli("-i", "5", *multi)
    assert p.returncode == 5 and "not converged" in p.stdout, p.stdout + p.stderr
