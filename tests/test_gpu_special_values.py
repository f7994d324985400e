"""Every kernel family on subnormal, huge, infinite and NaN cells.

tests/test_gpu_boundary_data.py varies WHERE values sit; this file varies WHAT
they are.  The fields keep ring_field's structure (every ghost cell a value of
its own, a star's ring edges and all padding poison NaN) and draw their values
from the classes of tests/special_values.py:

  subnormal    operands, sums and products in and around the subnormal range
  wide         the whole exponent range in one neighbourhood, no overflow
  tiny_sparse  products that underflow to +0 and to -0
  overflow     partial sums that overflow; inf - inf in later sweeps
  nonfinite    planted +inf, -inf and NaN cells, ghosts included

Every comparison is against `ob.sweep` applied step by step, bit for bit; where
the result holds NaNs (the last two classes) they must sit exactly where the
oracle's do, with any payload (assert_same_values).  The write checks of the
boundary-data tests are kept: they compare the allocation's own bits.  Every
start field comes from special_values.SPECIAL, for which
tests/test_oracle_special_values.py shows on the CPU that the oracle is a
plain restatement of the sweep on these values; and every oracle result used
here is asserted to be in the regime its class is meant to reach
(special_values.assert_regime), so no case passes on a degenerate field.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import binding as ob
from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, SlabJob, StencilSpec
from tests import boundary_data as bd
from tests import special_values as sv
from tests import test_gpu_boundary_data as tb
from tests.test_gpu_boundary_data import FAMILIES, HALO, REGION2, REGION3, subrange

pytestmark = pytest.mark.gpu

KINDS = list(sv.KINDS)
FINITE = list(sv.NAN_FREE_KINDS)


@pytest.fixture(scope="module", autouse=True)
def drop_references():
    """The shared oracle grids of this file are released when it is done."""
    yield
    for key in [k for k in tb._STATES if k[0] == "special"]:
        del tb._STATES[key]


def fill(e, dims, dtype, shape, r, order, size, seed, kind, same_ghosts, tall=0):
    """Fill the engine's grids with the SPECIAL field of this case; returns
    (dense start, oracle problem, cache key, the sweep counts it is listed for)."""
    sc = sv.special_case(dims, dtype, shape, r, order, size, seed, kind, tall)
    start = sv.poison_and_fill(e, seed, shape == "star", same_ghosts=same_ghosts, kind=kind, q=sc["q"],
                               seams=sc["seams"], limit=sc["limit"])
    nx, ny, nz = size
    p = ob.problem(dims, dtype, shape, r, order, nx, ny, nz + 2 * tall)
    return start, p, ("special", dims, dtype, shape, r, order, size, seed, kind, tall), sc["sweeps"]


def regime(key, p, start, steps, slow, kind, tall=0, threads=1):
    """The oracle's interior after `steps` sweeps is where the class belongs."""
    want = tb.oracle_interiors(key, p, start, steps, slow, threads)
    first = tb.oracle_interiors(key, p, start, 1, slow, threads) if kind == "wide" else None
    res = want[tall:want.shape[0] - tall] if tall else want
    shape, r, order = key[3], key[4], key[5]
    return sv.assert_regime(kind, res, first, f"oracle after {steps} sweeps", shape, r, order, steps)


def setup_single(gpu, dtype, shape, kernel, size, seed, kind, r=1, halo=0, flags=0):
    e = tb.make_engine(gpu, 3, dtype, shape, r, "naive", kernel, size, halo=halo, flags=flags)
    tall = int(e.layout.zghost) if flags else 0
    start, p, key, sweeps = fill(e, 3, dtype, shape, r, "naive", size, seed, kind, False, tall)
    return e, p, start, tall, key, sweeps


def run_launch(e, launch, p, start, steps, ranges, key, sweeps, kind, tall=0, threads=1):
    assert steps in sweeps, f"{steps} sweeps are not listed in special_values.SPECIAL for {key}"
    regime(key, p, start, steps, int(e.prob.nz) + 2 * tall, kind, tall, threads)
    # the reference is in the cache now (computed with `threads`); check_launch compares with the class's comparison
    with sv.comparing(sv.comparison(kind)):
        tb.check_launch(e, launch, p, start, steps, ranges, key, tall=tall)


# ------------------------------------------------------------ single launches
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape,kernel,steps", FAMILIES)
def test_forced_families(gpu, monkeypatch, kind, dtype, shape, kernel, steps):
    """direct, zmarch, temporal2 and temporalk in both layouts, one launch of
    as many sweeps as the family fuses, several ragged tiles."""
    rows = kernel == "temporalk-rows"
    if rows:
        monkeypatch.setenv("STENCIL_TK_STRIP", "0")
        kernel = "temporalk"
    size = (130, 37, 29)
    e, p, start, tall, key, sweeps = setup_single(gpu, dtype, shape, kernel, size, 505, kind)
    assert e.plan(steps)[1] == _lib.KERNEL_NAMES[kernel]
    if rows:
        assert e.lib.stencil_debug_knobs() == 1
    run_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, [(0, 29), subrange(29)], key,
               sweeps, kind)


# strip shapes (STENCIL_TK_STRIP, debug library) exist per (dtype, K): the SPLIT shapes with 16-byte lane vectors
# (packed math may appear there), stage 1's history in LDS, and the default shape without its interior fast path
STRIP_SHAPES = ([(dt, k, "default") for dt in ("fp32", "fp64") for k in (3, 4, 5)]
                + [("fp32", 5, "1040208"), ("fp64", 4, "1020408"), ("fp64", 4, "810708"), ("fp64", 5, "810708"),
                   ("fp64", 4, "710708")])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("zchunk", [0, 7])
@pytest.mark.parametrize("dtype,steps,cfg", STRIP_SHAPES)
def test_tkstrip(gpu, monkeypatch, kind, zchunk, dtype, steps, cfg):
    """The strip K-step kernel: several ragged tiles, whole march and forced
    7-plane z-chunks, the default and the forced shapes."""
    monkeypatch.setenv("STENCIL_TK_ZCHUNK", str(zchunk))
    if cfg != "default":
        monkeypatch.setenv("STENCIL_TK_STRIP", cfg)
    size = (131, 61, 29)
    assert tb.multi_tile(dtype, size)
    e, p, start, tall, key, sweeps = setup_single(gpu, dtype, "star", "temporalk", size, 501, kind)
    assert not (zchunk or cfg != "default") or e.lib.stencil_debug_knobs() == 1  # the knobs are read
    ranges = [(0, 29), subrange(29, zchunk)]
    if cfg == "default":
        for b, en in ranges:
            geo = e.sweepk_geometry(steps, b, en)
            chunks = -(-(en - b) // zchunk) if zchunk else 1
            assert geo["workgroups"] // chunks > 1 and (not zchunk or (geo["zchunk"] == zchunk and chunks > 1)), geo
    run_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, ranges, key, sweeps, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fast", [0, 5])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("steps", [3, 4, 5])
def test_tkstrip_interior_tiles(gpu, monkeypatch, kind, fast, dtype, steps):
    """Interior tiles with no ghost selects at all (STENCIL_TK_FAST=5) beside
    edge tiles, and every tile with them (0)."""
    monkeypatch.setenv("STENCIL_TK_FAST", str(fast))
    size = (300, 250, 40)
    w, h = REGION3[dtype]
    assert size[0] > 2 * w and size[1] > 2 * h  # at least 3 x 3 tiles: one with no edge
    e, p, start, tall, key, sweeps = setup_single(gpu, dtype, "star", "temporalk", size, 502, kind)
    assert e.sweepk_geometry(steps)["workgroups"] >= 9 and e.lib.stencil_debug_knobs() == 1
    run_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, [(0, 40), subrange(40)], key,
               sweeps, kind, threads=16)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("zchunk", [0, 5])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("steps", [1, 2, 3, 4])
def test_box_strip(gpu, monkeypatch, kind, zchunk, dtype, steps):
    """The 27-point box's K-step launches, the default shape per step count,
    whole march and forced 5-plane z-chunks.  `acc - centre` is where an
    infinite sum meets an infinite centre."""
    monkeypatch.setenv("STENCIL_BOXK_ZCHUNK", str(zchunk))
    size = (131, 61, 29)
    e, p, start, tall, key, sweeps = setup_single(gpu, dtype, "box", "auto", size, 501, kind)
    assert e.lib.stencil_debug_knobs() == 1
    run_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, [(0, 29), subrange(29, zchunk)],
               key, sweeps, kind)
    assert tb.box_tiles(e, 2) > 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape,r", [("star", 2), ("star", 3), ("box", 2)])
def test_direct_wider_stencils(gpu, kind, dtype, shape, r):
    size = (45, 23, 17)
    e, p, start, tall, key, sweeps = setup_single(gpu, dtype, shape, "direct", size, 506, kind, r=r)
    assert e.plan(1) == (1, _lib.KERNEL_DIRECT)
    run_launch(e, lambda s, d, b, en: e.sweep(s, d, b, en), p, start, 1, [(0, 17), subrange(17)], key, sweeps, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", ["star", "box"])
def test_halo_layout(gpu, kind, dtype, shape):
    """HALO_LO|HALO_HI at the engine's fuse_steps: K live planes per side,
    advanced in registers and never stored -- special cells among them."""
    size = (131, 61, 29)
    steps = JacobiEngine(StencilSpec(dims=3, dtype=dtype, shape=shape), *size, device=gpu, allocate=False).fuse_steps
    e, p, start, tall, key, sweeps = setup_single(gpu, dtype, shape, "auto", size, 503, kind, halo=steps, flags=HALO)
    assert int(e.layout.zghost) == steps == tall
    run_launch(e, lambda s, d, b, en: e.sweepk(s, d, b, en, steps), p, start, steps, [(0, 29), subrange(29)], key,
               sweeps, kind, tall=tall)


# ------------------------------------------------------------ update-max, norms
@pytest.mark.parametrize("kind", FINITE)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_update_max(gpu, kind, dtype):
    """stencil_sweepk_update_max at fuse_steps: the plain launch's grid, and
    the word is max |double(u_K) - double(u_(K-1))| of the oracle's two last
    grids -- exact in double, so compared for equality (subnormal differences
    included)."""
    size = (131, 61, 29)
    e, p, start, tall, key, sweeps = setup_single(gpu, dtype, "star", "auto", size, 501, kind)
    k = e.fuse_steps
    assert k in sweeps and k - 1 in sweeps
    regime(key, p, start, k, 29, kind)
    src0, dst0 = e.a.clone(), e.b.clone()
    for b, en in ((0, 29), subrange(29)):
        e.b.copy_(dst0)
        cur = tb.oracle_interiors(key, p, start, k, 29)[b:en]
        prev = tb.oracle_interiors(key, p, start, k - 1, 29)[b:en]
        want = float(np.abs(cur.astype(np.float64) - prev.astype(np.float64)).max())
        got = e.sweepk_update_max(e.a, e.b, b, en, k)
        torch.cuda.synchronize()
        print(f"{kind} {dtype} planes [{b}, {en}): got {got!r} want {want!r}")
        # tiny_sparse: (1/6) of at most six smallest subnormals rounds to zero within K sweeps; both grids are +-0
        assert (want > 0 or kind == "tiny_sparse") and got == want, (got, want)
        bd.assert_only_wrote(e, dst0, e.b, b, en)
        bd.assert_untouched(e, src0, e.a)
        bd.assert_bitwise(e.interior(e.b)[b:en].cpu().numpy(), cur, f"u^{k} on [{b}, {en})")


@pytest.mark.parametrize("kind", ["subnormal", "wide"])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_diff_norms(gpu, kind, dtype):
    """stencil_diff_norms of two fields of one class: max_abs is numpy's; sum_sq
    is within the reordering bound of tests/test_gpu_bench_outputs.py,
    (n - 1) 2^-53 relative for n non-negative terms, of the exactly rounded sum
    of the squares formed in double.  Squares of fp64 subnormals are 0 on both
    sides; those of fp32 subnormals are normal doubles."""
    size = (131, 61, 29)
    e = tb.make_engine(gpu, 3, dtype, "star", 1, "naive", "auto", size)
    sc = sv.special_case(3, dtype, "star", 1, "naive", size, 501, kind)
    sv.poison_and_fill(e, 501, True, same_ghosts=False, kind=kind, q=sc["q"])
    ia, ib = e.interior(e.a).cpu().numpy(), e.interior(e.b).cpu().numpy()
    for f in (ia, ib):
        c = sv.census(f)
        assert c["nan"] + c["+inf"] + c["-inf"] == 0 and (kind != "subnormal" or 4 * c["subnormal"] >= f.size), c
    d = (ia.astype(np.float64) - ib.astype(np.float64)).reshape(29, -1)
    with np.errstate(over="ignore"):
        sq = d * d
    want_max = np.abs(d).max(axis=1)
    want_sum = np.array([math.fsum(row) for row in sq])
    got_max, got_sum = e.diff_norms(e.a, e.b)
    assert bd.same_bits(got_max, want_max)
    n = d.shape[1]
    ok = np.isfinite(want_sum)  # fp64 wide: squares beyond 2^1024 are +inf on both sides
    assert bd.same_bits(got_sum[~ok], want_sum[~ok]) and (ok.all() or (kind, dtype) == ("wide", "fp64"))
    assert np.all(np.abs(got_sum[ok] - want_sum[ok]) <= (n - 1) * 2.0 ** -53 * want_sum[ok]), (got_sum, want_sum)
    if kind == "subnormal":
        assert (want_max > 0).all()
        if dtype == "fp64":
            assert (want_sum == 0).all() and bd.same_bits(got_sum, np.zeros(29))
        else:
            assert (want_sum > 0).all()


# ----------------------------------------------------------------- whole jobs
def run_job(e, p, start, it, slow, key, sweeps, kind, run=None):
    assert it in sweeps, f"{it} sweeps are not listed in special_values.SPECIAL for {key}"
    regime(key, p, start, it, slow, kind)
    with sv.comparing(sv.comparison(kind)):
        tb.check_job(e, p, start, it, slow, key, run=run)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", ["star", "box"])
def test_3d_jobs(gpu, monkeypatch, kind, dtype, shape):
    """AUTO's 3D jobs, 2 K + 1 sweeps: two K-step launches and a single sweep.
    overflow and nonfinite bound the spread by planting and by a smaller K
    (STENCIL_TK_STEPS=3, STENCIL_BOX_STEPS=2)."""
    if kind in sv.NAN_KINDS:
        monkeypatch.setenv("STENCIL_TK_STEPS" if shape == "star" else "STENCIL_BOX_STEPS", "3" if shape == "star" else "2")
    size = (131, 61, 29)
    e = tb.make_engine(gpu, 3, dtype, shape, 1, "naive", "auto", size)
    start, p, key, sweeps = fill(e, 3, dtype, shape, 1, "naive", size, 504, kind, True)
    k = e.fuse_steps
    assert k >= (3 if kind in sv.NAN_FREE_KINDS or shape == "star" else 2) and e.plan(2 * k + 1)[0] == 3
    run_job(e, p, start, 2 * k + 1, 29, key, sweeps, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("order", ["naive", "dma"])
@pytest.mark.parametrize("r,cfg", [(1, "default"), (1, "92808"), (1, "192808"), (2, "default"), (2, "92808"),
                                   (2, "192808"), (3, "default"), (4, "default"), (5, "default")])
def test_2d_star_jobs(gpu, monkeypatch, kind, dtype, order, r, cfg):
    """2D stars through AUTO over several ragged tiles: the register-strip
    regions with per-row branches (92808) and with branch-free ghost selects
    (192808, and the default), the LDS regions, sweep_direct (r = 5).  23
    sweeps; overflow and nonfinite: STENCIL_TB2D_K=3 and 7 sweeps -- two 3-step
    launches and a single sweep -- so that most of the grid stays finite."""
    if cfg != "default":
        monkeypatch.setenv("STENCIL_TB2D_CFG", cfg)
    size = (301, 170, 1)
    assert size[0] > 2 * REGION2[0] and size[1] > 2 * REGION2[1]
    nan = kind in sv.NAN_KINDS
    if nan:
        monkeypatch.setenv("STENCIL_TB2D_K", "3")
    e = tb.make_engine(gpu, 2, dtype, "star", r, order, "auto", size)
    start, p, key, sweeps = fill(e, 2, dtype, "star", r, order, size, 601, kind, True)
    it = 23 if not nan else (7 if r < 5 else 3)
    if nan:
        assert e.plan(it)[0] == 3 and e.lib.stencil_debug_knobs() == 1
    elif r <= 4:
        assert e.plan(it)[0] < it  # K-step launches
    run_job(e, p, start, it, 170, key, sweeps, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", ["naive", "dma"])
@pytest.mark.parametrize("size,r", [((64, 64, 1), 1), ((64, 64, 1), 2), ((64, 64, 1), 3), ((64, 64, 1), 4),
                                    ((20, 9, 1), 1), ((20, 9, 1), 2)])
def test_2d_single_workgroup_jobs(gpu, kind, order, size, r):
    """Grids one workgroup holds in LDS: the whole job is one launch."""
    for dtype in ("fp32", "fp64"):
        e = tb.make_engine(gpu, 2, dtype, "star", r, order, "auto", size)
        start, p, key, sweeps = fill(e, 2, dtype, "star", r, order, size, 602, kind, True)
        it = sweeps[-1]
        assert e.plan(it)[0] == 1
        run_job(e, p, start, it, size[1], key, sweeps, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("order", ["naive", "dma"])
def test_2d_persistent_jobs(gpu, kind, dtype, r, order):
    """The persistent kernel: one cooperative launch for the whole job."""
    size = (64, 64, 1)
    e = tb.make_engine(gpu, 2, dtype, "star", r, order, "persistent", size)
    start, p, key, sweeps = fill(e, 2, dtype, "star", r, order, size, 603, kind, True)
    it = sweeps[-1]
    assert e.plan(it) == (1, _lib.KERNEL_PERSISTENT)
    run_job(e, p, start, it, 64, key, sweeps, kind)


# ------------------------------------------------------------------ slab jobs
@pytest.mark.parametrize("kind", ["subnormal", "nonfinite"])
@pytest.mark.parametrize("dtype,shape", [("fp64", "star"), ("fp32", "box")])
@pytest.mark.parametrize("nslabs", [2, 3])
def test_slab_job(gpu, kind, dtype, shape, nslabs):
    """SlabJob, slabs sharing the GPU with the copy exchange: an uploaded field,
    2 K + 1 sweeps, the downloaded grid against the oracle -- special cells on
    both sides of every slab seam and in the ghost ring."""
    size = (70, 45, 41)
    nx, ny, nz = size
    bd.require_bounded(3, dtype, shape, 1, "naive")
    key = next(k for k in sv.SPECIAL if k[:8] == (3, dtype, shape, 1, "naive", size, 701, kind))
    start = sv.special_start(key)
    p = ob.problem(3, dtype, shape, 1, "naive", nx, ny, nz)
    job = SlabJob(StencilSpec(dims=3, dtype=dtype, shape=shape), nx, ny, nz, devices=[gpu] * nslabs, exchange="copy")
    k = job.info(0)["sweeps_per_round"]
    it = 2 * k + 1
    assert k >= 3 and it in sv.SPECIAL[key], (k, sv.SPECIAL[key])
    firsts = [job.info(i)["first"] for i in range(1, nslabs)]
    assert kind != "nonfinite" or all(z in key[9][0] for z in firsts), firsts  # planted on both sides of each seam
    want = bd.oracle_steps(p, start, it, nz)
    sv.assert_regime(kind, want[1:-1, 1:-1, 1:-1], None, f"oracle after {it} sweeps", shape, 1, "naive", it)
    job.upload(start)
    bd.assert_bitwise(job.download(), start, "upload / download")  # NaN payloads and infinities travel unchanged
    job.run(it)
    sv.comparison(kind)(job.download(), want, f"after {it} sweeps")
    job.close()


# -------------------------------------------------------------- reference ABI
@pytest.mark.parametrize("kind", ["subnormal", "nonfinite"])
@pytest.mark.parametrize("fn,order", [("stencil_iterate_dma", "dma"), ("stencil_iterate_dma_static_unroll", "naive")])
@pytest.mark.parametrize("n,r", [(64, 1), (96, 3)])
@pytest.mark.parametrize("it", [6, 7])
def test_reference_abi(gpu, kind, fn, order, n, r, it):
    """The reference entry points on host buffers: the parity-selected buffer
    is the oracle's grid in that variant's order, and neither buffer's ghosts
    change."""
    lib = _lib.load()
    bd.require_bounded(2, "fp32", "star", r, order)
    key = next(k for k in sv.SPECIAL if k[:8] == (2, "fp32", "star", r, order, (n, n, 1), 801, kind))
    assert it in sv.SPECIAL[key]
    p = ob.problem(2, "fp32", "star", r, order, n, n)
    start = sv.special_start(key)
    want = bd.oracle_steps(p, start, it, n)
    sv.assert_regime(kind, want[r:-r, r:-r], None, f"oracle after {it} sweeps", "star", r, order, it)
    a, b = start.copy(), start.copy()

    def view(arr):
        return _lib.MatrixView(n + 2 * r, n + 2 * r, r, r, n + 2 * r, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    args = _lib.Arguments(n // 8, it, view(a), view(b))
    getattr(lib, fn)(ctypes.byref(args))
    assert lib.stencil_last_error() == 0, lib.stencil_last_error_message()
    sv.comparison(kind)(b if it % 2 else a, want, fn)
    ring = np.ones(start.shape, dtype=bool)
    ring[r:-r, r:-r] = False
    assert bd.same_bits(a[ring], start[ring]) and bd.same_bits(b[ring], start[ring])


# ----------------------------------------------------------------- decay jobs
@pytest.mark.parametrize("dtype,shape,size,sweeps", [("fp32", "star", (140, 9, 7), 70), ("fp32", "star", (120, 9, 7), 56),
                                                     ("fp32", "box", (200, 9, 7), 95), ("fp64", "star", (900, 5, 3), 440)])
def test_decay_into_the_subnormal_range(gpu, dtype, shape, size, sweeps):
    """The reference initial condition (x-ghosts 1, everything else 0) on a long
    thin grid: the front decays through the subnormal range to exact zero on
    its way in, which no other 3D test reaches.  Through AUTO's
    K-step launches, bitwise against the oracle's run."""
    nx, ny, nz = size
    bd.require_bounded(3, dtype, shape, 1, "naive")
    p = ob.problem(3, dtype, shape, 1, "naive", nx, ny, nz)
    want = ob.run(p, sweeps)
    c = sv.census(ob.interior(p, want))
    print(f"{dtype} {shape} {size} after {sweeps}: {c}")
    assert c["subnormal"] >= 100 and c["+0"] + c["-0"] >= 100 and c["nan"] + c["+inf"] + c["-inf"] == 0, c
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype, shape=shape), nx, ny, nz, device=gpu)
    k = e.fuse_steps
    launches, kernel = e.plan(sweeps)
    assert k >= 3 and launches <= sweeps // k + 2, (k, launches)  # K-step launches and at most two remainder launches
    e.reset()
    fin, _ = e.iterate(sweeps)
    bd.assert_bitwise(e.to_numpy(fin), want, f"after {sweeps} sweeps")
