"""stencil_sweepk_update_max: the K-step 7-point launch that also reports
max |u^K - u^(K-1)| over the cells it stores, and stencil_iterate_until through
it.

The expectation is always the oracle's: K - 1 and K sweeps from the same start,
the differences taken in double, the maximum over the interior cells of planes
[begin, end).  A maximum does not depend on the order it is taken in, so every
comparison is for equality, and the output grid is compared bit for bit.
"""
import ctypes
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import binding as ob
from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, StencilSpec
from tests import boundary_data as bd
from tests import test_gpu_norm as tn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = _lib.HALO_LO | _lib.HALO_HI
CASES = [(dt, k) for dt in ("fp32", "fp64") for k in (3, 4, 5)]
# StripTile (kernels_strip.hip) of the checking launches, 8 waves each: cells per lane V and rows per wave RY.
# A region is 64 V x 8 RY cells, an output tile the region less a ring of ceil(K / V) lane vectors per x side
# and K rows per y side.  fp32 K = 4 checks in 6-row strips (launch_tkstrip_update_max); the plain launch of
# that shape has 7.
STRIP = {("fp32", 3): (4, 4), ("fp32", 4): (2, 6), ("fp32", 5): (2, 5),
         ("fp64", 3): (2, 4), ("fp64", 4): (1, 7), ("fp64", 5): (1, 5)}
PLAIN_RY = {**{key: v[1] for key, v in STRIP.items()}, ("fp32", 4): 7}


def tile(dtype, k, ry=None):
    v, r = STRIP[dtype, k]
    ry = r if ry is None else ry
    return 64 * v - 2 * (-(-k // v)) * v, 8 * ry - 2 * k


def seam_size(dtype, k, nz=9):
    """Odd nx (an fp32 lane vector is cut at the row's end) and ny that cross a
    tile seam, in the checking and in the plain launch, and end ragged."""
    tx, ty = tile(dtype, k)
    ty = max(ty, tile(dtype, k, PLAIN_RY[dtype, k])[1])
    nx = tx + 11 if (tx + 11) % 2 else tx + 12
    return nx, ty + 5, nz


def test_tile_table():
    assert tile("fp64", 4) == (56, 48) and tile("fp32", 5) == (116, 30) and tile("fp32", 3) == (248, 26)
    for dt, k in CASES:
        nx, ny, _ = seam_size(dt, k)
        tx, ty = tile(dt, k)
        assert nx % 2 == 1 and tx < nx < 2 * tx and ty < ny < 2 * ty


def make_engine(gpu, dtype, size, halo=0, flags=0, kernel="auto"):
    bd.require_bounded(3, dtype, "star", 1, "naive")
    spec = StencilSpec(dims=3, dtype=dtype, shape="star", radius=1, order="naive", kernel=kernel, halo=halo)
    return JacobiEngine(spec, size[0], size[1], size[2], device=gpu, flags=flags)


def oracle_pair(dtype, size, start, k):
    """(u^(K-1), u^K) interiors of the dense start array, by the oracle."""
    nx, ny, nz = size
    p = ob.problem(3, dtype, "star", 1, "naive", nx, ny, start.shape[0] - 2)
    slow = start.shape[0] - 2
    a, b = start.copy(), start.copy()
    for _ in range(k - 1):
        ob.sweep(p, a, b, 0, slow, 1)
        a, b = b, a
    prev = a[1:-1, 1:-1, 1:-1].copy()
    ob.sweep(p, a, b, 0, slow, 1)
    return prev, b[1:-1, 1:-1, 1:-1].copy()


def update(prev, cur):
    with np.errstate(invalid="ignore"):
        return np.abs(cur.astype(np.float64) - prev.astype(np.float64))


def same_value(got, want):
    return (math.isnan(got) and math.isnan(want)) or got == want


def check(e, prev, cur, k, b, en, tall=0, stream=None):
    """One checking launch a -> b over [b, en): the oracle's maximum, u^K bitwise on the range."""
    with np.errstate(invalid="ignore"):
        want = float(update(prev, cur)[tall + b:tall + en].max())
    got = e.sweepk_update_max(e.a, e.b, b, en, k, stream=stream)
    print(f"planes [{b}, {en}) K={k}: got {got!r} want {want!r}")
    assert same_value(got, want), (got, want)
    bd.assert_bitwise(e.interior(e.b)[b:en].cpu().numpy(), cur[tall + b:tall + en], f"u^{k} on [{b}, {en})")
    return got


def zero_grids(e):
    e.a.zero_()
    e.b.zero_()


def poke(e, start, cells, tall=0):
    """Set interior cells (z, y, x) -> value in grid a and in the dense start array."""
    view = e.interior(e.a)
    for (z, y, x), v in cells.items():
        view[z, y, x] = v
        start[1 + tall + z, 1 + y, 1 + x] = v
    torch.cuda.synchronize()


# ------------------------------------------------------------ random fields
@pytest.mark.parametrize("dtype,k", CASES)
@pytest.mark.parametrize("shape", ["seams", "67x29x11"])
def test_random_fields(gpu, dtype, k, shape):
    """Fields with a value of its own in every ghost cell, NaN in all padding:
    whole and inner ranges; the launch stores only the interior of its planes
    and never its source."""
    size = seam_size(dtype, k) if shape == "seams" else (67, 29, 11)
    nx, ny, nz = size
    e = make_engine(gpu, dtype, size)
    start = bd.poison_and_fill(e, 201, True, same_ghosts=False)
    prev, cur = oracle_pair(dtype, size, start, k)
    assert nz - 4 >= k
    if shape == "seams":
        tx, ty = tile(dtype, k)
        assert -(-nx // tx) == 2 and -(-ny // ty) == 2
        assert e.sweepk_geometry(k)["workgroups"] >= 4  # 2 x 2 tiles in the plain launch's shape too
    src0, dst0 = e.a.clone(), e.b.clone()
    for b, en in ((0, nz), (2, nz - 2)):
        e.b.copy_(dst0)
        check(e, prev, cur, k, b, en)
        bd.assert_only_wrote(e, dst0, e.b, b, en)
        bd.assert_untouched(e, src0, e.a)


@pytest.mark.parametrize("dtype,k,size", [("fp64", 4, (67, 29, 41)), ("fp32", 5, (127, 35, 53))])
def test_several_z_chunks_per_tile(gpu, dtype, k, size):
    nx, ny, nz = size
    e = make_engine(gpu, dtype, size)
    start = bd.poison_and_fill(e, 202, True, same_ghosts=False)
    prev, cur = oracle_pair(dtype, size, start, k)
    tx, ty = tile(dtype, k)
    tiles = -(-nx // tx) * -(-ny // ty)
    geo = e.sweepk_geometry(k)
    assert geo["packed"] or (0 < geo["zchunk"] < nz and geo["workgroups"] > tiles), geo
    for b, en in ((0, nz), (2, nz - 2)):
        check(e, prev, cur, k, b, en)


# ------------------------------------------------- where the maximum sits
def spike_cells(dtype, k, size):
    """cell -> the range it is launched over."""
    nx, ny, nz = size
    tx, ty = tile(dtype, k)
    whole, inner = (0, nz), (2, nz - 2)
    cells = {(z, y, x): whole for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)}
    cells.update({(nz // 2, 3, tx - 1): whole, (nz // 2, 3, tx): whole})          # both sides of the x seam
    cells.update({(nz // 2, ty - 1, 5): whole, (nz // 2, ty, 5): whole})          # both sides of the y seam
    cells.update({(inner[0], ty + 1, tx + 2): inner, (inner[1] - 1, 2, 7): inner})  # an inner range's end planes
    cells[(nz // 2, ny // 2, nx - 1)] = whole                                      # the row's last cell
    return cells


def spike_start(size, cell, dtype, k=0):
    """Zeros with 1 at `cell`.  A grid corner at K = 5 also gets -1/8 on its
    three in-grid diagonal cells: the corner's zero ghosts absorb half of what
    it receives each sweep, so after four sweeps a lone corner spike has more
    mass on those cells (distance 2) than on the corner, and the maximum would
    not pin the corner's own mask."""
    nx, ny, nz = size
    start = np.zeros((nz + 2, ny + 2, nx + 2), dtype=np.float64 if dtype == "fp64" else np.float32)
    z, y, x = cell
    start[1 + z, 1 + y, 1 + x] = 1.0
    if k == 5 and z in (0, nz - 1) and y in (0, ny - 1) and x in (0, nx - 1):
        sz, sy, sx = (1 if z == 0 else -1), (1 if y == 0 else -1), (1 if x == 0 else -1)
        for dz, dy, dx in ((0, sy, sx), (sz, 0, sx), (sz, sy, 0)):
            start[1 + z + dz, 1 + y + dy, 1 + x + dx] = -0.125
    return start


@pytest.mark.parametrize("dtype,k", CASES)
def test_where_the_maximum_sits(gpu, dtype, k):
    """Zero background and ghosts, one spike (spike_start): the update's maximum sits at the
    spike (odd K: the star has no centre term, so u^(K-1) is non-zero there and
    u^K zero) or next to it (even K).  A cell the launch's store mask and the
    maximum's mask disagree on changes the value."""
    size = seam_size(dtype, k)
    e = make_engine(gpu, dtype, size)
    for cell, (b, en) in spike_cells(dtype, k, size).items():
        start = spike_start(size, cell, dtype, k)
        prev, cur = oracle_pair(dtype, size, start, k)
        d = update(prev, cur)[b:en]
        top = np.argwhere(d == d.max()) + (b, 0, 0)
        assert d.max() > 0
        far = np.abs(top - cell).sum(axis=1).max()
        assert far <= (0 if k % 2 else 1), (cell, top.tolist())  # before the GPU is touched
        zero_grids(e)
        e.interior(e.a).copy_(torch.from_numpy(start[1:-1, 1:-1, 1:-1]))
        torch.cuda.synchronize()
        check(e, prev, cur, k, b, en)


# ------------------------------------------------------ what must not count
@pytest.mark.parametrize("dtype,k", CASES)
def test_planes_outside_the_range_do_not_count(gpu, dtype, k):
    size = seam_size(dtype, k, nz=k + 6)
    nx, ny, nz = size
    b, en = 2, nz - 2
    e = make_engine(gpu, dtype, size)
    zero_grids(e)
    # zero ghosts, a small field in the range, large ones in the planes just below and above it
    rng = np.random.default_rng(207)
    start = np.zeros((nz + 2, ny + 2, nx + 2), dtype=np.float64 if dtype == "fp64" else np.float32)
    start[1 + b:1 + en, 1:-1, 1:-1] = 0.01 * rng.standard_normal((en - b, ny, nx))
    start[b, 1:-1, 1:-1] = 100.0 * rng.standard_normal((ny, nx))
    start[1 + en, 1:-1, 1:-1] = -100.0 * rng.standard_normal((ny, nx))
    e.interior(e.a).copy_(torch.from_numpy(start[1:-1, 1:-1, 1:-1]))
    torch.cuda.synchronize()
    prev, cur = oracle_pair(dtype, size, start, k)
    d = update(prev, cur)
    assert d.max() > d[b:en].max() > 0  # from the oracle alone
    got = check(e, prev, cur, k, b, en)
    assert got < float(d.max())


@pytest.mark.parametrize("dtype,k", CASES)
def test_advanced_halo_planes_do_not_count(gpu, dtype, k):
    """HALO_LO|HALO_HI, halo = K live planes per side: the launch advances them
    in registers on the way and stores none of them."""
    size = seam_size(dtype, k)
    nx, ny, nz = size
    e = make_engine(gpu, dtype, size, halo=k, flags=HALO)
    assert int(e.layout.zghost) == k
    start = bd.poison_and_fill(e, 203, True, same_ghosts=False)  # the tall grid: nz + 2K planes and a host-only ring
    spikes = {(k - 1, 6, 10): 500.0, (k + nz, ny - 2, nx - 1): -700.0}  # tall-grid planes -1 and nz of the slab
    view = bd.box_view(e, e.a, k)
    for (z, y, x), v in spikes.items():
        view[z, 1 + y, 1 + x] = v
        start[1 + z, 1 + y, 1 + x] = v
    torch.cuda.synchronize()
    prev, cur = oracle_pair(dtype, (nx, ny, nz + 2 * k), start, k)
    d = update(prev, cur)
    # the halo planes' own update is the larger one
    assert d.max() > d[k:k + nz].max() > 0
    src0, dst0 = e.a.clone(), e.b.clone()
    got = check(e, prev, cur, k, 0, nz, tall=k)
    assert got < float(d.max())
    bd.assert_only_wrote(e, dst0, e.b, 0, nz)
    bd.assert_untouched(e, src0, e.a)
    e.b.copy_(dst0)
    check(e, prev, cur, k, 2, nz - 2, tall=k)


# -------------------------------------------------------------- NaN and inf
@pytest.mark.parametrize("dtype,k", CASES)
def test_nan_and_inf(gpu, dtype, k):
    size = seam_size(dtype, k, nz=2 * k + 8)
    nx, ny, nz = size
    b, en = 2, k + 2
    e = make_engine(gpu, dtype, size)
    base = bd.poison_and_fill(e, 204, True)
    src0 = e.a.clone()
    cell = (0, ny // 2, nx - 1)
    for z, value, kind in ((en, math.nan, "nan"), (en + k, math.nan, "finite"), (en, math.inf, "numpy"),
                           (b + 1, math.inf, "numpy"), (b + 1, math.nan, "nan")):
        e.a.copy_(src0)
        start = base.copy()
        poke(e, start, {(z,) + cell[1:]: value})
        prev, cur = oracle_pair(dtype, size, start, k)
        with np.errstate(invalid="ignore"):
            want = float(update(prev, cur)[b:en].max())
        if kind == "nan":
            assert math.isnan(want)
        elif kind == "finite":
            assert math.isfinite(want) and np.isnan(update(prev, cur)).any()  # NaN beyond the range, out of reach
        else:
            assert not math.isfinite(want)
        check(e, prev, cur, k, b, en)


# ------------------------------------------- accumulation, determinism
def raw_launch(e, word, b, en, k, stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = e.lib.stencil_sweepk_update_max(ctypes.byref(e.layout), ctypes.c_void_p(e.a.data_ptr()),
                                         ctypes.c_void_p(e.b.data_ptr()), b, en, k, ctypes.c_void_p(word.data_ptr()),
                                         ctypes.c_void_p(s.cuda_stream))
    return rc


def as_double(word):
    torch.cuda.synchronize()
    return float(word.cpu().numpy().view(np.float64)[0])


@pytest.mark.parametrize("dtype,k", [("fp64", 4), ("fp32", 5)])
def test_word_accumulates_over_launches(gpu, dtype, k):
    size = seam_size(dtype, k, nz=2 * k + 3)
    nx, ny, nz = size
    e = make_engine(gpu, dtype, size)
    start = bd.poison_and_fill(e, 205, True)
    prev, cur = oracle_pair(dtype, size, start, k)
    d = update(prev, cur)
    lo, hi = float(d[:k].max()), float(d[k:].max())
    assert lo != hi
    for first, second in (((0, k), (k, nz)), ((k, nz), (0, k))):
        word = torch.zeros(1, dtype=torch.int64, device=e.device)
        assert raw_launch(e, word, *first, k) == 0
        assert as_double(word) == float(d[first[0]:first[1]].max())
        assert raw_launch(e, word, *second, k) == 0  # not zeroed in between
        assert as_double(word) == max(lo, hi) == float(d.max())
    # a word already above the result stays, and so does a NaN
    for preset in (float(d.max()) * 4, math.inf, math.nan):
        word = torch.from_numpy(np.array([preset], dtype=np.float64).view(np.int64)).to(e.device)
        bits = int(word.item())
        assert raw_launch(e, word, 0, nz, k) == 0
        torch.cuda.synchronize()
        assert int(word.item()) == bits


@pytest.mark.parametrize("dtype,k", [("fp64", 4), ("fp32", 4)])
def test_same_bits_on_another_stream_and_again(gpu, dtype, k):
    size = (67, 29, 41)
    e = make_engine(gpu, dtype, size)
    start = bd.poison_and_fill(e, 206, True)
    prev, cur = oracle_pair(dtype, size, start, k)
    side = torch.cuda.Stream(device=e.device)
    first = check(e, prev, cur, k, 0, 41)
    torch.cuda.synchronize()
    values = [check(e, prev, cur, k, 0, 41, stream=side)] + [check(e, prev, cur, k, 0, 41) for _ in range(3)]
    assert all(np.float64(v).view(np.uint64) == np.float64(first).view(np.uint64) for v in values)


# -------------------------------------------------------- invalid arguments
def test_invalid_arguments(gpu):
    e = make_engine(gpu, "fp64", (20, 12, 9))
    e.reset()
    word = torch.zeros(1, dtype=torch.int64, device=e.device)
    lay, a, b = ctypes.byref(e.layout), ctypes.c_void_p(e.a.data_ptr()), ctypes.c_void_p(e.b.data_ptr())
    w = ctypes.c_void_p(word.data_ptr())
    f = e.lib.stencil_sweepk_update_max
    assert f(lay, a, b, 0, 9, 4, None, None) == -1  # NULL word
    assert e.lib.stencil_last_error_message()
    assert f(lay, a, b, 0, 9, 2, w, None) == -1 and f(lay, a, b, 0, 9, 6, w, None) == -1
    assert f(lay, a, b, -1, 9, 4, w, None) == -1 and f(lay, a, b, 0, 10, 4, w, None) == -1
    assert f(lay, a, a, 0, 9, 4, w, None) == -1
    assert f(lay, a, b, 0, 9, 4, w, None) == 0
    assert f(lay, a, b, 3, 3, 4, w, None) == 0  # an empty range is a launch of nothing
    torch.cuda.synchronize()
    for spec, n in ((StencilSpec(dims=3, dtype="fp64", shape="box"), (20, 12, 9)),
                    (StencilSpec(dims=3, dtype="fp64", radius=2), (20, 12, 9)),
                    (StencilSpec(dims=2, dtype="fp32"), (64, 64, 1))):
        o = JacobiEngine(spec, n[0], n[1], n[2], device=gpu)
        o.reset()
        rc = o.lib.stencil_sweepk_update_max(ctypes.byref(o.layout), ctypes.c_void_p(o.a.data_ptr()),
                                             ctypes.c_void_p(o.b.data_ptr()), 0, o.slow_extent, 4, w, None)
        assert rc == -5, (spec, rc)
        with pytest.raises(_lib.StencilError):
            o.sweepk_update_max(o.a, o.b, 0, o.slow_extent, 4)
    torch.cuda.synchronize()


# --------------------------------------- iterate_until through the checking launch
FUSED_CONFIGS = ["3d_7pt_f64_67x29x11", "3d_7pt_f32_130x20x9"]
EVERY = [4, 5, 7, 10, 100]
RUNS = [(1e-3, tn.CAP), (1e-12, 23)]  # converging; a cap that leaves a last block of 3, 3, 2, 3 and 23 sweeps


def grid_digest(e, grid):
    return hashlib.sha256(e.to_numpy(grid).tobytes()).hexdigest()


@pytest.mark.parametrize("every", EVERY)
@pytest.mark.parametrize("tol,cap", RUNS)
@pytest.mark.parametrize("cfg", FUSED_CONFIGS)
def test_iterate_until_through_the_checking_launch(gpu, cfg, tol, cap, every):
    maxes, _ = tn.oracle_updates(cfg)
    count, conv = tn.expected_stop(maxes, tol, every, cap)
    e = tn.until_engine(gpu, cfg)
    assert e.fuse_steps == 4
    plan = e.until_plan(every)
    assert plan["fused_check"] and plan["launches"] == e.plan(every - 4)[0] + 1
    assert not e.until_plan(every, "l2")["fused_check"] and not e.until_plan(3)["fused_check"]
    res = e.iterate_until(tol, cap, check_every=every)
    assert (res.iterations, res.converged) == (count, conv)
    assert res.norm == maxes[count]
    assert tn.same_bits(e.to_numpy(res.grid), ob.run(tn.oracle_problem(cfg), count))


CHILD = """
import hashlib, json, sys
import numpy as np
sys.path.insert(0, {root!r})
from tests import test_gpu_norm as tn
out = {{}}
for cfg in {cfgs!r}:
    for tol, cap in {runs!r}:
        for every in {every!r}:
            e = tn.until_engine(0, cfg)
            fused = e.until_plan(every)["fused_check"]
            res = e.iterate_until(tol, cap, check_every=every)
            out[f"{{cfg}}/{{tol}}/{{cap}}/{{every}}"] = [fused, res.iterations, res.converged,
                int(np.float64(res.norm).view(np.uint64)), hashlib.sha256(e.to_numpy(res.grid).tobytes()).hexdigest()]
print(json.dumps(out))
"""


def test_unfused_knob_gives_the_same_run(gpu):
    """STENCIL_UNTIL_FUSED=0 in a fresh process: the old path, with the same
    counts, norm bits and final grids as the checking launches in this one."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("STENCIL_")}
    env["STENCIL_UNTIL_FUSED"] = "0"
    code = CHILD.format(root=ROOT, cfgs=FUSED_CONFIGS, runs=RUNS, every=EVERY)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    old = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(old) == len(FUSED_CONFIGS) * len(RUNS) * len(EVERY)
    for cfg in FUSED_CONFIGS:
        for tol, cap in RUNS:
            for every in EVERY:
                e = tn.until_engine(gpu, cfg)
                assert e.until_plan(every)["fused_check"]
                res = e.iterate_until(tol, cap, check_every=every)
                want = [False, res.iterations, res.converged, int(np.float64(res.norm).view(np.uint64)),
                        grid_digest(e, res.grid)]
                assert old[f"{cfg}/{tol}/{cap}/{every}"] == want, (cfg, tol, cap, every)
