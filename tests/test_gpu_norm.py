"""Convergence-controlled runs on the GPU: stencil_diff_norms against numpy and
stencil_iterate_until against the CPU oracle.

Every kernel is bitwise the naive sweep, so the update's max norm -- and with
it the sweep count at which a run stops -- is tested for equality.
"""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "build", "bin", "stencil_main")

# dims, (nx, ny, nz), dtype, radius
NORM_SHAPES = [
    (2, (33, 17, 1), "fp32", 1),
    (2, (20, 9, 1), "fp64", 3),
    (3, (67, 29, 11), "fp64", 1),
    (3, (130, 5, 3), "fp32", 1),
    (3, (1, 1, 1), "fp64", 1),
    (3, (3, 2, 2), "fp32", 2),
    # the kernel's other paths: rows wider than the workgroup's 256 vectors (several x steps per row), and units
    # of more than 16 trips, which are cut into chunks (here 18 trips, 2 chunks, the cut inside a row)
    (2, (1030, 3, 1), "fp64", 2),
    (3, (600, 9, 2), "fp64", 1),
    (2, (17413, 3, 1), "fp32", 1),
]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def make_engine(gpu, dims, n, dtype, r, shape="star", order="naive", kernel="auto"):
    from stencil_amd.engine import JacobiEngine, StencilSpec
    return JacobiEngine(StencilSpec(dims=dims, dtype=dtype, shape=shape, radius=r, order=order, kernel=kernel),
                        n[0], n[1], n[2], device=gpu)


def load_junk_grids(e, seed, same_interior=False):
    """Both grids filled whole-allocation with distinct junk (1e30 in a, -7 in
    b, NaN in b's row padding; the tail pad included), interiors from a seeded
    generator.  Returns the interiors as (nz, ny, nx) arrays (nz = 1 in 2D)."""
    import torch
    lay, p, r = e.layout, e.prob, e.r
    dt = np.float64 if e.spec.dtype == "fp64" else np.float32
    planes, rows, row, zg = int(lay.planes), int(lay.rows), int(lay.row), int(lay.zghost)
    ox = int(lay.origin) % row
    nx, ny, nz = int(p.nx), int(p.ny), int(p.nz)
    ha = np.full((planes, rows, row), 1e30, dtype=dt)
    hb = np.full((planes, rows, row), -7.0, dtype=dt)
    pad = np.ones(row, dtype=bool)
    pad[ox - r:ox + nx + r] = False
    hb[:, :, pad] = np.nan
    rng = np.random.default_rng(seed)
    ia = rng.standard_normal((nz, ny, nx)).astype(dt)
    ib = ia.copy() if same_interior else rng.standard_normal((nz, ny, nx)).astype(dt)
    ha[zg:zg + nz, r:r + ny, ox:ox + nx] = ia
    hb[zg:zg + nz, r:r + ny, ox:ox + nx] = ib
    e.a.fill_(1e30)
    e.b.fill_(-7.0)
    e.a[:ha.size].copy_(torch.from_numpy(ha.ravel()))
    e.b[:hb.size].copy_(torch.from_numpy(hb.ravel()))
    torch.cuda.synchronize()
    return ia, ib


def per_unit(e, ia, ib):
    """numpy's per-unit max |d| and the exactly rounded sum of the double
    squares (math.fsum), d = double(a) - double(b)."""
    d = ia.astype(np.float64) - ib.astype(np.float64)
    d = d.reshape(e.slow_extent, -1)
    sq = d * d
    return np.abs(d).max(axis=1), np.array([math.fsum(row) for row in sq]), d.shape[1]


def assert_norms(got_max, got_sum, want_max, want_sum, cells):
    assert same_bits(got_max, want_max)
    # n non-negative terms added in any order stay within about (n - 1) * 2^-53 (relative) of the exact sum, so the
    # bound (2n + 8) * 2^-53 holds for every summation order
    bound = (2 * cells + 8) * 2.0 ** -53
    assert np.all(np.abs(got_sum - want_sum) <= bound * want_sum), (got_sum, want_sum)


# ------------------------------------------------------------- diff_norms
@pytest.mark.parametrize("dims,n,dtype,r", NORM_SHAPES)
def test_diff_norms_match_numpy(gpu, dims, n, dtype, r):
    e = make_engine(gpu, dims, n, dtype, r)
    ia, ib = load_junk_grids(e, 11)
    want_max, want_sum, cells = per_unit(e, ia, ib)
    got_max, got_sum = e.diff_norms(e.a, e.b)
    assert got_max.shape == got_sum.shape == (e.slow_extent,)
    assert_norms(got_max, got_sum, want_max, want_sum, cells)
    ext = e.slow_extent
    for begin, end in {(0, 0), (ext, ext), (ext - 1, ext), (0, 1), (ext // 2, ext), (0, max(1, ext - 1))}:
        m, s = e.diff_norms(e.a, e.b, begin, end)
        assert m.shape == s.shape == (end - begin,)
        assert same_bits(m, got_max[begin:end]) and same_bits(s, got_sum[begin:end])
    assert e.diff_norm(e.a, e.b, "max") == want_max.max()
    assert e.diff_norm(e.a, e.b, "l2") == pytest.approx(math.sqrt(math.fsum(want_sum)), rel=(2 * ia.size + 8) * 2.0 ** -53,
                                                        abs=0)


@pytest.mark.parametrize("dims,n,dtype,r", [NORM_SHAPES[0], NORM_SHAPES[2], NORM_SHAPES[3], NORM_SHAPES[5],
                                            NORM_SHAPES[7], NORM_SHAPES[8]])
def test_single_cell_at_every_interior_corner(gpu, dims, n, dtype, r):
    e = make_engine(gpu, dims, n, dtype, r)
    ia, _ = load_junk_grids(e, 12, same_interior=True)
    nx, ny, nz = n
    corners = sorted({(z, y, x) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)})
    assert len(corners) == (8 if dims == 3 else 4)
    import torch
    for k, (z, y, x) in enumerate(corners):
        view = e.interior(e.b)
        idx = (z, y, x) if dims == 3 else (y, x)
        changed = ia.dtype.type(float(ia[z, y, x]) + 0.5 + k)  # rounded to the grid's format
        view[idx] = float(changed)
        torch.cuda.synchronize()
        d = abs(float(ia[z, y, x]) - float(changed))
        assert d > 0
        m, s = e.diff_norms(e.a, e.b)
        unit = z if dims == 3 else y
        want_m, want_s = np.zeros(e.slow_extent), np.zeros(e.slow_extent)
        want_m[unit], want_s[unit] = d, d * d
        assert same_bits(m, want_m) and same_bits(s, want_s), (z, y, x)
        view[idx] = float(ia[z, y, x])


@pytest.mark.parametrize("dims,n,dtype,r", NORM_SHAPES)
def test_ghost_and_padding_differences_are_not_read(gpu, dims, n, dtype, r):
    """Equal interiors; ghosts, row padding and tail pad differ (1e30 / -7 / NaN)."""
    e = make_engine(gpu, dims, n, dtype, r)
    load_junk_grids(e, 13, same_interior=True)
    m, s = e.diff_norms(e.a, e.b)
    zeros = np.zeros(e.slow_extent)
    assert same_bits(m, zeros) and same_bits(s, zeros)
    m, s = e.diff_norms(e.a, e.a.clone())  # the grid against itself in another allocation
    assert same_bits(m, zeros) and same_bits(s, zeros)


@pytest.mark.parametrize("dims,n,dtype,r", [NORM_SHAPES[0], NORM_SHAPES[2], NORM_SHAPES[3], NORM_SHAPES[7]])
def test_nan_is_sticky_for_its_unit_only(gpu, dims, n, dtype, r):
    import torch
    e = make_engine(gpu, dims, n, dtype, r)
    ia, ib = load_junk_grids(e, 14)
    want_max, want_sum, cells = per_unit(e, ia, ib)
    nx, ny, nz = n
    z, y, x = nz // 2, ny - 1, nx - 1
    e.interior(e.a)[(z, y, x) if dims == 3 else (y, x)] = float("nan")
    torch.cuda.synchronize()
    unit = z if dims == 3 else y
    m, s = e.diff_norms(e.a, e.b)
    assert np.isnan(m[unit]) and np.isnan(s[unit])
    keep = np.arange(e.slow_extent) != unit
    assert not np.isnan(m[keep]).any() and not np.isnan(s[keep]).any()
    assert_norms(m[keep], s[keep], want_max[keep], want_sum[keep], cells)
    assert math.isnan(e.diff_norm(e.a, e.b, "max")) and math.isnan(e.diff_norm(e.a, e.b, "l2"))
    # infinities propagate normally
    e.interior(e.a)[(z, y, x) if dims == 3 else (y, x)] = float("inf")
    torch.cuda.synchronize()
    m, s = e.diff_norms(e.a, e.b)
    assert m[unit] == math.inf and s[unit] == math.inf


def test_same_bits_on_another_stream(gpu):
    import torch
    e = make_engine(gpu, 3, (67, 29, 11), "fp64", 1)
    load_junk_grids(e, 15)
    first = e.diff_norms(e.a, e.b)
    side = torch.cuda.Stream(device=e.device)
    second = e.diff_norms(e.a, e.b, stream=side)
    third = e.diff_norms(e.a, e.b)
    for got in (second, third):
        assert same_bits(got[0], first[0]) and same_bits(got[1], first[1])


def test_invalid_arguments(gpu):
    from stencil_amd import _lib
    e = make_engine(gpu, 3, (20, 12, 6), "fp64", 1)
    e.reset()
    lib, lay = e.lib, ctypes.byref(e.layout)
    a, b = ctypes.c_void_p(e.a.data_ptr()), ctypes.c_void_p(e.b.data_ptr())
    out = (ctypes.c_double * 8)()
    for begin, end in ((-1, 3), (0, 7), (4, 3)):
        assert lib.stencil_diff_norms(lay, a, b, begin, end, out, out, None) == -1
    assert lib.stencil_diff_norms(lay, a, a, 0, 6, out, out, None) == -1
    assert lib.stencil_diff_norms(lay, None, b, 0, 6, out, out, None) == -1
    assert lib.stencil_diff_norms(lay, a, None, 0, 6, out, out, None) == -1
    assert lib.stencil_diff_norms(lay, a, b, 0, 6, None, None, None) == -1
    assert lib.stencil_diff_norms(lay, a, b, 0, 6, out, None, None) == 0
    assert lib.stencil_diff_norms(lay, a, b, 0, 6, None, out, None) == 0

    def until(ga, gb, every=1, norm=_lib.NORM_MAX, tol=1e-3):
        return lib.stencil_iterate_until(lay, ga, gb, 5, every, norm, tol, None, None, None, None, None, None)
    assert until(a, b, every=0) == -1
    assert until(a, b, tol=-1e-9) == -1
    assert until(a, b, tol=float("nan")) == -1
    assert until(a, b, norm=2) == -1 and until(a, b, norm=-1) == -1
    assert until(a, a) == -1 and until(None, b) == -1 and until(a, None) == -1
    assert lib.stencil_last_error_message()
    assert until(a, b) == 0  # every output pointer may be NULL


# ----------------------------------------------------------- iterate_until
CAP = 400
# name: dims, (nx, ny, nz), dtype, shape, radius, order, kernel
UNTIL_CONFIGS = {
    "2d_r1_f32_64": (2, (64, 64, 1), "fp32", "star", 1, "naive", "auto"),
    "2d_r2_dma_f32_40x24": (2, (40, 24, 1), "fp32", "star", 2, "dma", "auto"),
    "3d_7pt_f64_67x29x11": (3, (67, 29, 11), "fp64", "star", 1, "naive", "auto"),
    "3d_7pt_f32_130x20x9": (3, (130, 20, 9), "fp32", "star", 1, "naive", "auto"),
    "3d_box_f32_40x24x9": (3, (40, 24, 9), "fp32", "box", 1, "naive", "auto"),
    "3d_r2_f64_20x12x6": (3, (20, 12, 6), "fp64", "star", 2, "naive", "auto"),
    "2d_persistent_64": (2, (64, 64, 1), "fp32", "star", 1, "naive", "persistent"),
}


def oracle_problem(cfg):
    dims, n, dtype, shape, r, order, _ = UNTIL_CONFIGS[cfg]
    return ob.problem(dims, dtype, shape, r, order, n[0], n[1], n[2])


@functools.lru_cache(maxsize=None)
def oracle_updates(cfg, nan_cell=False):
    """The oracle stepped CAP sweeps from the reference initial condition, once
    per configuration: max |u^n - u^(n-1)| and the L2 norm (exactly rounded sum)
    for n = 1 .. CAP, as lists indexed by n (entry 0 unused)."""
    p = oracle_problem(cfg)
    cur = ob.init(p)
    old = cur.copy()
    ext = p.nz if p.dims == 3 else p.ny
    maxes, l2s = [math.inf], [math.inf]
    for _ in range(CAP):
        ob.sweep(p, cur, old, 0, ext)
        cur, old = old, cur
        d = ob.interior(p, cur).astype(np.float64) - ob.interior(p, old).astype(np.float64)
        maxes.append(float(np.abs(d).max()))
        l2s.append(math.sqrt(math.fsum((d * d).ravel())))
    return maxes, l2s


def expected_stop(norms, tol, every, cap):
    done = 0
    while done < cap:
        done += min(every, cap - done)
        if norms[done] <= tol:
            return done, True
    return done, False


def until_engine(gpu, cfg):
    dims, n, dtype, shape, r, order, kernel = UNTIL_CONFIGS[cfg]
    e = make_engine(gpu, dims, n, dtype, r, shape, order, kernel)
    e.reset()
    return e


@pytest.mark.parametrize("every", [1, 7, 10])
@pytest.mark.parametrize("tol", [1e-2, 1e-3])
@pytest.mark.parametrize("cfg", list(UNTIL_CONFIGS))
def test_iterate_until_stops_where_the_oracle_does(gpu, cfg, tol, every):
    maxes, _ = oracle_updates(cfg)
    count, conv = expected_stop(maxes, tol, every, CAP)
    e = until_engine(gpu, cfg)
    res = e.iterate_until(tol, CAP, check_every=every)
    assert (res.iterations, res.converged) == (count, conv)
    assert res.norm == maxes[count]
    assert res.ms is None
    assert same_bits(e.to_numpy(res.grid), ob.run(oracle_problem(cfg), count))


def test_cap_is_checked_and_reported(gpu):
    cfg = "3d_7pt_f64_67x29x11"
    maxes, _ = oracle_updates(cfg)
    assert maxes[25] > 1e-9
    e = until_engine(gpu, cfg)
    res = e.iterate_until(1e-9, 25, check_every=7, timed=True)
    assert (res.iterations, res.converged, res.norm) == (25, False, maxes[25])
    assert res.ms is not None and res.ms > 0
    assert same_bits(e.to_numpy(res.grid), ob.run(oracle_problem(cfg), 25))


def test_zero_iterations(gpu):
    cfg = "3d_7pt_f64_67x29x11"
    e = until_engine(gpu, cfg)
    res = e.iterate_until(1e-3, 0, check_every=7, timed=True)
    assert (res.iterations, res.converged, res.norm, res.ms) == (0, False, math.inf, 0.0)
    assert res.grid is e.a
    assert same_bits(e.to_numpy(res.grid), ob.run(oracle_problem(cfg), 0))


@pytest.mark.parametrize("cfg", ["3d_7pt_f64_67x29x11", "2d_r1_f32_64"])
def test_l2_norm_stops_where_the_oracle_does(gpu, cfg):
    every = 7
    _, l2s = oracle_updates(cfg)
    checks = list(range(every, CAP + 1, every))
    # tol: the geometric middle of two consecutive check points' norms, about a third of the way down
    k = next(i for i in checks if l2s[i] < l2s[every] / 3)
    tol = math.sqrt(l2s[k - every] * l2s[k])
    count, conv = expected_stop(l2s, tol, every, CAP)
    assert conv and count == k
    # the device's sum of n non-negative squares is within (2n + 8) * 2^-53 of the exact one in any order,
    # its root within half of that plus a rounding: tol must be further from every check's norm
    p = oracle_problem(cfg)
    cells = p.nx * p.ny * p.nz
    bound = (2 * cells + 8) * 2.0 ** -53
    assert all(abs(l2s[i] - tol) > bound * l2s[i] for i in checks if i <= count)
    e = until_engine(gpu, cfg)
    res = e.iterate_until(tol, CAP, check_every=every, norm="l2")
    assert (res.iterations, res.converged) == (count, True)
    assert res.norm == pytest.approx(l2s[count], rel=bound, abs=0)
    assert same_bits(e.to_numpy(res.grid), ob.run(p, count))


def test_interior_nan_stops_at_the_first_check(gpu):
    import torch
    e = until_engine(gpu, "3d_7pt_f64_67x29x11")
    e.interior(e.a)[5, 14, 33] = float("nan")
    torch.cuda.synchronize()
    for norm in ("max", "l2"):
        res = e.iterate_until(1e-3, 50, check_every=7, norm=norm)
        assert (res.iterations, res.converged) == (7, False) and math.isnan(res.norm)
        e.reset()
        e.interior(e.a)[5, 14, 33] = float("nan")
        torch.cuda.synchronize()


# --------------------------------------------------------------------- CLI
def test_cli_hip_stops_where_cpu_does(gpu):
    def count(method):
        p = subprocess.run([CLI, "-s", "64", "-b", "8", "-i", "400", "-m", method, "--tol", "1e-3", "-c"],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert f"The results of method {method} is correct." in p.stdout
        found = re.findall(rf"^\[stencil-amd\] {method}: converged after (\d+) sweeps, ", p.stdout, flags=re.M)
        assert found and len(set(found)) == 1
        return int(found[0])
    assert count("HIP") == count("CPU")
