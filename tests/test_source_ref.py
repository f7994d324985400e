"""tests/source_ref.py, the expectation of every source-term test, pinned on
hand-computed cases: out(c) = fl(fl(sum6 * avg) + src(c)), the sum taken as
(0 + x- + x+ + y- + y+ + z- + z+), and NOT fma(sum6, avg, src).  No GPU."""
import numpy as np
import pytest

from oracle import binding as ob
from tests import source_ref as sr

NP = {"fp32": np.float32, "fp64": np.float64}
UINT = {"fp32": np.uint32, "fp64": np.uint64}


def bits(x, dtype):
    return int(np.array([x], dtype=NP[dtype]).view(UINT[dtype])[0])


@pytest.mark.parametrize("dtype,want_bits", [("fp32", 0x3F155556), ("fp64", 0x3FE2AAAAAAAAAAAA)])
def test_one_cell_with_the_reference_ghosts(dtype, want_bits):
    """1 x 1 x 1 interior, x-ghosts 1, the other ghosts 0, source 1/4:
    sum6 = 2, fl(2 * fl(1/6)) = 2 fl(1/6) exactly, and adding 1/4 lands exactly
    between two numbers of the format -- the add's own rounding (to even) shows."""
    T = NP[dtype]
    p = sr.problem(dtype, 1, 1, 1)
    u = ob.init(p)
    assert u[1, 1, 0] == 1 and u[1, 1, 2] == 1 and u.sum() == 18  # the x-ghost faces, nothing else
    src = np.full_like(u, np.nan)
    src[1, 1, 1] = 0.25
    out = sr.sweep(p, u, src)
    avg = T(1) / T(6)
    step = T(2) * avg
    assert out[1, 1, 1] == step + T(0.25)
    assert bits(out[1, 1, 1], dtype) == want_bits
    # the ghosts are the input's, bit for bit; no src ghost (NaN) reached anything
    out[1, 1, 1] = u[1, 1, 1]
    assert np.array_equal(out, u)
    # a second sweep: the x-ghosts again (the only neighbours), then the source
    out2 = sr.sweeps(p, u, src, 2)
    assert out2[1, 1, 1] == step + T(0.25)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_3x2x2_distinct_values(dtype):
    T = NP[dtype]
    nx, ny, nz = 3, 2, 2
    p = sr.problem(dtype, nx, ny, nz)
    rng = np.random.default_rng(5)
    u = rng.standard_normal((nz + 2, ny + 2, nx + 2)).astype(T)
    src = rng.uniform(-1, 1, u.shape).astype(T)
    avg = T(1) / T(6)

    def by_hand(f, begin, end):
        out = f.copy()
        for z in range(1 + begin, 1 + end):
            for y in range(1, ny + 1):
                for x in range(1, nx + 1):
                    s = T(0)
                    for v in (f[z, y, x - 1], f[z, y, x + 1], f[z, y - 1, x], f[z, y + 1, x], f[z - 1, y, x], f[z + 1, y, x]):
                        s = T(s + v)
                    out[z, y, x] = T(T(s * avg) + src[z, y, x])
        return out

    one = by_hand(u, 0, nz)
    assert np.array_equal(sr.sweep(p, u, src), one)
    assert np.array_equal(sr.sweeps(p, u, src, 3), by_hand(by_hand(one, 0, nz), 0, nz))
    # a plane range: the other plane keeps the input
    part = sr.sweep(p, u, src, 1, 2)
    assert np.array_equal(part, by_hand(u, 1, 2)) and np.array_equal(part[1], u[1])
    # a K-step launch over a range stores the whole grid's K-th sweep there
    k2 = sr.sweepk(p, u, src, 0, 1, 2)
    assert np.array_equal(k2[1, 1:-1, 1:-1], by_hand(one, 0, nz)[1, 1:-1, 1:-1]) and np.array_equal(k2[2], u[2])
    # one literal cell, fp64: (0 + x- + x+ + y- + y+ + z- + z+) / 6 + src at (z, y, x) = (0, 0, 1)
    f = u.astype(np.float64)
    near = float(f[1, 1, 1] + f[1, 1, 3] + f[1, 0, 2] + f[1, 2, 2] + f[0, 1, 2] + f[2, 1, 2]) / 6 + float(src[1, 1, 2])
    assert abs(float(one[1, 1, 2]) - near) <= 8 * np.finfo(T).eps * (1 + abs(near))


def test_until_and_sum_helpers():
    p = sr.problem("fp64", 4, 3, 2)
    u = ob.init(p)
    src = np.full_like(u, 1e-3)
    grid, done, conv, last = sr.until(p, u, src, 0.0, 5, 2)
    assert (done, conv) == (5, False) and np.array_equal(grid, sr.sweeps(p, u, src, 5))
    assert last == sr.update_norm(sr.sweeps(p, u, src, 5), sr.sweeps(p, u, src, 4))
    assert sr.until(p, u, src, 1e300, 50, 7)[1:3] == (7, True)
    assert sr.until(p, u, src, 1.0, 0, 7)[1:] == (0, False, float("inf"))
    bad = src.copy()
    bad[1, 1, 1] = np.nan
    _, done, conv, last = sr.until(p, u, bad, 1e300, 50, 3)
    assert (done, conv) == (3, False) and last != last
    assert sr.interior_sum(u) == 0.0 and sr.interior_sum(sr.sweep(p, u, src)) == pytest.approx(float(
        sr.sweep(p, u, src)[1:-1, 1:-1, 1:-1].sum()), rel=1e-12)


def test_a_contracted_fma_would_differ():
    """On a seeded 37 x 19 x 9 fp32 field, round(float64(sum6) * avg + g) once
    differs from the helper's two roundings in many cells: the parity tests
    catch a kernel that folds the source into the multiply."""
    nx, ny, nz = 37, 19, 9
    p = sr.problem("fp32", nx, ny, nz)
    u = ob.init(p, "random", 11)
    src = np.zeros_like(u)
    src[1:-1, 1:-1, 1:-1] = np.random.default_rng(12).uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    want = sr.sweep(p, u, src)[1:-1, 1:-1, 1:-1]
    s = np.zeros((nz, ny, nx), dtype=np.float32)
    for sl in ((slice(1, -1), slice(1, -1), slice(0, -2)), (slice(1, -1), slice(1, -1), slice(2, None)),
               (slice(1, -1), slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None), slice(1, -1)),
               (slice(0, -2), slice(1, -1), slice(1, -1)), (slice(2, None), slice(1, -1), slice(1, -1))):
        s = s + u[sl]
    avg = np.float32(1) / np.float32(6)
    # the helper's own sum first: two roundings from `s` reproduce it
    assert np.array_equal((s * avg) + src[1:-1, 1:-1, 1:-1], want)
    fused = (s.astype(np.float64) * np.float64(avg) + src[1:-1, 1:-1, 1:-1].astype(np.float64)).astype(np.float32)
    differ = int((fused != want).sum())
    print(f"{differ} of {want.size} cells differ ({100.0 * differ / want.size:.1f} %)")
    assert differ > 0
