"""The oracle as a judge of subnormal, huge, infinite and NaN cells, on the CPU.

tests/test_gpu_special_values.py compares every kernel family with `ob.sweep`
on the value classes of tests/special_values.py (draw, plant).  That is only
worth something if, in this process,
  * subnormals survive (no library has switched flush-to-zero on),
  * the oracle is a plain restatement of the sweep on such values: it equals a
    numpy model written from its statement order, NaN cells included,
  * every oracle result the GPU file uses is in the regime its class is meant
    to reach (special_values.assert_regime), and
  * the old fields really could not see the mistakes these classes catch.
All four are checked here without a GPU.
"""
import numpy as np
import pytest
import torch

from oracle import binding as ob
from tests import boundary_data as bd
from tests import special_values as sv
from tests.test_oracle_boundary_data import host_engine, numpy_sweeps, reference_ghost_field, shifted

assert torch is not None  # imported on purpose: what it loads must not change the floating-point mode


def _id(key):
    dims, dtype, shape, r, order, size, seed, kind, q, seams, limit, tall = key
    return (f"{dims}d-{dtype}-{shape}-r{r}-{order}-" + "x".join(str(n) for n in size[:dims]) + f"-s{seed}-{kind}"
            + (f"-tall{tall}" if tall else ""))


def problem_of(key):
    dims, dtype, shape, r, order, size, seed, kind, q, seams, limit, tall = key
    nx, ny, nz = size
    return ob.problem(dims, dtype, shape, r, order, nx, ny, nz + 2 * tall)


def slow_of(key):
    return key[5][2] + 2 * key[11] if key[0] == 3 else key[5][1]


def model_sweeps(f, shape, steps, r=1, order="naive"):
    """numpy_sweeps of tests/test_oracle_boundary_data.py (the 3D r = 1 pair) for every stencil the GPU files
    run: a kernel model in numpy alone, written from oracle/oracle_impl.inc's
    statement order with shifted slices, in the field's own dtype with
    avg = T(1) / T(n): `steps` sweeps, reading whatever ghosts `f` holds, of
      * the naive star of radius r, 2D or 3D: 0 + x- (far to near) + x+ + y- + y+ (+ z- + z+), times avg;
      * the DMA order (2D): r = 1: 0.25 * (((up + left) + right) + down); r > 1: 0 + the row window + the column
        window (both with the centre, increasing index), less (centre + centre), times avg;
      * the 3D box: row sums, plane sums and their sum, each starting with its first term, less the centre."""
    T = f.dtype.type
    nd = f.ndim
    inner = (slice(r, -r),) * nd

    def at(a, ax, o):
        offs = [0] * nd
        offs[ax] = o
        return shifted(a, r, offs)

    a = f.copy()
    for _ in range(steps):
        b = a.copy()
        with np.errstate(all="ignore"):
            if shape == "box":
                assert nd == 3
                w = 2 * r + 1
                n = a.shape[2] - 2 * r
                rows = a[:, :, 0:n]
                for d in range(1, w):
                    rows = rows + a[:, :, d:d + n]
                n = a.shape[1] - 2 * r
                planes = rows[:, 0:n]
                for d in range(1, w):
                    planes = planes + rows[:, d:d + n]
                n = a.shape[0] - 2 * r
                acc = planes[0:n]
                for d in range(1, w):
                    acc = acc + planes[d:d + n]
                b[inner] = (acc - a[inner]) * (T(1) / T(w ** 3 - 1))
            elif order == "dma" and r == 1:
                assert nd == 2
                b[inner] = T(0.25) * (((at(a, 0, -1) + at(a, 1, -1)) + at(a, 1, 1)) + at(a, 0, 1))
            elif order == "dma":
                assert nd == 2
                s = np.zeros_like(a[inner])
                for ax in (1, 0):
                    for k in range(-r, r + 1):
                        s = s + at(a, ax, k)
                s = s - (a[inner] + a[inner])
                b[inner] = s * (T(1) / T(2 * nd * r))
            else:
                s = np.zeros_like(a[inner])
                for ax in range(nd - 1, -1, -1):
                    for k in range(r, 0, -1):
                        s = s + at(a, ax, -k)
                    for k in range(1, r + 1):
                        s = s + at(a, ax, k)
                b[inner] = s * (T(1) / T(2 * nd * r))
        a = b
    return a



# ------------------------------------------------------------- environment
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_subnormals_survive_in_numpy(dtype):
    """A product of two small numbers is a non-zero subnormal, scalar and
    array, with torch imported (a library built with fast-math can switch
    flushing on for the whole process when it is loaded)."""
    fi = np.finfo(dtype)
    a = np.full(64, fi.smallest_normal, dtype=dtype)
    b = np.full(64, 0.25, dtype=dtype)
    prod = a * b
    assert prod.dtype == dtype and (prod > 0).all() and (prod < fi.smallest_normal).all()
    assert (prod + prod == a * dtype(0.5)).all()  # subnormal operands are read, not flushed
    tiny = dtype(fi.smallest_subnormal)
    assert tiny > 0 and tiny * dtype(0.5) == 0 and np.signbit(-tiny * dtype(0.25))


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_subnormals_survive_in_the_oracle(dtype, threads):
    """The oracle's sweep of the subnormal field, single- and multi-threaded
    (every OpenMP thread has its own floating-point mode): at least a quarter
    of the result is subnormal, and the threads agree bit for bit."""
    key = next(k for k in sv.SPECIAL if k[:8] == (3, dtype, "star", 1, "naive", (131, 61, 29), 501, "subnormal"))
    p = problem_of(key)
    start = sv.special_start(key)
    got = bd.oracle_steps(p, start, 1, 29, threads)
    c = sv.assert_regime("subnormal", got[1:-1, 1:-1, 1:-1], what=f"{threads} threads")
    print(f"{dtype}, {threads} threads: {100 * c['subnormal'] / got[1:-1, 1:-1, 1:-1].size:.1f} % subnormal")
    bd.assert_bitwise(got, bd.oracle_steps(p, start, 1, 29, 1), "threads")


# -------------------------------------- oracle = numpy model, and the regimes
@pytest.mark.parametrize("shape", ["star", "box"])
def test_model_is_the_earlier_model_where_that_one_is_defined(shape):
    """3D r = 1: model_sweeps is numpy_sweeps bit for bit, on the varying ring and on a subnormal field."""
    for kind in ("normal", "subnormal"):
        f = sv.ring_field((11, 15, 23), 1, 7, np.float64, False, kind=kind)
        assert bd.same_bits(model_sweeps(f, shape, 3), numpy_sweeps(f, shape, 3)), kind


def test_every_gpu_case_has_every_class():
    """Each (dims, dtype, shape, r, order) the GPU files judge by the oracle is
    in the table below with every value class."""
    have = {(k[:5], k[7]) for k in sv.SPECIAL}
    for case in bd.GPU_CASES:
        for kind in sv.KINDS:
            assert (case[:5], kind) in have, (case[:5], kind)


@pytest.mark.parametrize("key", sorted(sv.SPECIAL, key=_id), ids=_id)
def test_oracle_is_the_numpy_model_and_in_its_regime(key):
    """For one start field of the GPU file: every oracle sweep up to the
    largest count used equals the numpy model's sweep of the same grid (NaN
    where the oracle has NaN, every other cell bit for bit), ghosts are never
    written, and at each count the GPU file compares at, the oracle's interior
    meets its class's condition."""
    dims, dtype, shape, r, order, size, seed, kind, q, seams, limit, tall = key
    sweeps = sv.SPECIAL[key]
    p = problem_of(key)
    slow = slow_of(key)
    start = sv.special_start(key)
    inner = (slice(r, -r),) * start.ndim
    ring = np.ones(start.shape, dtype=bool)
    ring[inner] = False
    threads = 8 if start.size > 1 << 20 else 1
    a, b = start.copy(), start.copy()
    first = None
    for n in range(1, max(sweeps) + 1):
        ob.sweep(p, a, b, 0, slow, threads)
        # a halo layout's host-only outermost planes aside, the model sweeps the same grid
        sv.assert_same_values(b, model_sweeps(a, shape, 1, r, order), f"sweep {n}: oracle against the numpy model")
        a, b = b, a
        assert bd.same_bits(a[ring], start[ring]), "the oracle wrote a ghost cell"
        if n == 1:
            first = a[inner].copy()
        if n in sweeps:
            res = a[inner][tall:a[inner].shape[0] - tall] if tall else a[inner]
            c = sv.assert_regime(kind, res, first, f"after {n} sweeps", shape, r, order, n)
            if kind == "wide":  # the operands' spread, whatever the stencil does with it
                assert sv.spread_log2(start[inner]) >= (40 if dtype == "fp32" else 300)
            if kind in sv.NAN_FREE_KINDS:
                assert c["nan"] == 0 and c["+inf"] + c["-inf"] == 0, c
            print(f"{_id(key)} after {n}: {c}")


@pytest.mark.parametrize("kind", sv.KINDS)
@pytest.mark.parametrize("dims,dtype,shape,r,size,seed,halo", [(3, "fp64", "star", 1, (131, 61, 29), 501, 0),
                                                               (3, "fp32", "box", 1, (131, 61, 29), 503, 4),
                                                               (2, "fp32", "star", 4, (301, 170, 1), 601, 0)])
def test_filled_grids_hold_the_tables_field(kind, dims, dtype, shape, r, size, seed, halo):
    """poison_and_fill on host tensors in the device layout: the dense array it
    returns and the one grid a holds are special_start() of the table's entry
    (what this file judges the oracle on), in a halo layout too; grid b holds a
    field of its own, and all padding is poison."""
    from stencil_amd import _lib
    e = host_engine(dims, dtype, shape, r, size, halo=halo, flags=(_lib.HALO_LO | _lib.HALO_HI) if halo else 0)
    sc = sv.special_case(dims, dtype, shape, r, "naive", size, seed, kind, halo)
    key = next(k for k in sv.SPECIAL if k[:8] == (dims, dtype, shape, r, "naive", size, seed, kind) and k[11] == halo)
    want = sv.special_start(key)
    got = sv.poison_and_fill(e, seed, shape == "star", same_ghosts=False, kind=kind, q=sc["q"], seams=sc["seams"],
                             limit=sc["limit"])
    assert bd.same_bits(got, want)
    held = bd.box_view(e, e.a, halo if halo else None).numpy()
    assert bd.same_bits(held, want[r:-r] if halo else want)
    assert not bd.same_bits(bd.box_view(e, e.b, halo if halo else None).numpy(), held)
    assert int(bd.ibits(e.a)[-1]) == bd.nan_pattern(e.torch_dtype)
    assert bd.ring_field is sv._normal_field  # put back


# ------------------------------------------------------------------- teeth
def flushed(a):
    """Subnormals replaced by zeros of their sign."""
    out = a.copy()
    small = np.abs(a) < np.finfo(a.dtype).smallest_normal
    out[small] = np.copysign(a.dtype.type(0), a[small])
    return out


def wrong_ftz(f, shape, steps, inputs):
    """A kernel that flushes subnormal outputs (and, with `inputs`, what it reads) to zero."""
    a = f.copy()
    inner = (slice(1, -1),) * f.ndim
    for _ in range(steps):
        b = model_sweeps(flushed(a) if inputs else a, shape, 1)
        a[inner] = flushed(b[inner])
    return a


def star_everywhere(f):
    """One naive 7-point sweep evaluated at EVERY cell of `f`, ghost positions
    included (what lies beyond the array reads as 0)."""
    g = np.pad(f, 1)
    s = np.zeros_like(f)
    with np.errstate(all="ignore"):
        for ax in (2, 1, 0):
            for o in (-1, 1):
                offs = [0, 0, 0]
                offs[ax] = o
                s = s + shifted(g, 1, offs)
        return s * (f.dtype.type(1) / f.dtype.type(6))


def wrong_blend(f):
    """Two fused sweeps of the 7-point star whose intermediate stage is computed
    at ghost positions too and then restored there by the blend
    m * new + (1 - m) * ghost (m = 1 inside the grid, 0 at ghosts) instead of a
    select."""
    m = np.zeros_like(f)
    m[1:-1, 1:-1, 1:-1] = 1
    with np.errstate(all="ignore"):
        stage = m * star_everywhere(f) + (1 - m) * f
    stage[1:-1, 1:-1, 1:-1] = model_sweeps(f, "star", 1)[1:-1, 1:-1, 1:-1]  # the interior itself is stored exactly
    return model_sweeps(stage, "star", 1)


def teeth_field(dtype, kind, size=(21, 13, 9)):
    """A field without NaN ring edges (a box's ring): every ghost cell and every
    ring edge holds a value, so that the blend model reads no poison."""
    nx, ny, nz = size
    npdt = np.float64 if dtype == "fp64" else np.float32
    if kind == "uniform":
        return reference_ghost_field(size).astype(npdt)
    q = {"overflow": 0.05, "nonfinite": 0.0}.get(kind, 0.0)
    return sv.ring_field((nz + 2, ny + 2, nx + 2), 1, 7, npdt, False, kind=kind, q=q)


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", ["star", "box"])
@pytest.mark.parametrize("inputs", [True, False], ids=["inputs-and-outputs", "outputs-only"])
def test_flush_to_zero_is_seen_by_the_small_classes_only(dtype, shape, inputs):
    """Wrong kernels (a) and (b): subnormals flushed to zero on the way in and
    out, or on the way out only.  Bit-identical to the oracle on the fields
    every earlier test used (uniform [0, 1), standard normal); different on
    `subnormal`, and -- when inputs are flushed -- on `tiny_sparse`."""
    size = (21, 13, 9)
    p = ob.problem(3, dtype, shape, 1, "naive", *size)
    steps = 3
    for kind in ("uniform", "normal", "subnormal", "tiny_sparse"):
        f = teeth_field(dtype, kind)
        want = bd.oracle_steps(p, f, steps, size[2])
        assert bd.same_bits(model_sweeps(f, shape, steps), want), f"the numpy model is not the oracle ({kind})"
        got = wrong_ftz(f, shape, steps, inputs)
        sees = kind == "subnormal" or (kind == "tiny_sparse" and inputs)
        if kind in ("uniform", "normal"):
            assert bd.same_bits(got, want), f"the {kind} field sees flushing after all"
        elif sees:
            assert not bd.same_bits(got, want), f"{kind} does not see flushing"


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_blended_ghosts_are_seen_by_the_nan_classes_only(dtype):
    """Wrong kernel (c): ghosts restored by arithmetic at the intermediate
    stage.  0 * new + 1 * ghost is the ghost whenever `new` is finite, so the
    old fields see nothing; with an infinite, NaN or overflowing cell next to
    a face, `new` at the ghost is not finite and the ghost turns NaN."""
    size = (21, 13, 9)
    p = ob.problem(3, dtype, "star", 1, "naive", *size)
    for kind in ("uniform", "normal", "nonfinite", "overflow"):
        f = teeth_field(dtype, kind)
        want = bd.oracle_steps(p, f, 2, size[2])
        sv.assert_same_values(model_sweeps(f, "star", 2), want, f"the numpy model is not the oracle ({kind})")
        got = wrong_blend(f)
        bad = (np.isnan(got) != np.isnan(want)).any() or \
            not bd.same_bits(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0))
        if kind in ("uniform", "normal"):
            assert bd.same_bits(got, want), f"the {kind} field sees the blend after all"
        else:
            assert bad, f"{kind} does not see the blend"
            with pytest.raises(AssertionError, match="cells differ"):
                sv.assert_same_values(got, want, kind)


# ------------------------------------------------ the comparison and the census
def test_assert_same_values_and_census():
    for dt, u in ((np.float32, np.uint32), (np.float64, np.uint64)):
        fi = np.finfo(dt)
        want = np.array([1.0, fi.smallest_subnormal, 0.0, -0.0, np.inf, -np.inf, np.nan, np.nan], dtype=dt)
        assert sv.census(want) == {"normal": 1, "subnormal": 1, "+0": 1, "-0": 1, "+inf": 1, "-inf": 1, "nan": 2}
        got = want.copy()
        got.view(u)[6] ^= u(0x155)                        # another payload
        got[7] = -got[7]                                   # another sign
        assert not bd.same_bits(got, want)
        sv.assert_same_values(got, want, "payloads")
        for i, v in ((2, -0.0), (3, 0.0), (4, -np.inf), (1, 0.0), (6, 1.0), (0, np.nan),
                     (1, 2 * fi.smallest_subnormal)):
            bad = want.copy()
            bad[i] = v
            with pytest.raises(AssertionError, match=rf"1 cells differ, first at \(ghost-padded indices\) \[\[{i}\]\]"):
                sv.assert_same_values(bad, want, "x")


def test_comparing_substitutes_and_restores_the_comparison():
    own = bd.assert_bitwise
    nan_a, nan_b = np.array([np.nan], dtype=np.float32), -np.array([np.nan], dtype=np.float32)
    with sv.comparing(sv.comparison("nonfinite")):
        assert bd.assert_bitwise is sv.assert_same_values
        bd.assert_bitwise(nan_a, nan_b, "payload")
        with pytest.raises(AssertionError):
            with sv.comparing(sv.comparison("wide")):
                assert bd.assert_bitwise is own
                bd.assert_bitwise(nan_a, nan_b, "payload")
        assert bd.assert_bitwise is sv.assert_same_values  # restored after a failure inside
    assert bd.assert_bitwise is own
