"""Value classes for the fields of tests/boundary_data.py, and what goes with
them: the comparison for results that hold NaNs, the census of a result, the
condition each class's oracle result must meet, and the table of cases that
tests/test_gpu_special_values.py (device grids) and
tests/test_oracle_special_values.py (CPU) share.

tests/boundary_data.py varies WHERE values sit: every ghost cell a value of its
own, a star's ring edges and all padding poison NaN.  This module keeps that
structure -- ring_field and poison_and_fill here are boundary_data's with a
`kind` argument, and `kind="normal"` IS boundary_data's field -- and varies
WHAT the values are: subnormal, wide-range, underflowing, overflowing,
non-finite.  All classes are seeded, built in float64 with np.ldexp and cast to
the grid's dtype.
"""
from __future__ import annotations

import contextlib

import numpy as np

from tests import boundary_data as bd

_normal_field = bd.ring_field  # boundary_data's own, whatever poison_and_fill below puts in its place meanwhile

# The first three classes give results without a NaN and are compared with assert_bitwise, the other two with
# assert_same_values.
NAN_FREE_KINDS = ("subnormal", "wide", "tiny_sparse")
NAN_KINDS = ("overflow", "nonfinite")
KINDS = NAN_FREE_KINDS + NAN_KINDS


def draw(kind, shape, rng, dtype, q=0.0) -> np.ndarray:
    """Independent values of one class, built in float64 (np.ldexp) and cast
    to `dtype`:
      normal       standard normal
      subnormal    +-(1 + u) 2^e, e uniform in [minexp - nmant - 2, minexp + 4]: subnormal operands, sums
                   that cross the normal / subnormal border, products that round in the subnormal range
      wide         +-(1 + u) 2^e, e uniform in [minexp - nmant, maxexp - 7]: the whole exponent range in one
                   neighbourhood; no sum of 32 terms overflows
      tiny_sparse  +0, and +-smallest_subnormal in 5 % of the cells: products that underflow to +0 and -0
      overflow     standard normal, a share q of the cells +-max (0.25 + 0.75 u): partial sums overflow
      nonfinite    standard normal, a share q of the cells +inf, -inf or NaN (more are planted, plant())"""
    fi = np.finfo(dtype)
    if kind in ("subnormal", "wide"):
        lo, hi = ((fi.minexp - fi.nmant - 2, fi.minexp + 4) if kind == "subnormal"
                  else (fi.minexp - fi.nmant, fi.maxexp - 7))
        e = rng.integers(lo, hi + 1, size=shape)
        m = 1.0 + rng.random(shape)
        s = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
        return np.ldexp(s * m, e).astype(dtype)
    if kind == "tiny_sparse":
        f = np.zeros(shape)
        hit = rng.random(shape) < 0.05
        s = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
        f[hit] = (s * float(fi.smallest_subnormal))[hit]
        return f.astype(dtype)
    f = rng.standard_normal(shape)
    if kind == "normal":
        return f.astype(dtype)
    hit = rng.random(shape) < q
    s = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    u = rng.random(shape)
    if kind == "overflow":
        f[hit] = (s * float(fi.max) * (0.25 + 0.75 * u))[hit]
        return f.astype(dtype)
    assert kind == "nonfinite", kind
    f[hit] = np.where(u < 1 / 3, np.inf, np.where(u < 2 / 3, -np.inf, np.nan))[hit]
    return f.astype(dtype)


def plant_sites(interior, seams=None, limit=None):
    """Where kernels decide things, as interior coordinates (slow axis first;
    -1 and n are the first ghost cells): the grid's corner cells; a cell of the
    first and of the last column, row and plane; the two cells on either side
    of every seam (seams[axis] = coordinates s: the cells s - 1 and s); and one
    ghost cell on each face.  `limit`: at most so many of them, evenly taken
    (grids too small to stay mostly finite with all of them)."""
    nd = len(interior)
    seams = seams or [()] * nd
    sites = [tuple(c) for c in np.ndindex(*(2,) * nd)]
    sites = [tuple((n - 1) * c for n, c in zip(interior, s)) for s in sites]
    for ax, n in enumerate(interior):
        mid = [m // 3 + 1 for m in interior]
        far = [2 * m // 3 for m in interior]
        for k, s in enumerate(seams[ax]):
            if 0 < s < n:
                at = [(m // 3 + 5 * k + 2 * ax) % m for m in interior]
                for side in (s - 1, s):
                    at[ax] = side
                    sites.append(tuple(at))
        for end, ghost in ((0, -1), (n - 1, n)):
            mid[ax], far[ax] = end, ghost
            sites.append(tuple(mid))
            sites.append(tuple(far))
    sites = list(dict.fromkeys(sites))
    if limit is not None and len(sites) > limit:
        sites = [sites[i * len(sites) // limit] for i in range(limit)]
    return sites


def plant(f, depth, kind, seams=None, limit=None) -> None:
    """Put special cells at plant_sites() of the padded field `f`.  nonfinite:
    +inf, -inf and NaN in turn (ghost cells +-inf only).  overflow: the site
    and every cell within one of it (a block of same-signed values of at least
    0.75 max, so that the first sweep's sum at the site overflows whatever the
    stencil), and beside it in x a block of the other sign, so that the two
    infinities meet in the second sweep; signs in turn."""
    fi = np.finfo(f.dtype)
    interior = tuple(n - 2 * d for n, d in zip(f.shape, depth))
    for i, site in enumerate(plant_sites(interior, seams, limit)):
        ghost = any(c < 0 or c >= n for c, n in zip(site, interior))
        at = tuple(c + d for c, d in zip(site, depth))
        if kind == "nonfinite":
            f[at] = (np.inf, -np.inf)[i % 2] if ghost else (np.inf, -np.inf, np.nan)[i % 3]
        else:
            big = (1, -1)[i % 2] * fi.max * f.dtype.type(0.75 + 0.25 * ((i * 7) % 10) / 10)
            side = 3 if at[-1] + 4 < f.shape[-1] else -3
            for shift, v in ((side, -big), (0, big)):
                block = tuple(slice(max(0, c - 1), c + 2) for c in at[:-1] + (at[-1] + shift,))
                f[block] = v


def ring_field(shape, r, seed, dtype, star, zr=None, kind="normal", q=0.0, seams=None, limit=None) -> np.ndarray:
    """boundary_data.ring_field with a value class: the interior (seed) and
    every ghost cell (seed + 1) drawn independently from `kind` (draw()),
    overflow and nonfinite fields with special cells at plant_sites() (`seams`:
    interior coordinates per axis, slow axis first; `limit`: at most so many),
    and -- for stars -- the ring's edges and corners poison NaN, as there.
    The default kind is boundary_data's own standard normal field."""
    ref = _normal_field(shape, r, seed, dtype, star, zr)
    if kind == "normal":
        return ref
    nd = len(shape)
    depth = [r] * nd
    if nd == 3 and zr is not None:
        depth[0] = zr
    inner = tuple(slice(d, n - d) for d, n in zip(depth, shape))
    f = draw(kind, shape, np.random.default_rng(seed + 1), dtype, q)
    f[inner] = draw(kind, f[inner].shape, np.random.default_rng(seed), dtype, q)
    if kind in NAN_KINDS:
        plant(f, depth, kind, seams, limit)
    poison = np.isnan(ref)  # a standard normal field holds no other NaN: the star's ring edges and corners
    f[poison] = ref[poison]
    assert bd.same_bits(f[poison], ref[poison])  # the poison's payload travels
    return f


@contextlib.contextmanager
def swapped(module, name, value):
    """`module.name` is `value` inside the block (the helpers of
    tests/boundary_data.py and tests/test_gpu_boundary_data.py look their
    field and their comparison up in boundary_data when they are called)."""
    old = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, old)


def comparing(compare):
    """Inside the block the boundary-data checks (check_launch, check_job)
    compare results with `compare` in place of assert_bitwise."""
    return swapped(bd, "assert_bitwise", compare)


def poison_and_fill(e, seed: int, star: bool, same_ghosts: bool = True, kind: str = "normal", q: float = 0.0, seams=None,
                    limit=None) -> np.ndarray:
    """boundary_data.poison_and_fill with the fields of ring_field() above:
    the same poisoning, layouts and return value.  `seams` are interior
    coordinates of the engine's own grid; in a halo layout, whose dense array
    is taller by zghost planes per side, the z seams move up with it."""
    nz = int(e.prob.nz)

    def field(shape, r, s, dtype, is_star, zr=None):
        tall = (shape[0] - 2 * r - nz) // 2 if len(shape) == 3 else 0
        at = (tuple(z + tall for z in seams[0]),) + tuple(seams[1:]) if seams and tall else seams
        return ring_field(shape, r, s, dtype, is_star, zr, kind=kind, q=q, seams=at, limit=limit)

    with swapped(bd, "ring_field", field):
        return bd.poison_and_fill(e, seed, star, same_ghosts)


# ------------------------------------------------------------ comparison, census, regimes
def _uint(a: np.ndarray):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same_values(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """NaN exactly where `want` has NaN, with any payload and sign (x86 and the
    GPU may generate different ones); every other cell bit for bit --
    subnormals, the sign of zero, the sign of infinity.  Reports the first
    cells that differ, as assert_bitwise does."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~wn & (_uint(got) != _uint(want)))
    if bad.any():
        diff = np.argwhere(bad)
        first = tuple(diff[0])
        raise AssertionError(f"{what}: {len(diff)} cells differ, first at (ghost-padded indices) {diff[:4].tolist()}: "
                             f"got {got[first]!r} ({int(_uint(got)[first]):#x}), want {want[first]!r} "
                             f"({int(_uint(want)[first]):#x})")


def comparison(kind):
    """assert_bitwise for the classes whose results hold no NaN."""
    return assert_same_values if kind in NAN_KINDS else bd.assert_bitwise


def census(a: np.ndarray) -> dict:
    """How many cells of `a` are normal, subnormal, +0, -0, +inf, -inf, NaN."""
    fi = np.finfo(a.dtype)
    mag = np.abs(a)
    neg = np.signbit(a)
    with np.errstate(invalid="ignore"):
        out = {"normal": int((np.isfinite(a) & (mag >= fi.smallest_normal)).sum()),
               "subnormal": int(((mag > 0) & (mag < fi.smallest_normal)).sum()),
               "+0": int(((a == 0) & ~neg).sum()), "-0": int(((a == 0) & neg).sum()),
               "+inf": int((a == np.inf).sum()), "-inf": int((a == -np.inf).sum()), "nan": int(np.isnan(a).sum())}
    assert sum(out.values()) == a.size
    return out


def assert_regime(kind, interior: np.ndarray, after_one: np.ndarray | None = None, what: str = "", shape: str = "star",
                  r: int = 1, order: str = "naive", sweeps: int = 0) -> dict:
    """The condition a class's ORACLE result must meet (never the GPU's), so
    that no test passes on a field that has degenerated.  `interior`: the
    result's interior after `sweeps` sweeps; `after_one`: the interior after
    the first sweep (wide only).

      subnormal    at least 25 % of the cells are subnormal
      tiny_sparse  at least one -0 and one +0
      wide         no inf, no NaN; after one sweep the largest |value| is at least 2^40 (fp32) / 2^300 (fp64)
                   times the smallest non-zero one
      overflow, nonfinite   at least one +inf, one -inf and one NaN; at least 25 % of the cells finite

    Two cases cannot meet their condition as stated, whatever the seed:
      * overflow after ONE sweep of a naive star.  The cell is 0 + x1 + ... + xn with finite xi, added in
        sequence: once a partial sum is +inf, adding a finite term keeps it +inf, so inf - inf never forms
        (the DMA order's `c + c` and the box's separable sums do form it).  There the result must hold both
        infinities and NO NaN.
      * wide through the r = 2 box.  Each cell adds 125 operands whose exponents are uniform over the class's
        range, so every sum sits within a few binades of the top of the range (the chance that all 125 lie
        below the top 2^40 is 0.85^125 ~ 2e-9 per cell) and the results cannot spread by 2^40.  There only
        "no inf, no NaN" is asked of the result; tests/test_oracle_special_values.py asks the spread of the
        operands instead."""
    c = census(interior)
    n = interior.size
    finite = n - c["+inf"] - c["-inf"] - c["nan"]
    if kind == "subnormal":
        assert 4 * c["subnormal"] >= n, (what, c)
    elif kind == "tiny_sparse":
        assert c["-0"] >= 1 and c["+0"] >= 1, (what, c)
    elif kind == "wide":
        assert finite == n, (what, c)
        if not (shape == "box" and r >= 2):
            assert after_one is not None
            assert spread_log2(after_one) >= (40 if interior.dtype == np.float32 else 300), (what, spread_log2(after_one))
    elif kind in NAN_KINDS:
        assert c["+inf"] >= 1 and c["-inf"] >= 1 and 4 * finite >= n, (what, c)
        if kind == "overflow" and shape == "star" and order == "naive" and sweeps == 1:
            assert c["nan"] == 0, (what, c)
        else:
            assert c["nan"] >= 1, (what, c)
    return c


def spread_log2(a: np.ndarray) -> float:
    """log2 of the largest finite |value| over the smallest non-zero one."""
    mag = np.abs(a[np.isfinite(a) & (a != 0)]).astype(np.float64)
    return float(np.log2(mag.max()) - np.log2(mag.min()))


# What tests/test_gpu_special_values.py runs, one entry per start field:
#   (dims, dtype, shape, r, order, size, seed, kind, q, seams, limit, tall) -> the sweep counts it compares at
# tests/test_oracle_special_values.py checks, for every entry and count, the oracle against a numpy model and
# the class's condition (assert_regime); the GPU file takes its fields from here (special_case), so a case
# that is not listed cannot be run.  `tall`: planes per z side by which a halo layout's oracle grid is taller.
# Densities q (overflow): 0.05 for the 3D star and 0.002 for the box fill a K-step launch's sweeps with
# overflowing partial sums and leave most cells finite (the box is all NaN within 5 sweeps at 0.02).  Whole
# jobs and wide 2D stars bound the spread by planting alone (q = 0) and by fewer sweeps: after s sweeps a
# planted cell has reached L1 distance s r (star) or the cube of half-width s r (box).
def _seams3(dtype, nz_seams=(5, 7)):
    """(131, 61, 29) and (130, 37, 29): the first x and y seams of the strip kernels' output tiles at K = 3, 4, 5
    (a 64 V x 8 RY region less its ring, tests/test_gpu_update_max.py STRIP) and the forced z-chunks' first
    seams (STENCIL_BOXK_ZCHUNK 5, STENCIL_TK_ZCHUNK 7)."""
    return (tuple(nz_seams), (26, 30, 48), (54, 56, 58) if dtype == "fp64" else (116, 120))


def _seams2(r):
    """(301, 170) under STENCIL_TB2D_K=3: 128 x 64 regions (r <= 2) or 64 x 64 (r = 3, 4) less a ring of 3 r;
    r = 5 runs sweep_direct's 64 x 4 blocks."""
    if r == 5:
        return ((4,), (64,))
    w = 128 if r <= 2 else 64
    return ((64 - 6 * r,), (w - 6 * r,))


def _build_special():
    t = {}

    def add(dims, dtype, shape, r, order, size, seed, kind, sweeps, q=0.0, seams=None, limit=None, tall=0):
        key = (dims, dtype, shape, r, order, size, seed, kind, q, seams, limit, tall)
        t[key] = tuple(sorted(set(t.get(key, ()) + tuple(sweeps))))

    def dens(kind, shape):
        return {"overflow": 0.05 if shape == "star" else 0.002, "nonfinite": 0.0005}.get(kind, 0.0)

    for dtype in ("fp32", "fp64"):
        for kind in KINDS:
            nan = kind in NAN_KINDS
            for shape in ("star", "box"):
                q = dens(kind, shape)
                s3 = _seams3(dtype) if nan else None
                # single launches: the forced families (1..4 sweeps); the strip kernels, the update-max launch
                add(3, dtype, shape, 1, "naive", (130, 37, 29), 505, kind, (1, 2, 3, 4) if shape == "star" else (1, 2),
                    q, s3)
                add(3, dtype, shape, 1, "naive", (131, 61, 29), 501, kind, (2, 3, 4, 5) if shape == "star"
                    else (1, 2, 3, 4), q, s3)
                # halo layouts at the engine's fuse_steps (4 or 5, box 3 or 4; the GPU file asserts that its count is
                # listed): the oracle's grid is taller by K planes per side
                for k in ((4, 5) if shape == "star" else (3, 4)):
                    add(3, dtype, shape, 1, "naive", (131, 61, 29), 503, kind, (k,), q, s3, tall=k)
                # whole jobs: 2 K + 1 sweeps; overflow / nonfinite: STENCIL_TK_STEPS=3 / STENCIL_BOX_STEPS=2, planted
                if nan:
                    add(3, dtype, shape, 1, "naive", (131, 61, 29), 504, kind, (7,) if shape == "star" else (5,), 0.0, s3)
                else:
                    add(3, dtype, shape, 1, "naive", (131, 61, 29), 504, kind, (7, 9, 11))
            # interior tiles: STENCIL_TK_FAST 0 and 5
            add(3, dtype, "star", 1, "naive", (300, 250, 40), 502, kind, (3, 4, 5), dens(kind, "star"),
                ((7,), (48, 96), (54, 58, 116, 120)) if nan else None)
            # sweep_direct's wider stencils, one sweep
            for shape, r in (("star", 2), ("star", 3), ("box", 2)):
                add(3, dtype, shape, r, "naive", (45, 23, 17), 506, kind, (1,), dens(kind, shape),
                    ((8,), (4, 8), (22,)) if nan else None)
            # 2D jobs through AUTO; overflow / nonfinite: STENCIL_TB2D_K=3 and 7 sweeps (r = 5: 3 single sweeps)
            for r in (1, 2, 3, 4, 5):
                for order in ("naive", "dma"):
                    if nan:
                        q2 = {1: 0.002, 2: 0.0005}.get(r, 0.0) if kind == "nonfinite" else 0.0
                        add(2, dtype, "star", r, order, (301, 170, 1), 601, kind, (7,) if r < 5 else (3,), q2, _seams2(r),
                            limit=12 if r >= 4 else None)
                    else:
                        add(2, dtype, "star", r, order, (301, 170, 1), 601, kind, (23,))
            # one workgroup: r = 1..4 at (64, 64), r = 1, 2 at (20, 9) (a wider star leaves no finite cell there)
            for order in ("naive", "dma"):
                for r in (1, 2, 3, 4):
                    add(2, dtype, "star", r, order, (64, 64, 1), 602, kind, (3,) if nan else (7,), limit=6 if nan else None)
                for r in (1, 2):
                    add(2, dtype, "star", r, order, (20, 9, 1), 602, kind, (2,) if nan else (7,),
                        limit={"overflow": 1, "nonfinite": 3}.get(kind))
                # the persistent kernel
                for r in (1, 2):
                    add(2, dtype, "star", r, order, (64, 64, 1), 603, kind, (5,) if nan else (12,),
                        limit=6 if nan else None)
    # the slab job: 2 K + 1 sweeps (K = 4 star fp64; 3 or 4 box fp32), seams where 2 and 3 slabs meet
    for dtype, shape, sweeps in (("fp64", "star", (9,)), ("fp32", "box", (7, 9))):
        for kind in ("subnormal", "nonfinite"):
            add(3, dtype, shape, 1, "naive", (70, 45, 41), 701, kind, sweeps, 0.0,
                ((13, 14, 20, 21, 27, 28), (), ()) if kind == "nonfinite" else None)
    # the reference ABI on host buffers
    for n, r in ((64, 1), (96, 3)):
        for order in ("naive", "dma"):
            for kind in ("subnormal", "nonfinite"):
                add(2, "fp32", "star", r, order, (n, n, 1), 801, kind, (6, 7), limit=6 if kind == "nonfinite" else None)
    return t


SPECIAL = _build_special()


def special_case(dims, dtype, shape, r, order, size, seed, kind, tall=0):
    """The one SPECIAL entry of this field: (q, seams, limit, sweep counts)."""
    hits = [(k, v) for k, v in SPECIAL.items() if k[:8] == (dims, dtype, shape, r, order, tuple(size), seed, kind)
            and k[11] == tall]
    assert len(hits) == 1, f"{len(hits)} entries of special_values.SPECIAL for {(dims, dtype, shape, r, order, size, seed, kind, tall)}"
    key, sweeps = hits[0]
    return {"q": key[8], "seams": key[9], "limit": key[10], "sweeps": sweeps}


def special_start(key) -> np.ndarray:
    """The dense start field of a SPECIAL key: what poison_and_fill returns
    for an engine of that case."""
    dims, dtype, shape, r, order, size, seed, kind, q, seams, limit, tall = key
    nx, ny, nz = size
    padded = (ny + 2 * r, nx + 2 * r) if dims == 2 else (nz + 2 * tall + 2 * r, ny + 2 * r, nx + 2 * r)
    if tall and seams:
        seams = (tuple(z + tall for z in seams[0]),) + tuple(seams[1:])
    return ring_field(padded, r, seed, np.float64 if dtype == "fp64" else np.float32, shape == "star", kind=kind, q=q,
                      seams=seams, limit=limit)
