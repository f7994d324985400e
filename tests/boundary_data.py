"""Fields whose boundary data varies in every direction, and whole-allocation
write checks, for the engine's padded layout (include/stencil_hip.h
stencil_layout).  A plain helper module: tests/test_gpu_boundary_data.py runs
it on device grids, tests/test_oracle_boundary_data.py on host tensors.

Every parity test before these started from ghosts that are the same in every
row and plane (x-ghosts 1, the rest 0) and from padding that holds 0.  Here
  * every element of both allocations -- row padding, unused ghost planes,
    the 256-B tail -- first gets a quiet NaN with a recognisable payload, so a
    value that leaks from there into a result is seen, and a store there
    changes bits;
  * the interior is a seeded standard normal field and every ghost cell gets
    a value of its own, so a ghost taken from the wrong plane, row or stage,
    or treated as a literal 0 or 1, changes the result;
  * for star stencils the ring cells with two or more coordinates in the
    ghost range (edges and corners, which a star never reads) go back to NaN.
"""
from __future__ import annotations

import numpy as np
import torch

from stencil_amd import _lib

# quiet NaNs (exponent all ones, top mantissa bit set) with a payload no arithmetic produces
NAN_BITS = {torch.float32: 0x7FC0BEEF, torch.float64: 0x7FF8DEADBEEFCAFE}
INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64}

# Every (dims, dtype, shape, radius, order) tests/test_gpu_boundary_data.py judges by the oracle, each with
# one of the grid sizes it runs there.  That file refuses to build an engine for a tuple that is not listed
# (`require_bounded`), and tests/test_oracle_boundary_data.py bounds the oracle's error for every entry, so
# the two cannot drift apart.
GPU_CASES = ([(2, dt, "star", r, order, (301, 170, 1)) for dt in ("fp32", "fp64") for r in (1, 2, 3, 4, 5)
              for order in ("naive", "dma")]
             + [(2, "fp32", "star", 1, order, (64, 64, 1)) for order in ("naive", "dma")]      # reference ABI
             + [(2, "fp32", "star", 3, order, (96, 96, 1)) for order in ("naive", "dma")]      # reference ABI
             + [(3, dt, shape, 1, "naive", (131, 61, 29)) for dt in ("fp32", "fp64") for shape in ("star", "box")]
             + [(3, dt, shape, r, "naive", (45, 23, 17)) for dt in ("fp32", "fp64")
                for shape, r in (("star", 2), ("star", 3), ("box", 2))])
GPU_CASE_KEYS = frozenset(c[:5] for c in GPU_CASES)


def require_bounded(dims, dtype, shape, r, order) -> None:
    """A GPU case may lean on the oracle only where its error is bounded on the CPU."""
    assert (dims, dtype, shape, r, order) in GPU_CASE_KEYS, \
        f"add {(dims, dtype, shape, r, order)} to boundary_data.GPU_CASES: the oracle's error is not bounded for it"


def _signed(bits: int, width: int) -> int:
    return bits - (1 << width) if bits >= 1 << (width - 1) else bits


def nan_pattern(dtype: torch.dtype) -> int:
    """The poison's bits as the signed integer of the dtype's integer view."""
    return _signed(NAN_BITS[dtype], 32 if dtype == torch.float32 else 64)


def ibits(t: torch.Tensor) -> torch.Tensor:
    return t.view(INT_VIEW[t.dtype])


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                 np.ascontiguousarray(b).view(np.uint8))


def geometry(e) -> dict:
    """Where the logical cells sit in the allocation."""
    lay, r = e.layout, e.r
    three = e.spec.dims == 3
    zg = int(lay.zghost) if three else 0
    row, plane = int(lay.row), int(lay.plane)
    ox = int(lay.origin) - zg * plane - r * row  # padded column of interior x = 0
    assert 0 <= ox - r and ox + int(e.prob.nx) + r <= row
    return {"three": three, "r": r, "zg": zg, "row": row, "plane": plane, "ox": ox, "nx": int(e.prob.nx),
            "ny": int(e.prob.ny), "nz": int(e.prob.nz) if three else 1, "elems": int(lay.elems)}


def box_view(e, grid: torch.Tensor, zdepth: int | None = None) -> torch.Tensor:
    """Strided view of the interior with r ghost cells in x and y and `zdepth`
    planes per side in z (default r; up to the layout's zghost).  2D: the
    (ny + 2r, nx + 2r) box."""
    g = geometry(e)
    r = g["r"]
    base = grid.storage_offset()
    if not g["three"]:
        return grid.as_strided((g["ny"] + 2 * r, g["nx"] + 2 * r), (g["row"], 1), base + g["ox"] - r)
    d = r if zdepth is None else zdepth
    assert 0 <= d <= g["zg"]
    first = (g["zg"] - d) * g["plane"] + g["ox"] - r
    return grid.as_strided((g["nz"] + 2 * d, g["ny"] + 2 * r, g["nx"] + 2 * r), (g["plane"], g["row"], 1), base + first)


def ring_field(shape, r, seed, dtype, star, zr=None) -> np.ndarray:
    """A dense ghost-padded field: standard normal interior (seed), an
    independently drawn ghost ring (seed + 1) in which every ghost cell has
    its own value, and -- for stars -- NaN in every ring cell with two or
    more coordinates in the ghost range.  `shape` is the padded shape; `zr`
    the ghost depth along the first axis of a 3D field (default r)."""
    nd = len(shape)
    depth = [r] * nd
    if nd == 3 and zr is not None:
        depth[0] = zr
    inner = tuple(slice(d, n - d) for d, n in zip(depth, shape))
    f = np.random.default_rng(seed + 1).standard_normal(shape)
    f[inner] = np.random.default_rng(seed).standard_normal(f[inner].shape)
    f = f.astype(dtype)
    if star:
        nghost = np.zeros(shape, dtype=np.int8)
        for ax, (d, n) in enumerate(zip(depth, shape)):
            idx = np.arange(n)
            out = ((idx < d) | (idx >= n - d)).astype(np.int8)
            nghost += out.reshape([-1 if a == ax else 1 for a in range(nd)])
        f[nghost >= 2] = np.nan
        f.view(np.uint32 if f.dtype == np.float32 else np.uint64)[nghost >= 2] = \
            NAN_BITS[torch.float32 if f.dtype == np.float32 else torch.float64]
    return f


def poison_and_fill(e, seed: int, star: bool, same_ghosts: bool = True) -> np.ndarray:
    """Set up e.a and e.b and return e.a's dense start array in the oracle's
    layout.

    Both allocations are filled with the NaN pattern, tail included; then the
    ghost-padded box of each gets ring_field().  same_ghosts: grid b is a copy
    of grid a (what stencil_iterate requires); otherwise b gets a field of its
    own (seed + 1000), interior and ring, so that a launch a -> b shows both
    "ghosts are read from the source" and "ghosts are never written".

    Halo layouts (HALO_LO|HALO_HI with zghost = K planes per side): all zghost
    planes per side are filled, rings included -- they are a neighbour slab's
    interior planes.  The array returned is then the grid the oracle sweeps
    instead: nz + 2 zghost interior planes plus r ghost planes per side that
    exist only on the host (K sweeps later the middle nz planes do not depend
    on them)."""
    g = geometry(e)
    r = g["r"]
    npdt = np.float64 if e.torch_dtype == torch.float64 else np.float32
    flags = int(e.prob.flags)
    halo = g["three"] and (flags & (_lib.HALO_LO | _lib.HALO_HI)) == (_lib.HALO_LO | _lib.HALO_HI)
    assert halo or not flags, "one-sided halo layouts are not covered"
    zd = g["zg"] if halo else r
    dense = None
    for i, grid in enumerate((e.a, e.b)):
        ibits(grid).fill_(nan_pattern(grid.dtype))
        if i == 1 and same_ghosts:
            box_view(e, grid, zd if g["three"] else None).copy_(box_view(e, e.a, zd if g["three"] else None))
            continue
        s = seed + 1000 * i
        if not g["three"]:
            f = ring_field((g["ny"] + 2 * r, g["nx"] + 2 * r), r, s, npdt, star)
            box_view(e, grid).copy_(torch.from_numpy(f))
        elif halo:
            f = ring_field((g["nz"] + 2 * zd + 2 * r, g["ny"] + 2 * r, g["nx"] + 2 * r), r, s, npdt, star)
            box_view(e, grid, zd).copy_(torch.from_numpy(f[r:-r]))
        else:
            f = ring_field((g["nz"] + 2 * r, g["ny"] + 2 * r, g["nx"] + 2 * r), r, s, npdt, star)
            box_view(e, grid, r).copy_(torch.from_numpy(f))
        if i == 0:
            dense = f
    if e.a.is_cuda:
        torch.cuda.synchronize(e.a.device)
    return dense


def dense_of(e, grid: torch.Tensor) -> np.ndarray:
    """Host copy of the grid's ghost-padded box (r ghosts per side), the oracle's layout."""
    if grid.is_cuda:
        torch.cuda.synchronize(grid.device)
    return box_view(e, grid).cpu().numpy().copy()


def locate(e, index: int) -> str:
    """Logical (plane, row, column) of an element of the allocation."""
    g = geometry(e)
    if index >= g["elems"]:
        return f"tail pad element {index - g['elems']} past the grid"
    if g["three"]:
        z, rem = divmod(index, g["plane"])
        y, x = divmod(rem, g["row"])
        return f"(plane {z - g['zg']}, row {y - g['r']}, column {x - g['ox']})"
    y, x = divmod(index, g["row"])
    return f"(row {y - g['r']}, column {x - g['ox']})"


def assert_only_wrote(e, dst_before: torch.Tensor, dst_after: torch.Tensor, begin: int, end: int) -> None:
    """Over the WHOLE allocation, as integers: every element outside the
    interior cells of planes (2D: rows) [begin, end) has the bits it had
    before -- ghost cells, halo planes, the other planes, row padding and the
    tail pad."""
    g = geometry(e)
    assert dst_before.shape == dst_after.shape and dst_before.numel() >= g["elems"]
    changed = ibits(dst_before) != ibits(dst_after)
    own = torch.zeros_like(changed)
    if end > begin:
        if g["three"]:
            first = (g["zg"] + begin) * g["plane"] + g["r"] * g["row"] + g["ox"]
            own.as_strided((end - begin, g["ny"], g["nx"]), (g["plane"], g["row"], 1), first).fill_(True)
        else:
            first = (g["r"] + begin) * g["row"] + g["ox"]
            own.as_strided((end - begin, g["nx"]), (g["row"], 1), first).fill_(True)
    stray = changed & ~own
    n = int(stray.sum().item())
    if n:
        i = int(torch.nonzero(stray)[0].item())
        raise AssertionError(f"{n} elements outside the interior of [{begin}, {end}) were written; first at "
                             f"{locate(e, i)}: {int(ibits(dst_before)[i].item()):#x} -> "
                             f"{int(ibits(dst_after)[i].item()):#x}")


def assert_untouched(e, before: torch.Tensor, after: torch.Tensor, what: str = "source grid") -> None:
    """The whole allocation is bit-identical (a launch's source grid)."""
    changed = ibits(before) != ibits(after)
    n = int(changed.sum().item())
    if n:
        i = int(torch.nonzero(changed)[0].item())
        raise AssertionError(f"{what}: {n} elements changed; first at {locate(e, i)}")


def assert_bitwise(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """Equal bits, NaN payloads included; reports the first cells that differ."""
    assert got.shape == want.shape, (got.shape, want.shape)
    if not same_bits(got, want):
        u = np.uint32 if got.dtype == np.float32 else np.uint64
        diff = np.argwhere(np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u))
        raise AssertionError(f"{what}: {len(diff)} cells differ, first at (ghost-padded indices) {diff[:4].tolist()}")


def oracle_steps(p, start: np.ndarray, steps: int, slow: int, threads: int = 1) -> np.ndarray:
    """`steps` oracle sweeps of the dense field, one at a time (both buffers
    hold the field's ghosts)."""
    from oracle import binding as ob
    a, b = start.copy(), start.copy()
    for _ in range(steps):
        ob.sweep(p, a, b, 0, slow, threads)
        a, b = b, a
    return a
