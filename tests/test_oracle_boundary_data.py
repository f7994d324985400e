"""The oracle as a judge of fields with plane- and row-varying boundary data
(tests/boundary_data.py), on the CPU.

tests/test_gpu_boundary_data.py compares every kernel family bit for bit with
`ob.sweep` on such fields.  That is only worth something if the oracle itself
honours arbitrary ghost values, never writes a ghost, never reads what a
stencil must not read, and if the old uniform-ring fields really could not see
the mistakes the new ones catch.  Those four things are checked here, without
a GPU, together with the slab job's round logic on the fake device and the
helper's own write checks.
"""
import threading

import numpy as np
import pytest
import torch

from oracle import binding as ob
from stencil_amd import _lib
from stencil_amd.engine import SlabJob, StencilSpec
from tests import boundary_data as bd
from tests.cpu_slab import binding as fb

# every (dims, dtype, shape, r, order) tests/test_gpu_boundary_data.py runs, at one of its grid sizes: the GPU
# file asserts that each of its engines is in this list (boundary_data.require_bounded)
CASES = bd.GPU_CASES


def _id(c):
    return f"{c[0]}d-{c[1]}-{c[2]}-r{c[3]}-{c[4]}-" + "x".join(str(n) for n in c[5][:c[0]])


def field(dims, dtype, shape, r, size, seed=7):
    nx, ny, nz = size
    padded = (ny + 2 * r, nx + 2 * r) if dims == 2 else (nz + 2 * r, ny + 2 * r, nx + 2 * r)
    return bd.ring_field(padded, r, seed, np.float64 if dtype == "fp64" else np.float32, shape == "star")


def shifted(f, r, offs):
    """The interior-sized window of `f` displaced by `offs` (one offset per axis)."""
    return f[tuple(slice(r + o, n - r + o) for o, n in zip(offs, f.shape))]


def exact_sweep(f, dims, shape, r, order):
    """One sweep's interior in longdouble, straight from the definition (the
    mean of the neighbours), with no regard for any summation order; also the
    sum of |operand| over every value that enters an addition of `order`, the
    number m of additions and subtractions `order` performs, 1 / avg, and the
    number of operands in that sum."""
    L = f.astype(np.longdouble)
    A = np.abs(L)
    nd = f.ndim
    zero = (0,) * nd
    if shape == "box":
        offs = [o for o in np.ndindex(*(2 * r + 1,) * nd)]
        offs = [tuple(int(v) - r for v in o) for o in offs]
        cube = sum(shifted(L, r, o) for o in offs)
        acube = sum(shifted(A, r, o) for o in offs)
        n = (2 * r + 1) ** nd - 1
        # (P(-r) + ... + P(r)) - centre: w^3 - 1 additions and one subtraction; the centre enters twice
        return (cube - shifted(L, r, zero)) / n, acube + shifted(A, r, zero), n + 1, n, n + 2
    nb = [tuple(s * k if a == ax else 0 for a in range(nd)) for ax in range(nd) for k in range(1, r + 1)
          for s in (-1, 1)]
    total = sum(shifted(L, r, o) for o in nb)
    atotal = sum(shifted(A, r, o) for o in nb)
    n = 2 * nd * r
    if order == "dma" and r == 1:
        return total / n, atotal, 3, n, n  # ((up + left) + right) + down
    if order == "dma":
        # 0 + row window + column window (both with the centre), c + c, one subtraction
        return total / n, atotal + 3 * shifted(A, r, zero), 2 * (2 * r + 1) + 2, n, n + 3
    return total / n, atotal, n, n, n  # 0 + each neighbour


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_sweep_against_longdouble_mean(case):
    """ob.sweep on a poisoned-ring field against the longdouble mean of the
    neighbours:

        |got - exact| <= (m + 1) u (1 + small) avg sum|operands|

    Derivation.  The oracle computes fl(fl(sum) * avg_T) with avg_T = fl(1/n).
    Recursive summation in ANY order satisfies |fl(sum) - sum| <= gamma_k
    sum|x_i| where k is the most roundings one operand passes through (Higham,
    Accuracy and Stability, 4.2), and k <= the number m of additions and
    subtractions the order performs.  Every order here rounds fewer than m
    times on any operand's way: the naive and DMA orders begin with the exact
    `0 + x` (and the DMA r > 1 order's `c + c` is exact as well), and the box's
    separable sums are 6r + 1 deep against m = w^3.  That leaves room for the
    two roundings after the sum, avg_T's own (|avg_T - 1/n| <= u / n; none
    when n is a power of two) and the multiply's, inside m + 1 roundings in
    all, each of relative size u = eps / 2: (1 + u)^(m+1) - 1 <= (m + 1) u
    (1 + small).  The operand sum runs over every value that enters an
    addition, so the DMA r > 1 order counts the centre three times (its two
    windows and the doubled centre it subtracts) and the box twice.  Three is
    the convention this check was specified with, not the rigorous weight:
    the subtracted operand is the exact 2c, so the summation theorem carries
    the centre with weight four.  The bound used here is therefore slightly
    TIGHTER than the theorem's for that order (never looser), which the
    measured errors leave ample room for.
    `small` = 2^-10 holds the second-order term ((m + 1) u <= 126 * 2^-24) and
    the longdouble evaluation's own error (at most m roundings of 2^-64
    against u = 2^-53 in fp64: 2^-11 of the bound).

    Measured on these fields: at most 0.55 of the bound (2D r = 1 DMA fp64),
    2.3 eps mean|operand| (2D r = 2 DMA fp64), i.e. well inside.  Also: the
    destination's ghosts keep their bits, and a star's result is NaN-free
    although every ring cell with two or more ghost coordinates is NaN."""
    dims, dtype, shape, r, order, size = case
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "needs an extended-precision long double"
    nx, ny, nz = size
    p = ob.problem(dims, dtype, shape, r, order, nx, ny, nz)
    src = field(dims, dtype, shape, r, size)
    if shape == "star":
        assert np.isnan(src).any()
    dst = field(dims, dtype, shape, r, size, seed=99)  # its own ghosts and interior
    before = dst.copy()
    slow = nz if dims == 3 else ny
    ob.sweep(p, src, dst, 0, slow)
    inner = tuple(slice(r, -r) for _ in range(src.ndim))
    got = dst[inner]
    assert not np.isnan(got).any()
    ring = np.ones(dst.shape, dtype=bool)
    ring[inner] = False
    assert bd.same_bits(dst[ring], before[ring]), "the oracle wrote a ghost cell"
    exact, asum, m, n, nops = exact_sweep(src, dims, shape, r, order)
    u = np.longdouble(np.finfo(src.dtype).eps) / 2
    bound = (m + 1) * u * (1 + np.longdouble(2.0) ** -10) * asum / n
    err = np.abs(got.astype(np.longdouble) - exact)
    worst = float((err / (2 * u * asum / nops)).max())
    print(f"{_id(case)}: max error {worst:.3f} eps mean|operand|, max error / bound {float((err / bound).max()):.4f}")
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("dims,shape,r,order", [(3, "star", 1, "naive"), (3, "box", 1, "naive"), (3, "star", 2, "naive"),
                                                (2, "star", 2, "dma"), (2, "star", 1, "naive")])
def test_oracle_subrange_leaves_other_units_alone(dims, shape, r, order):
    """A sweep over [b, e) writes the interior of those planes (2D: rows) and
    nothing else, and what it writes equals the full sweep there."""
    size = (37, 19, 13) if dims == 3 else (37, 19, 1)
    nx, ny, nz = size
    slow = nz if dims == 3 else ny
    p = ob.problem(dims, "fp64", shape, r, order, nx, ny, nz)
    src = field(dims, "fp64", shape, r, size)
    full = field(dims, "fp64", shape, r, size, seed=99)
    part = full.copy()
    before = full.copy()
    ob.sweep(p, src, full, 0, slow)
    b, e = 3, slow - 4
    ob.sweep(p, src, part, b, e)
    assert bd.same_bits(part[r + b:r + e], full[r + b:r + e])
    assert bd.same_bits(part[:r + b], before[:r + b]) and bd.same_bits(part[r + e:], before[r + e:])


# ------------------------------------------------------------------- teeth
def reference_ghost_field(shape3, seed=5):
    """The old tests' field: random interior, x-ghosts 1, every other ghost 0."""
    nx, ny, nz = shape3
    f = np.zeros((nz + 2, ny + 2, nx + 2))
    f[:, :, 0] = f[:, :, -1] = 1.0
    f[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).random((nz, ny, nx))
    return f


def roll_ring(f, axis):
    """f with its ghost ring displaced by one unit along `axis` (0: planes,
    1: rows): every ghost cell of the other two axes' faces takes the value of
    the ghost cell one unit before it, and the two faces of `axis` itself
    trade places.  The interior is unchanged."""
    others = np.zeros(f.shape, dtype=bool)
    for ax in range(3):
        if ax != axis:
            face = [slice(None)] * 3
            for end in (0, -1):
                face[ax] = end
                others[tuple(face)] = True
    out = f.copy()
    out[others] = np.roll(f, 1, axis=axis)[others]
    lo, hi = [slice(None)] * 3, [slice(None)] * 3
    lo[axis], hi[axis] = 0, -1
    lo, hi = tuple(lo), tuple(hi)
    keep = ~others[lo]
    out[lo][keep] = f[hi][keep]
    out[hi][keep] = f[lo][keep]
    return out


def yz_ghosts(shape):
    """Ghost cells of the y and z faces (x inside the grid)."""
    m = np.zeros(shape, dtype=bool)
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    m[:, :, 0] = m[:, :, -1] = False
    return m


WRONG = {
    "ring rolled by one plane": lambda f: roll_ring(f, 0),
    "ring rolled by one row": lambda f: roll_ring(f, 1),
    "y and z ghosts read as 0": lambda f: np.where(yz_ghosts(f.shape), 0.0, f),
}


def numpy_sweeps(f, shape, steps):
    """A kernel model in numpy alone: `steps` sweeps of the 7-point star in the
    naive order (0 + x- + x+ + y- + y+ + z- + z+, times 1/6) or the box's
    separable sums, reading whatever ghosts `f` holds."""
    a = f.copy()
    for _ in range(steps):
        b = a.copy()
        if shape == "star":
            s = np.zeros_like(a[1:-1, 1:-1, 1:-1])
            for ax in (2, 1, 0):
                for o in (-1, 1):
                    offs = [0, 0, 0]
                    offs[ax] = o
                    s = s + shifted(a, 1, offs)
            b[1:-1, 1:-1, 1:-1] = s * (1.0 / 6.0)
        else:
            rows = (a[:, :, :-2] + a[:, :, 1:-1]) + a[:, :, 2:]
            planes = (rows[:, :-2] + rows[:, 1:-1]) + rows[:, 2:]
            acc = (planes[:-2] + planes[1:-1]) + planes[2:]
            b[1:-1, 1:-1, 1:-1] = (acc - a[1:-1, 1:-1, 1:-1]) * (1.0 / 26.0)
        a = b
    return a


@pytest.mark.parametrize("shape", ["star", "box"])
@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_uniform_ring_is_blind_where_the_varying_ring_sees(shape, wrong):
    """Three wrong kernels, modelled with numpy alone by handing a correct
    sweep the wrong ghosts: the ring rolled by one plane, rolled by one row,
    and y- and z-ghosts read as literal 0.  On the reference-ghost field (the
    only ring any earlier test used) each is BIT-IDENTICAL to the oracle; on
    the varying ring each differs.  (The numpy model with the right ghosts is
    first shown to be the oracle bit for bit on both fields.)"""
    size = (21, 13, 9)
    nx, ny, nz = size
    steps = 3
    p = ob.problem(3, "fp64", shape, 1, "naive", nx, ny, nz)
    old = reference_ghost_field(size)
    new = field(3, "fp64", "box", 1, size)  # every ghost cell its own value, edges and corners included
    inner = (slice(1, -1),) * 3
    for name, f in (("uniform", old), ("varying", new)):
        want = bd.oracle_steps(p, f, steps, nz)
        assert bd.same_bits(numpy_sweeps(f, shape, steps), want), f"the numpy model is not the oracle ({name} ring)"
        got = numpy_sweeps(WRONG[wrong](f), shape, steps)
        if name == "uniform":
            assert bd.same_bits(got[inner], want[inner]), "the old field sees this mistake after all"
        else:
            assert not bd.same_bits(got[inner], want[inner]), "the varying ring does not see this mistake"


# ---------------------------------------------------- the slab rounds (fake device)
needs_fake = pytest.mark.skipif(not fb.available(), reason="tests/cpu_slab/libslab_fake.so not built (run make)")


@pytest.fixture()
def fake():
    lib = fb.load()
    lib.set_k(0)
    lib.set_signal(True)
    lib.set_free_bytes(1 << 40)
    yield lib
    lib.set_k(0)
    lib.set_signal(True)
    lib.set_free_bytes(1 << 40)


SLAB_SHAPES = [("fp64", "star", 4), ("fp32", "star", 5), ("fp64", "box", 4), ("fp32", "box", 3)]


@needs_fake
@pytest.mark.parametrize("dtype,shape,k", SLAB_SHAPES)
@pytest.mark.parametrize("nslabs", [1, 2, 3])
@pytest.mark.parametrize("exchange,devices", [("rccl", "distinct"), ("copy", "distinct"), ("copy", "shared")])
def test_fake_slab_job_keeps_a_varying_ring(fake, dtype, shape, k, nslabs, exchange, devices):
    """csrc/slab_core.hpp's rounds (face-signalled on distinct devices,
    boundary + interior launches on a shared one, remainder rounds) on an
    uploaded poisoned-ring grid, non-rolling: the downloaded grid is the
    oracle's bit for bit, ghosts (and a star's NaN edges) included."""
    fake.set_k(k)
    spec = StencilSpec(dims=3, dtype=dtype, shape=shape)
    nx, ny, nz = 13, 7, 3 * k * nslabs + 2
    p = ob.problem(3, dtype, shape, 1, "naive", nx, ny, nz)
    start = field(3, dtype, shape, 1, (nx, ny, nz), seed=31)
    devs = list(range(nslabs)) if devices == "distinct" else [0] * nslabs
    job = SlabJob(spec, nx, ny, nz, devs, exchange=exchange, lib=fake)
    job.upload(start)
    bd.assert_bitwise(job.download(), start, "upload / download")
    sweeps = 0
    for it in (2 * k + 1, k - 1):
        job.run(it)
        sweeps += it
        bd.assert_bitwise(job.download(), bd.oracle_steps(p, start, sweeps, nz), f"after {sweeps} sweeps")
    job.close()


@needs_fake
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("shape", ["star", "box"])
def test_fake_rank_mode_keeps_a_varying_ring(fake, nranks, shape):
    """Rank mode (one slab per rank, one thread per rank here): each rank
    uploads the global poisoned-ring grid, and the ranks' planes, assembled,
    are the oracle's grid bit for bit, the ring of every plane included."""
    k = 4 if shape == "star" else 3
    fake.set_k(k)
    spec = StencilSpec(dims=3, dtype="fp64", shape=shape)
    nx, ny, nz = 10, 6, 9 * nranks + 1
    sweeps = 2 * k + 3
    p = ob.problem(3, "fp64", shape, 1, "naive", nx, ny, nz)
    start = field(3, "fp64", shape, 1, (nx, ny, nz), seed=33)
    uid = SlabJob.unique_id(lib=fake)
    out, errs = [None] * nranks, [None] * nranks

    def body(r):
        try:
            job = SlabJob(spec, nx, ny, nz, [r], rank=(nranks, r, uid), lib=fake)
            job.upload(start)
            job.run(k + 1)
            job.run(sweeps - k - 1)
            out[r] = (job.info(0), job.download())
            job.close()
        except Exception as exc:  # surfaced below
            errs[r] = exc

    th = [threading.Thread(target=body, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not any(t.is_alive() for t in th), "a rank hung"
    assert not any(errs), errs
    want = bd.oracle_steps(p, start, sweeps, nz)
    got = np.zeros_like(want)
    for r in range(nranks):
        inf, dense = out[r]
        z0 = inf["first"] + (0 if r > 0 else -1)
        z1 = inf["first"] + inf["planes"] + (1 if r == nranks - 1 else 0)
        got[z0 + 1:z1 + 1] = dense[z0 + 1:z1 + 1]
    bd.assert_bitwise(got, want, "assembled ranks")


# ------------------------------------------------- the helper's own write checks
class HostGrids:
    """What the helper uses of a JacobiEngine, with the two grids as host
    tensors in the device layout (the layout rule needs no GPU); the oracle
    plays the kernel."""

    def __init__(self, spec, nx, ny, nz, flags=0):
        self.spec = spec
        self.prob = spec.problem(nx, ny, nz, flags)
        self.layout = _lib.make_layout(self.prob)
        self.r = spec.radius
        self.torch_dtype = torch.float64 if spec.dtype == "fp64" else torch.float32
        n = int(self.layout.elems) + 256 // spec.elem_bytes  # tail pad, as stencil_alloc
        self.a = torch.empty(n, dtype=self.torch_dtype)
        self.b = torch.empty(n, dtype=self.torch_dtype)


def host_engine(dims, dtype, shape, r, size, halo=0, flags=0):
    return HostGrids(StencilSpec(dims=dims, dtype=dtype, shape=shape, radius=r, halo=halo), *size, flags=flags)


@pytest.mark.parametrize("dims,dtype,shape,r", [(3, "fp64", "star", 1), (3, "fp32", "box", 1), (2, "fp32", "star", 2),
                                                (2, "fp64", "star", 5)])
def test_helper_accepts_a_correct_launch_and_locates_stray_stores(dims, dtype, shape, r):
    """poison_and_fill + assert_only_wrote on host tensors: a launch modelled
    by the oracle (interior of [b, e) only) passes; one extra store into a
    ghost cell, another plane, the row padding or the tail pad fails and is
    reported at its logical coordinates."""
    size = (21, 9, 7) if dims == 3 else (21, 9, 1)
    nx, ny, nz = size
    slow = nz if dims == 3 else ny
    e = host_engine(dims, dtype, shape, r, size)
    g = bd.geometry(e)
    start = bd.poison_and_fill(e, 3, shape == "star", same_ghosts=False)
    pat = bd.nan_pattern(e.torch_dtype)
    bits = bd.ibits(e.a)
    assert int(bits[-1]) == pat and int(bits[0]) == pat and int(bits[g["elems"]]) == pat  # padding, tail
    assert bd.same_bits(bd.dense_of(e, e.a), start)
    assert not bd.same_bits(bd.dense_of(e, e.b), start)  # the destination has ghosts of its own
    inner = tuple(slice(r, -r) for _ in range(start.ndim))
    assert not np.isnan(start[inner]).any() and np.isnan(start).any() == (shape == "star")
    ring = start.copy()
    ring[inner] = np.nan
    vals = ring[~np.isnan(ring)]
    assert len(np.unique(vals)) == len(vals), "every ghost cell has its own value"

    p = ob.problem(dims, dtype, shape, r, "naive", nx, ny, nz)
    b, en = 2, slow - 1
    before = e.b.clone()
    dense = bd.dense_of(e, e.b)
    ob.sweep(p, start, dense, b, en)
    bd.box_view(e, e.b).copy_(torch.from_numpy(dense))  # ghosts rewritten with the bits they had
    bd.assert_only_wrote(e, before, e.b, b, en)
    with pytest.raises(AssertionError, match="were written"):
        bd.assert_only_wrote(e, before, e.b, b + 1, en)  # unit b is now outside the launch's range

    origin = int(e.layout.origin)
    unit = g["plane"] if dims == 3 else g["row"]
    where = "plane" if dims == 3 else "row"
    assert g["ox"] > r  # there is row padding left of the ghost columns
    strays = {origin - 1: "column -1", origin + nx: f"column {nx}", origin + en * unit: f"{where} {en},",
              origin - r - 1: f"column -{r + 1}", g["elems"] + 1: "tail pad element 1"}
    for idx, text in strays.items():
        after = e.b.clone()
        bd.ibits(after)[idx] = 12345
        with pytest.raises(AssertionError, match=text):
            bd.assert_only_wrote(e, before, after, b, en)
        with pytest.raises(AssertionError, match="elements changed"):
            bd.assert_untouched(e, e.b, after)
    bd.assert_untouched(e, e.b, e.b.clone())


def test_helper_fills_every_halo_plane():
    """Halo layouts (HALO_LO|HALO_HI, zghost = K): all K planes per side are
    filled, rings included, and the dense array is the taller grid the oracle
    sweeps; without the flags only r ghost planes are, the rest stays NaN."""
    k = 4
    nx, ny, nz = 11, 6, 9
    e = host_engine(3, "fp64", "star", 1, (nx, ny, nz), halo=k, flags=_lib.HALO_LO | _lib.HALO_HI)
    tall = bd.poison_and_fill(e, 5, True)
    assert tall.shape == (nz + 2 * k + 2, ny + 2, nx + 2)
    assert bd.same_bits(bd.box_view(e, e.a, k).numpy(), tall[1:-1])
    assert bd.same_bits(bd.box_view(e, e.b, k).numpy(), tall[1:-1])
    assert not np.isnan(tall[1:-1, 1:-1, :]).any() and not np.isnan(tall[1:-1, :, 1:-1]).any()
    assert np.isnan(tall[1:-1, 0, 0]).all()
    e = host_engine(3, "fp64", "box", 1, (nx, ny, nz), halo=k)
    dense = bd.poison_and_fill(e, 5, False)
    assert dense.shape == (nz + 2, ny + 2, nx + 2) and not np.isnan(dense).any()
    deep = bd.box_view(e, e.a, k).numpy()
    assert np.isnan(deep[:k - 1]).all() and np.isnan(deep[-(k - 1):]).all() and bd.same_bits(deep[k - 1:-(k - 1)], dense)
