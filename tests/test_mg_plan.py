"""The multigrid entry points on the host, no GPU: stencil_coarsen_problem on
good and bad extents, every argument error that fires before a device is
touched (with messages that name the restriction), stencil_mg_plan against the
sum of stencil_relax_plan plus the transfer launches, and the names in the
header / binding / library."""
import ctypes
import os
import re

import pytest

from stencil_amd import _lib
from stencil_amd import multigrid as mgm
from stencil_amd.engine import StencilSpec
from tests import mg_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stencil_coarsen_problem", "stencil_residual_norms", "stencil_restrict_residual", "stencil_prolong_add",
         "stencil_mg_create", "stencil_mg_destroy", "stencil_mg_levels", "stencil_mg_level", "stencil_mg_upload",
         "stencil_mg_download", "stencil_mg_vcycle", "stencil_mg_solve", "stencil_mg_plan")
EINVAL, EUNSUPPORTED = -1, -5
# never dereferenced: every call below fails its argument checks or has nothing to launch
A, B, C = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
NAN, INF = float("nan"), float("inf")
OUT_OF_SCOPE = [(dict(dims=2, nx=301, ny=301, nz=1), "3D"), (dict(shape=_lib.BOX), "box"), (dict(radius=2), "radius"),
                (dict(halo=3, flags=_lib.HALO_LO), "halo"), (dict(halo=3, flags=_lib.HALO_HI), "halo"),
                (dict(kernel=_lib.KERNEL_DIRECT), "kernel"), (dict(kernel=_lib.KERNEL_ZMARCH), "kernel"),
                (dict(kernel=_lib.KERNEL_TEMPORAL2), "kernel")]


def lib():
    return _lib.load(debug=False)


def msg():
    return lib().stencil_last_error_message().decode()


def problem(**kw):
    base = dict(dims=3, dtype=_lib.F64, nx=31, ny=15, nz=7)
    base.update(kw)
    return _lib.make_problem(**base)


def layout(**kw):
    return _lib.make_layout(problem(**kw))


def ref(x):
    return ctypes.byref(x) if x is not None else None


def params(pre=2, post=3, coarse=8, w=(0.8, 1.1), period=None):
    arr = None if w is None else (ctypes.c_double * max(1, len(w)))(*w)
    p = _lib.MgParams(pre, post, coarse, (len(w) if w is not None else 1) if period is None else period, arr)
    p._keep = arr
    return p


def coarsen(p):
    out = _lib.Problem()
    return lib().stencil_coarsen_problem(ref(p), ctypes.byref(out)), out


def restrict(lf, lc, u=A, g=B, gc=C, cb=0, ce=None):
    ce = (int(lc.prob.nz) if lc is not None else 0) if ce is None else ce
    return lib().stencil_restrict_residual(ref(lf), u, g, ref(lc), gc, cb, ce, None)


def prolong(lc, lf, e=A, u=B, b=0, en=None):
    en = (int(lf.prob.nz) if lf is not None else 0) if en is None else en
    return lib().stencil_prolong_add(ref(lc), e, ref(lf), u, b, en, None)


def norms(lay, u=A, g=B, b=0, en=0, want_max=True, want_sum=True):
    buf = (ctypes.c_double * 64)()
    return lib().stencil_residual_norms(ref(lay), u, g, b, en, buf if want_max else None, buf if want_sum else None, None)


def plan(p, levels=0, par=None):
    n, lv = ctypes.c_int64(-1), ctypes.c_int32(-1)
    rc = lib().stencil_mg_plan(ref(p), levels, ref(par if par is not None else params()), ctypes.byref(n), ctypes.byref(lv))
    return rc, n.value, lv.value


def test_names():
    header = open(os.path.join(ROOT, "include", "stencil_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib(), name) and name in _lib.mg_signatures()
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert "typedef struct stencil_mg_params" in header and ctypes.sizeof(_lib.MgParams) == 24
    # the Python mirror of the kernel's tile constants
    src = open(os.path.join(ROOT, "stencil_amd", "csrc", "kernels_mg.hip")).read()
    tx, ty = (int(re.search(rf"kMg{a} = (\d+)", src).group(1)) for a in ("TX", "TY"))
    assert (tx, ty) == mgm.RESTRICT_TILE and int(re.search(r"kMgZRun = (\d+)", src).group(1)) == mgm.RESTRICT_ZRUN


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.F64])
def test_coarsen_problem(dtype):
    for size in ((31, 15, 7), (7, 5, 3), (3, 3, 3), (511, 255, 127), (131, 61, 29)):
        p = problem(dtype=dtype, nx=size[0], ny=size[1], nz=size[2], kernel=_lib.KERNEL_TEMPORALK)
        rc, c = coarsen(p)
        assert rc == 0 and (c.nx, c.ny, c.nz) == mr.coarse_size(*size)
        assert (c.dims, c.dtype, c.shape, c.radius, c.order, c.kernel, c.halo, c.flags) == \
            (3, dtype, _lib.STAR, 1, _lib.ORDER_NAIVE, _lib.KERNEL_TEMPORALK, 0, 0)
        got = mgm.coarsen_problem(p)
        assert (got.nx, got.ny, got.nz) == (c.nx, c.ny, c.nz)
    for size in ((30, 15, 7), (31, 16, 7), (31, 15, 8), (1, 15, 7), (31, 1, 7), (31, 15, 1), (2, 2, 2), (0, 3, 3)):
        rc, _ = coarsen(problem(dtype=dtype, nx=size[0], ny=size[1], nz=size[2]))
        assert rc == EINVAL and "odd" in msg(), (size, msg())
    assert lib().stencil_coarsen_problem(None, ctypes.byref(_lib.Problem())) == EINVAL
    assert lib().stencil_coarsen_problem(ref(problem()), None) == EINVAL
    with pytest.raises(_lib.StencilError):
        mgm.coarsen_problem(problem(nx=30))


@pytest.mark.parametrize("kw,word", OUT_OF_SCOPE)
def test_eunsupported_names_the_restriction(kw, word):
    p = problem(**kw)
    lay = _lib.make_layout(p)
    good_f, good_c = layout(), layout(nx=15, ny=7, nz=3)
    calls = (lambda: coarsen(p)[0], lambda: norms(lay), lambda: restrict(lay, good_c), lambda: restrict(good_f, lay),
             lambda: prolong(lay, good_f), lambda: prolong(good_c, lay), lambda: plan(p)[0],
             lambda: lib().stencil_mg_create(ref(p), 0, ctypes.byref(ctypes.c_void_p())))
    for call in calls:
        assert call() == EUNSUPPORTED
        assert word in msg() and "multigrid" in msg(), msg()


def test_dma_order_is_unsupported():
    p = _lib.make_problem(dims=2, nx=65, ny=65, nz=1, order=_lib.ORDER_DMA)
    assert coarsen(p)[0] == EUNSUPPORTED and plan(p)[0] == EUNSUPPORTED


def test_transfer_einval():
    lf, lc = layout(), layout(nx=15, ny=7, nz=3)
    lf32, lc32 = layout(dtype=_lib.F32), layout(dtype=_lib.F32, nx=15, ny=7, nz=3)
    assert restrict(lf, lc, ce=0) == 0 and prolong(lc, lf, en=0) == 0          # empty ranges: nothing to launch
    assert restrict(lf32, lc32, cb=2, ce=2) == 0 and prolong(lc32, lf32, b=7, en=7) == 0
    for other in (layout(nx=15, ny=7, nz=4), layout(nx=16, ny=7, nz=3), layout(nx=15, ny=6, nz=3), lf):
        for rc in (restrict(lf, other), prolong(other, lf)):
            assert rc == EINVAL and "coarsening" in msg(), msg()
    even = layout(nx=30, ny=15, nz=7)
    assert restrict(even, layout(nx=15, ny=7, nz=3)) == EINVAL and "coarsening" in msg()
    for rc in (restrict(lf, lc32), restrict(lf32, lc), prolong(lc32, lf), prolong(lc, lf32)):
        assert rc == EINVAL and "dtype" in msg(), msg()
    bent = _lib.Layout.from_buffer_copy(lc)
    bent.row += 16
    for rc in (restrict(lf, bent), prolong(bent, lf), norms(bent)):
        assert rc == EINVAL and "stencil_layout_init" in msg(), msg()
    for rc in (restrict(None, lc), restrict(lf, None), prolong(None, lf), prolong(lc, None),
               restrict(lf, lc, u=None), restrict(lf, lc, g=None), restrict(lf, lc, gc=None),
               restrict(lf, lc, u=A, g=A), restrict(lf, lc, u=A, gc=A), restrict(lf, lc, g=B, gc=B),
               restrict(lf, lc, cb=-1), restrict(lf, lc, ce=4), restrict(lf, lc, cb=2, ce=1),
               prolong(lc, lf, e=None), prolong(lc, lf, u=None), prolong(lc, lf, e=A, u=A),
               prolong(lc, lf, b=-1), prolong(lc, lf, en=8), prolong(lc, lf, b=5, en=4)):
        assert rc == EINVAL, msg()
        assert msg()


def test_residual_norms_einval():
    lay = layout()
    for rc in (norms(None), norms(lay, u=None), norms(lay, g=None), norms(lay, u=A, g=A),
               norms(lay, want_max=False, want_sum=False), norms(lay, b=-1, en=2), norms(lay, b=0, en=8),
               norms(lay, b=4, en=3)):
        assert rc == EINVAL, msg()
        assert msg()


def test_params_and_solve_einval():
    p = problem()
    for par, word in ((params(w=None), "null weights"), (params(period=0), "period"), (params(w=(0.8, NAN)), "weight 1"),
                      (params(w=(INF,)), "weight 0"), (params(w=(0.8, 1.0, -INF)), "weight 2")):
        assert plan(p, 0, par)[0] == EINVAL and word in msg(), msg()
    assert lib().stencil_mg_plan(ref(p), 0, None, None, None) == EINVAL
    assert lib().stencil_mg_plan(None, 0, ref(params()), None, None) == EINVAL
    # a NULL hierarchy is refused before anything else
    par = params()
    assert lib().stencil_mg_vcycle(None, ref(par), None) == EINVAL
    assert lib().stencil_mg_solve(None, ref(par), 3, 1, _lib.NORM_MAX, 1e-3, None, None, None, None, None) == EINVAL
    assert lib().stencil_mg_levels(None, ctypes.byref(ctypes.c_int32())) == EINVAL
    assert lib().stencil_mg_level(None, 0, None, None, None) == EINVAL
    assert lib().stencil_mg_upload(None, A, None, 33, 17, None) == EINVAL
    assert lib().stencil_mg_download(None, A, None, 33, 17, None) == EINVAL
    assert lib().stencil_mg_destroy(None) == 0
    assert lib().stencil_mg_create(ref(p), 0, None) == EINVAL


@pytest.mark.parametrize("size,most", [((15, 15, 15), 4), ((31, 15, 7), 3), ((31, 31, 31), 5), ((30, 15, 7), 1),
                                       ((7, 5, 3), 2), ((511, 511, 511), 9)])
def test_level_counts(size, most):
    p = problem(nx=size[0], ny=size[1], nz=size[2])
    assert mr.max_levels(*size) == most
    assert plan(p, 0)[0] == 0 and plan(p, 0)[2] == most
    for levels in range(1, most + 1):
        assert plan(p, levels)[2] == levels
    for levels in (most + 1, -1, 100):
        assert plan(p, levels)[0] == EINVAL and "levels" in msg(), msg()
        assert lib().stencil_mg_create(ref(p), levels, ctypes.byref(ctypes.c_void_p())) == EINVAL and "levels" in msg()


def test_a_level_the_relaxed_job_cannot_run_is_refused():
    """A plane of 4 GiB or more is beyond the relaxed launches (kernels_strip.hip): the count is refused with a
    message, on the host, whatever the level."""
    p = problem(nx=32767, ny=32767, nz=7)
    assert plan(p, 1)[0] == EUNSUPPORTED and "relaxed" in msg() and "level 0" in msg(), msg()
    assert lib().stencil_mg_create(ref(p), 1, ctypes.byref(ctypes.c_void_p())) == EUNSUPPORTED and "relaxed" in msg()


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.F64])
@pytest.mark.parametrize("size,levels", [((15, 15, 15), 0), ((31, 15, 7), 2), ((31, 31, 31), 4), ((255, 255, 255), 0),
                                         ((9, 9, 8), 0)])
def test_plan_is_the_sum_of_the_relax_plans_plus_the_transfers(dtype, size, levels):
    p = problem(dtype=dtype, nx=size[0], ny=size[1], nz=size[2])
    for pre, post, coarse in ((2, 3, 8), (0, 0, 0), (1, 0, 5), (4, 4, 1), (9, 2, 30)):
        rc, launches, nlev = plan(p, levels, params(pre, post, coarse))
        assert rc == 0 and nlev == (levels or mr.max_levels(*size))
        want, shape = 0, size
        for i in range(nlev):
            lay = layout(dtype=dtype, nx=shape[0], ny=shape[1], nz=shape[2])
            for sweeps in ((coarse,) if i == nlev - 1 else (pre, post)):
                n = ctypes.c_int64(-1)
                assert lib().stencil_relax_plan(ctypes.byref(lay), sweeps, ctypes.byref(n), None) == 0
                want += n.value
            if i < nlev - 1:
                want += 2  # one restriction, one prolongation
                shape = mr.coarse_size(*shape)
        assert launches == want, (pre, post, coarse, launches, want)
    spec = StencilSpec(dims=3, dtype="fp64" if dtype == _lib.F64 else "fp32")
    got = mgm.mg_plan(spec, *size, levels=levels, pre=2, post=3, coarse_sweeps=8, omegas=(0.8, 1.1))
    assert got == {"launches": plan(p, levels, params(2, 3, 8))[1], "levels": levels or mr.max_levels(*size)}
