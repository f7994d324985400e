"""The full multigrid entry points on the host, no GPU: every argument error of
stencil_restrict_source, stencil_inject_ghosts, stencil_prolong_cubic,
stencil_mg_fmg and stencil_mg_fmg_plan (they fire before a device is touched:
the pointers below are never dereferenced), stencil_mg_fmg_plan against its
formula, and the names in the header / binding / library."""
import ctypes
import os
import re

import pytest

from stencil_amd import _lib
from stencil_amd import multigrid as mgm
from stencil_amd.engine import StencilSpec
from tests import mg_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stencil_restrict_source", "stencil_inject_ghosts", "stencil_prolong_cubic", "stencil_mg_fmg",
         "stencil_mg_fmg_plan")
EINVAL, EUNSUPPORTED = -1, -5
A, B = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
NAN, INF = float("nan"), float("inf")
OUT_OF_SCOPE = [(dict(dims=2, nx=301, ny=301, nz=1), "3D"), (dict(shape=_lib.BOX), "box"), (dict(radius=2), "radius"),
                (dict(halo=3, flags=_lib.HALO_LO), "halo"), (dict(kernel=_lib.KERNEL_DIRECT), "kernel")]


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


def rsource(lf, lc, g=A, gc=B, cb=0, ce=None):
    ce = (int(lc.prob.nz) if lc is not None else 0) if ce is None else ce
    return lib().stencil_restrict_source(ref(lf), g, ref(lc), gc, cb, ce, None)


def inject(lf, lc, u=A, uc=B):
    return lib().stencil_inject_ghosts(ref(lf), u, ref(lc), uc, None)


def cubic(lc, lf, e=A, u=B, b=0, en=None):
    en = (int(lf.prob.nz) if lf is not None else 0) if en is None else en
    return lib().stencil_prolong_cubic(ref(lc), e, ref(lf), u, b, en, None)


def fplan(p, levels=0, par=None, cycles=2):
    n, lv = ctypes.c_int64(-1), ctypes.c_int32(-1)
    rc = lib().stencil_mg_fmg_plan(ref(p), levels, ref(par if par is not None else params()), cycles, ctypes.byref(n),
                                   ctypes.byref(lv))
    return rc, n.value, lv.value


def test_names():
    header = open(os.path.join(ROOT, "include", "stencil_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib(), name) and name in _lib.mg_signatures()
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    for name in ("restrict_source", "inject_ghosts", "prolong_cubic", "fmg_plan"):
        assert callable(getattr(mgm, name))
    assert callable(mgm.PoissonMultigrid.fmg) and callable(mgm.PoissonMultigrid.fmg_plan)


@pytest.mark.parametrize("kw,word", OUT_OF_SCOPE)
def test_eunsupported_names_the_restriction(kw, word):
    p = problem(**kw)
    lay = _lib.make_layout(p)
    good_f, good_c = layout(), layout(nx=15, ny=7, nz=3)
    calls = (lambda: rsource(lay, good_c), lambda: rsource(good_f, lay), lambda: inject(lay, good_c),
             lambda: inject(good_f, lay), lambda: cubic(lay, good_f), lambda: cubic(good_c, lay), lambda: fplan(p)[0])
    for call in calls:
        assert call() == EUNSUPPORTED
        assert word in msg() and "multigrid" in msg(), msg()


def test_transfer_einval():
    lf, lc = layout(), layout(nx=15, ny=7, nz=3)
    lf32, lc32 = layout(dtype=_lib.F32), layout(dtype=_lib.F32, nx=15, ny=7, nz=3)
    assert rsource(lf, lc, ce=0) == 0 and cubic(lc, lf, en=0) == 0          # empty ranges: nothing to launch
    assert rsource(lf32, lc32, cb=2, ce=2) == 0 and cubic(lc32, lf32, b=7, en=7) == 0
    for other in (layout(nx=15, ny=7, nz=4), layout(nx=16, ny=7, nz=3), layout(nx=15, ny=6, nz=3), lf):
        for rc in (rsource(lf, other), inject(lf, other), cubic(other, lf)):
            assert rc == EINVAL and "coarsening" in msg(), msg()
    even = layout(nx=30, ny=15, nz=7)
    for rc in (rsource(even, lc), inject(even, lc), cubic(lc, even)):
        assert rc == EINVAL and "coarsening" in msg()
    for rc in (rsource(lf, lc32), rsource(lf32, lc), inject(lf, lc32), inject(lf32, lc), cubic(lc32, lf), cubic(lc, lf32)):
        assert rc == EINVAL and "dtype" in msg(), msg()
    bent = _lib.Layout.from_buffer_copy(lc)
    bent.row += 16
    for rc in (rsource(lf, bent), inject(lf, bent), cubic(bent, lf)):
        assert rc == EINVAL and "stencil_layout_init" in msg(), msg()
    for rc in (rsource(None, lc), rsource(lf, None), inject(None, lc), inject(lf, None), cubic(None, lf), cubic(lc, None),
               rsource(lf, lc, g=None), rsource(lf, lc, gc=None), rsource(lf, lc, g=A, gc=A),
               rsource(lf, lc, cb=-1), rsource(lf, lc, ce=4), rsource(lf, lc, cb=2, ce=1),
               inject(lf, lc, u=None), inject(lf, lc, uc=None), inject(lf, lc, u=A, uc=A),
               cubic(lc, lf, e=None), cubic(lc, lf, u=None), cubic(lc, lf, e=A, u=A),
               cubic(lc, lf, b=-1), cubic(lc, lf, en=8), cubic(lc, lf, b=5, en=4)):
        assert rc == EINVAL, msg()
        assert msg()


def test_fmg_and_plan_einval():
    p = problem()
    for par, word in ((params(w=None), "null weights"), (params(period=0), "period"), (params(w=(0.8, NAN)), "weight 1"),
                      (params(w=(INF,)), "weight 0")):
        assert fplan(p, 0, par)[0] == EINVAL and word in msg(), msg()
    assert lib().stencil_mg_fmg_plan(ref(p), 0, None, 2, None, None) == EINVAL
    assert lib().stencil_mg_fmg_plan(None, 0, ref(params()), 2, None, None) == EINVAL
    for levels in (4, -1, 100):   # (31, 15, 7) has 3
        assert fplan(p, levels)[0] == EINVAL and "levels" in msg(), msg()
    big = problem(nx=32767, ny=32767, nz=7)
    assert fplan(big, 1)[0] == EUNSUPPORTED and "relaxed" in msg()
    # a NULL hierarchy is refused before anything else
    assert lib().stencil_mg_fmg(None, ref(params()), 2, None) == EINVAL and "hierarchy" in msg()
    assert lib().stencil_mg_fmg(None, None, 2, None) == EINVAL
    assert lib().stencil_mg_fmg_plan(ref(p), 0, ref(params()), 2, None, None) == 0   # both outputs are optional


def relax_launches(lay, sweeps):
    n = ctypes.c_int64(-1)
    assert lib().stencil_relax_plan(ctypes.byref(lay), sweeps, ctypes.byref(n), None) == 0
    return n.value


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.F64])
@pytest.mark.parametrize("size,levels", [((15, 15, 15), 1), ((15, 15, 15), 2), ((15, 15, 15), 4), ((31, 15, 7), 0),
                                         ((255, 255, 255), 0), ((9, 9, 8), 0)])
def test_plan_is_the_formula(dtype, size, levels):
    """(L-1) source restrictions + (L-1) injections + (L-1) cubic prolongations
    + stencil_relax_plan of the coarsest run + cycles x the launches of a
    V-cycle started at each level l < L-1 (stencil_relax_plan of its runs plus a
    restriction and a prolongation per level below the start but the last)."""
    p = problem(dtype=dtype, nx=size[0], ny=size[1], nz=size[2])
    nlev_want = levels or mr.max_levels(*size)
    shapes = [size]
    for _ in range(nlev_want - 1):
        shapes.append(mr.coarse_size(*shapes[-1]))
    lays = [layout(dtype=dtype, nx=s[0], ny=s[1], nz=s[2]) for s in shapes]
    for pre, post, coarse in ((2, 3, 8), (0, 0, 0), (1, 0, 5), (9, 2, 30)):
        def vcycle_from(start):
            n = 0
            for i in range(start, nlev_want):
                if i == nlev_want - 1:
                    n += relax_launches(lays[i], coarse)
                else:
                    n += relax_launches(lays[i], pre) + relax_launches(lays[i], post) + 2
            return n

        for cycles in (0, 1, 2, 5):
            rc, launches, nlev = fplan(p, levels, params(pre, post, coarse), cycles)
            assert rc == 0 and nlev == nlev_want
            want = 3 * (nlev_want - 1) + relax_launches(lays[-1], coarse)
            want += cycles * sum(vcycle_from(s) for s in range(nlev_want - 1))
            assert launches == want, (pre, post, coarse, cycles, launches, want)
        # a V-cycle from level 0 is stencil_mg_plan's count
        n0 = ctypes.c_int64(-1)
        assert lib().stencil_mg_plan(ref(p), levels, ref(params(pre, post, coarse)), ctypes.byref(n0), None) == 0
        assert n0.value == vcycle_from(0)
    if nlev_want == 1:
        assert fplan(p, levels, params(2, 3, 8), 2)[1] == relax_launches(lays[0], 8)
    spec = StencilSpec(dims=3, dtype="fp64" if dtype == _lib.F64 else "fp32")
    got = mgm.fmg_plan(spec, *size, levels=levels, cycles=2, pre=2, post=3, coarse_sweeps=8, omegas=(0.8, 1.1))
    assert got == {"launches": fplan(p, levels, params(2, 3, 8), 2)[1], "levels": nlev_want}
