"""stencil_slab_until_plan: the rounds of one block of stencil_slab_run_until
and whether its check rides in the checking round's launches -- on the host,
no GPU and no job.

With K sweeps per round (as stencil_plan resolves it for the global problem) a
block of `block` sweeps is, checked in the launch, (block - K) sweeps as
stencil_slab_run issues them -- full rounds, one shorter remainder round -- and
one checking round; un-fused it is (block - 1) sweeps issued the same way and
one round of a single sweep.
"""
import ctypes

import pytest

from stencil_amd import _lib
from stencil_amd.engine import StencilSpec, slab_until_plan

SHAPE = (64, 48, 40)


def plan(block, norm="max", **kw):
    spec = StencilSpec(**{**dict(dims=3, dtype="fp64"), **kw})
    got = slab_until_plan(spec, *SHAPE, block, norm, lib=_lib.load(debug=False))
    return got["rounds"], got["fused_check"]


def rounds(block, k, fused):
    before = block - k if fused else block - 1
    return before // k + (1 if before % k else 0) + 1


def test_round_formula():
    assert rounds(100, 4, True) == 25 and rounds(100, 4, False) == 26
    assert rounds(4, 4, True) == 1 and rounds(7, 4, True) == 2
    # 2 sweeps as one remainder round, then the single sweep's round
    assert rounds(3, 4, False) == 2 and rounds(1, 4, False) == 1 and rounds(2, 4, False) == 2


def test_k4_blocks_of_the_7_point_star():
    assert plan(100) == (25, True)
    assert plan(4) == (1, True)
    assert plan(7) == (2, True)
    assert plan(5) == (2, True)
    # shorter than one round: un-fused, block - 1 = 2 sweeps (one remainder round) and the single sweep
    assert plan(3) == (rounds(3, 4, False), False) == (2, False)
    assert plan(1) == (1, False)


def test_the_knob_keeps_the_unfused_check(monkeypatch):
    monkeypatch.setenv("STENCIL_UNTIL_FUSED", "0")
    assert plan(100) == (26, False)
    assert plan(4) == (rounds(4, 4, False), False)


@pytest.mark.parametrize("kw,k", [(dict(norm="l2"), 4), (dict(shape="box", dtype="fp32"), 3), (dict(radius=2), 1),
                                  (dict(kernel="zmarch"), 1), (dict(kernel="temporal2"), 2)])
def test_other_norms_and_families_keep_the_unfused_check(kw, k):
    kw = dict(kw)
    norm = kw.pop("norm", "max")
    for block in (1, 3, 10, 100):
        assert plan(block, norm, **kw) == (rounds(block, k, False), False), (kw, block)


def test_explicit_temporalk_is_fused():
    assert plan(100, kernel="temporalk") == (25, True)


def test_documented_steps_knob(monkeypatch):
    monkeypatch.setenv("STENCIL_TK_STEPS", "3")
    assert plan(3) == (1, True)
    assert plan(100) == (rounds(100, 3, True), True) == (34, True)
    monkeypatch.setenv("STENCIL_TK_STEPS", "5")
    assert plan(4) == (rounds(4, 5, False), False) == (2, False)
    assert plan(100) == (20, True)


def test_fp32_steps_follow_the_job():
    lib = _lib.load(debug=False)
    small = slab_until_plan(StencilSpec(dims=3, dtype="fp32"), 64, 48, 40, 4, lib=lib)
    wide = slab_until_plan(StencilSpec(dims=3, dtype="fp32"), 1024, 1024, 40, 4, lib=lib)  # K = 5 from 1024^2 cells
    assert (small["rounds"], small["fused_check"]) == (1, True)
    assert (wide["rounds"], wide["fused_check"]) == (rounds(4, 5, False), False)


def test_invalid_arguments():
    lib = _lib.load(debug=False)
    f = lib.stencil_slab_until_plan
    out, fused = ctypes.c_int64(), ctypes.c_int32()
    good = _lib.make_problem(dims=3, dtype=_lib.F64, nx=64, ny=48, nz=40)
    assert f(ctypes.byref(good), 10, _lib.NORM_MAX, ctypes.byref(out), ctypes.byref(fused)) == 0
    assert f(ctypes.byref(good), 10, _lib.NORM_MAX, None, None) == 0  # outputs are optional
    assert f(ctypes.byref(good), 0, _lib.NORM_MAX, ctypes.byref(out), ctypes.byref(fused)) == -1
    assert f(ctypes.byref(good), 10, 2, ctypes.byref(out), ctypes.byref(fused)) == -1
    assert f(ctypes.byref(good), 10, -1, ctypes.byref(out), ctypes.byref(fused)) == -1
    assert f(None, 10, _lib.NORM_MAX, ctypes.byref(out), ctypes.byref(fused)) == -1
    # not a slab job's global problem: 2D, a halo, flags, a bad radius
    for kw in (dict(dims=2, nx=64, ny=48, nz=1), dict(halo=4), dict(flags=_lib.HALO_LO), dict(radius=0)):
        bad = _lib.make_problem(**{**dict(dims=3, dtype=_lib.F64, nx=64, ny=48, nz=40), **kw})
        assert f(ctypes.byref(bad), 10, _lib.NORM_MAX, ctypes.byref(out), ctypes.byref(fused)) == -1, kw
        assert lib.stencil_last_error_message()
    with pytest.raises(_lib.StencilError):
        plan(0)


def test_symbols_and_signatures():
    new = ("stencil_sweepk_signal_update_max", "stencil_sweepk_signal_update_max_gated", "stencil_slab_run_until",
           "stencil_slab_until_plan")
    sigs = {**_lib.signatures(), **_lib.slab_until_signatures()}
    for lib in (_lib.load(debug=False), _lib.load(debug=True)):
        for name in new:
            assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
            res, args = sigs[name]
            assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    c, P = ctypes, ctypes.POINTER
    L = P(_lib.Layout)
    assert sigs["stencil_slab_run_until"] == (c.c_int, [c.c_void_p, c.c_uint32, c.c_uint32, c.c_int32, c.c_double,
                                                        P(c.c_uint32), P(c.c_double), P(c.c_int), P(c.c_float)])
    assert sigs["stencil_slab_until_plan"] == (c.c_int, [P(_lib.Problem), c.c_uint32, c.c_int32, P(c.c_int64),
                                                         P(c.c_int32)])
    assert sigs["stencil_sweepk_signal_update_max"][1] == [L, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int32,
                                                           c.c_void_p, c.c_void_p, c.c_void_p, P(c.c_int32), c.c_void_p]
    assert len(sigs["stencil_sweepk_signal_update_max_gated"][1]) == 13
    # the CPU fake device binds every stencil_slab_* name of signatures(): the new ones stay out of it
    assert not any(n in _lib.signatures() for n in ("stencil_slab_run_until", "stencil_slab_until_plan"))
