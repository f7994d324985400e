"""The relaxed-sweep entry points on the host, no GPU: stencil_relax_plan
against stencil_source_plan, every argument error that fires before a device
is touched (with messages that name the restriction), the names in the header
/ binding / library, and the CLI's --omega / --cheby on the CPU method."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import binding as ob
from stencil_amd import _lib
from tests import relax_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "build", "bin", "stencil_main")
NAMES = ("stencil_sweepk_relax", "stencil_iterate_relax", "stencil_iterate_until_relax", "stencil_relax_plan",
         "stencil_chebyshev_weights")
EINVAL, EUNSUPPORTED = -1, -5
K = rr.K_MAX
# never dereferenced: every call below fails its argument checks or has nothing to launch
A, B, S = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
NAN, INF = float("nan"), float("inf")


def layout(**kw):
    base = dict(dims=3, dtype=_lib.F64, nx=64, ny=40, nz=24)
    base.update(kw)
    return _lib.make_layout(_lib.make_problem(**base))


def lib():
    return _lib.load(debug=False)


def msg():
    return lib().stencil_last_error_message().decode()


def ref(lay):
    return ctypes.byref(lay) if lay is not None else None


def arr(w):
    return None if w is None else (ctypes.c_double * max(1, len(w)))(*w)


def sweepk(lay, a, b, s, begin, end, steps, w=(0.8, 1.7, 0.6, 1.25)):
    return lib().stencil_sweepk_relax(ref(lay), a, b, s, begin, end, steps, arr(w), None)


def iterate(lay, a, b, s, n=3, w=(0.8,), period=None, phase=0):
    return lib().stencil_iterate_relax(ref(lay), a, b, s, n, arr(w), len(w) if period is None else period, phase, None,
                                       None, None)


def until(lay, a, b, s, cap=10, every=5, norm=_lib.NORM_MAX, tol=1e-3, w=(0.8,), period=None):
    return lib().stencil_iterate_until_relax(ref(lay), a, b, s, cap, every, norm, tol, arr(w),
                                             len(w) if period is None else period, 0, None, None, None, None, None, None)


def test_names():
    header = open(os.path.join(ROOT, "include", "stencil_hip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib(), name)
        assert re.search(rf"^int {name}\(", header, flags=re.M), name


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.F64])
def test_relax_plan_is_the_source_plan(dtype):
    for lay in (layout(dtype=dtype), layout(dtype=dtype, nx=1024, ny=1024, nz=8)):
        for n in range(0, 14):
            got = [ctypes.c_int64(-1), ctypes.c_int32(-1)]
            want = [ctypes.c_int64(-2), ctypes.c_int32(-2)]
            assert lib().stencil_relax_plan(ctypes.byref(lay), n, ctypes.byref(got[0]), ctypes.byref(got[1])) == 0
            assert lib().stencil_source_plan(ctypes.byref(lay), n, ctypes.byref(want[0]), ctypes.byref(want[1])) == 0
            assert (got[0].value, got[1].value) == (want[0].value, want[1].value) == (-(-n // K), K)
    assert lib().stencil_relax_plan(ctypes.byref(layout()), 7, None, None) == 0  # outputs are optional
    assert lib().stencil_relax_plan(None, 3, None, None) == EINVAL


def test_einval_as_the_source_sweeps():
    lay = layout()
    nz = 24
    for rc in (sweepk(lay, A, B, None, 0, nz, 1),            # NULL src
               sweepk(lay, A, B, A, 0, nz, 1), sweepk(lay, A, B, B, 0, nz, 1),  # src is in / out
               sweepk(lay, A, A, S, 0, nz, 1),                # in place
               sweepk(lay, None, B, S, 0, nz, 1), sweepk(lay, A, None, S, 0, nz, 1),
               sweepk(lay, A, B, S, -1, nz, 1), sweepk(lay, A, B, S, 0, nz + 1, 1), sweepk(lay, A, B, S, 5, 4, 1),
               sweepk(lay, A, B, S, 0, nz, 0), sweepk(lay, A, B, S, 0, nz, K + 1), sweepk(lay, A, B, S, 0, nz, -2),
               sweepk(None, A, B, S, 0, nz, 1),
               iterate(lay, A, B, None), iterate(lay, A, B, A), iterate(lay, A, B, B), iterate(lay, A, A, S),
               iterate(lay, None, B, S), iterate(lay, A, None, S), iterate(None, A, B, S),
               until(lay, A, B, None), until(lay, A, B, A), until(lay, A, B, B), until(lay, A, A, S),
               until(lay, A, B, S, every=0), until(lay, A, B, S, tol=-1.0), until(lay, A, B, S, tol=NAN),
               until(lay, A, B, S, norm=2), until(None, A, B, S)):
        assert rc == EINVAL, msg()
        assert msg()


def test_einval_weights():
    lay = layout()
    nz = 24
    for call, word in (
            (lambda: sweepk(lay, A, B, S, 0, nz, 2, None), "null weights"),
            (lambda: iterate(lay, A, B, S, w=None, period=1), "null weights"),
            (lambda: until(lay, A, B, S, w=None, period=1), "null weights"),
            (lambda: iterate(lay, A, B, S, w=(0.8,), period=0), "period"),
            (lambda: until(lay, A, B, S, w=(0.8,), period=0), "period"),
            (lambda: sweepk(lay, A, B, S, 0, nz, 3, (0.8, NAN, 1.0)), "weight 1"),
            (lambda: sweepk(lay, A, B, S, 0, nz, 1, (INF,)), "weight 0"),
            (lambda: iterate(lay, A, B, S, w=(0.8, 1.0, -INF)), "weight 2"),
            (lambda: until(lay, A, B, S, w=(NAN,)), "weight 0")):
        assert call() == EINVAL
        assert word in msg(), msg()
    # a weight beyond the launch's steps is not read
    assert sweepk(lay, A, B, S, 3, 3, 2, (0.8, 1.2, NAN)) == 0


def test_nothing_to_do_needs_no_device():
    lay = layout()
    fin = ctypes.c_int(-1)
    w = arr((0.8, 1.2))
    assert lib().stencil_iterate_relax(ctypes.byref(lay), A, B, S, 0, w, 2, 1, None, ctypes.byref(fin), None) == 0
    assert fin.value == 0
    done, conv, last = ctypes.c_uint32(7), ctypes.c_int(7), ctypes.c_double(0.0)
    rc = lib().stencil_iterate_until_relax(ctypes.byref(lay), A, B, S, 0, 5, _lib.NORM_MAX, 1e-3, w, 2, 0, None,
                                           ctypes.byref(done), ctypes.byref(fin), ctypes.byref(last), ctypes.byref(conv), None)
    assert rc == 0 and (done.value, conv.value, fin.value) == (0, 0, 0) and last.value == INF


@pytest.mark.parametrize("kw,word", [(dict(dims=2, nx=300, ny=300, nz=1), "3D"), (dict(shape=_lib.BOX), "box"),
                                     (dict(radius=2), "radius"),
                                     (dict(halo=3, flags=_lib.HALO_LO), "halo"), (dict(halo=3, flags=_lib.HALO_HI), "halo"),
                                     (dict(kernel=_lib.KERNEL_DIRECT), "kernel"), (dict(kernel=_lib.KERNEL_ZMARCH), "kernel"),
                                     (dict(kernel=_lib.KERNEL_TEMPORAL2), "kernel")])
def test_eunsupported_names_the_restriction(kw, word):
    lay = layout(**kw)
    slow = int(lib().stencil_slow_extent(ctypes.byref(lay)))
    for rc in (sweepk(lay, A, B, S, 0, slow, 1), iterate(lay, A, B, S), until(lay, A, B, S),
               lib().stencil_relax_plan(ctypes.byref(lay), 3, None, None)):
        assert rc == EUNSUPPORTED
        assert word in msg()


def test_dma_order_is_unsupported():
    lay = layout(dims=2, nx=64, ny=64, nz=1, order=_lib.ORDER_DMA)
    assert iterate(lay, A, B, S) == EUNSUPPORTED


def test_chebyshev_errors():
    prob = _lib.make_problem(dims=3, dtype=_lib.F64, nx=15, ny=15, nz=15)
    w = (ctypes.c_double * 64)()
    for period in (0, -1, 3, 6, 65, 128):
        assert lib().stencil_chebyshev_weights(ctypes.byref(prob), period, w, None) == EINVAL
        assert "power of two" in msg()
    assert lib().stencil_chebyshev_weights(None, 4, w, None) == EINVAL
    assert lib().stencil_chebyshev_weights(ctypes.byref(prob), 4, None, None) == EINVAL
    flat = _lib.make_problem(dims=2, dtype=_lib.F64, nx=15, ny=15, nz=1)
    assert lib().stencil_chebyshev_weights(ctypes.byref(flat), 4, w, None) == EUNSUPPORTED
    assert "7-point" in msg()


# ----------------------------------------------------------------- the CLI
def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


BASE = ("-s", "10", "-b", "4", "--dims", "3", "-m", "CPU")


def test_cli_print_config_and_help():
    p = run(*BASE, "-i", "2", "--omega", "0.8", "--print-config")
    assert p.returncode == 0 and p.stdout.rstrip().endswith("omega=0.8")
    p = run(*BASE, "-i", "2", "--cheby", "8", "--source", "0.5", "--print-config")
    assert p.returncode == 0 and p.stdout.rstrip().endswith("source=0.5 cheby=8")
    p = run(*BASE, "-i", "2", "--print-config")
    assert "omega" not in p.stdout and "cheby" not in p.stdout
    out = run("--help").stdout
    assert "--omega" in out and "--cheby" in out and "--source" in out


@pytest.mark.parametrize("args,word", [
    (("--omega", "0.8", "--cheby", "4"), "mutually exclusive"),
    (("--cheby", "3"), "invalid value"), (("--cheby", "128"), "invalid value"), (("--omega", "nan"), "invalid value"),
    (("--omega", "0.8", "--shape", "box"), "7-point"), (("--cheby", "4", "-r", "2"), "7-point"),
    (("--omega", "0.8", "--gpus", "2"), "one GPU"), (("--omega", "0.8", "--kernel", "direct"), "--kernel"),
])
def test_cli_rejects(args, word):
    p = run(*BASE, "-i", "2", *args)
    assert p.returncode != 0 and word in p.stderr, p.stderr


def test_cli_rejects_2d_and_other_methods():
    p = run("-s", "10", "-b", "4", "-m", "CPU", "-i", "2", "--omega", "0.8")
    assert p.returncode != 0 and "--dims 3" in p.stderr
    p = run("-s", "10", "-b", "4", "--dims", "3", "-m", "HIPDirect", "-i", "2", "--cheby", "4")
    assert p.returncode != 0 and "HIP and CPU" in p.stderr


@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_cli_cpu_method_is_the_helper(dtype):
    """The CLI's own naive loop with the four-rounding update ends on the helper's grid, with and without --source."""
    p = rr.problem(dtype, 10, 10, 10)
    u = ob.init(p)
    for extra, g, what, omegas in (
            (("--omega", "0.8", "--source", "0.001"), 0.001, "omega 0.8", [0.8]),
            (("--omega", "1.3"), 0.0, "omega 1.3", [1.3]),
            (("--cheby", "4"), 0.0, "Chebyshev schedule of period 4", rr.chebyshev_weights(10, 10, 10, 4))):
        src = np.full_like(u, g)
        out = run(*BASE, "--dtype", dtype, "-i", "11", *extra, "-c")
        assert out.returncode == 0, out.stdout + out.stderr
        assert "The results of method CPU is correct." in out.stdout
        sums = re.findall(rf"^\[stencil-amd\] CPU: relaxed sweeps, {re.escape(what)}, 11 sweeps, interior sum = (\S+)$",
                          out.stdout, flags=re.M)
        want = rr.interior_sum(rr.sweeps(p, u, src, 11, omegas))
        assert len(sums) >= 1 and all(float(v) == want for v in sums), (sums, want)


def test_cli_cpu_tol():
    p = rr.problem("fp64", 10, 10, 10)
    u = ob.init(p)
    w = rr.chebyshev_weights(10, 10, 10, 4)
    grid, done, conv, _ = rr.until(p, u, np.zeros_like(u), 1e-4, 400, 8, w)
    assert conv and 8 <= done < 400
    out = run(*BASE, "--dtype", "fp64", "-i", "400", "--cheby", "4", "--tol", "1e-4", "--check-every", "8")
    assert out.returncode == 0, out.stdout + out.stderr
    counts = re.findall(r"^\[stencil-amd\] CPU: converged after (\d+) sweeps", out.stdout, flags=re.M)
    assert counts and all(int(n) == done for n in counts), (counts, done)
    sums = re.findall(r"interior sum = (\S+)$", out.stdout, flags=re.M)
    assert sums and all(float(v) == rr.interior_sum(grid) for v in sums)
