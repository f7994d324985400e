"""The source-term entry points on the host, no GPU: stencil_source_plan, every
argument error that fires before a device is touched, the four names in the
header / binding / library, the untouched plain plans, and the CLI's --source
on the CPU method."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import binding as ob
from stencil_amd import _lib
from tests import source_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "build", "bin", "stencil_main")
NAMES = ("stencil_sweepk_source", "stencil_iterate_source", "stencil_source_plan", "stencil_iterate_until_source")
EINVAL, EUNSUPPORTED = -1, -5
K = sr.K_MAX
# never dereferenced: every call below fails its argument checks or has nothing to launch
A, B, S = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)


def layout(**kw):
    base = dict(dims=3, dtype=_lib.F64, nx=64, ny=40, nz=24)
    base.update(kw)
    return _lib.make_layout(_lib.make_problem(**base))


def lib():
    return _lib.load(debug=False)


def source_plan(lay, iterations):
    launches, steps = ctypes.c_int64(-1), ctypes.c_int32(-1)
    rc = lib().stencil_source_plan(ctypes.byref(lay), iterations, ctypes.byref(launches), ctypes.byref(steps))
    assert rc == 0, lib().stencil_last_error_message()
    return launches.value, steps.value


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.F64])
def test_source_plan(dtype):
    """K = 4 for both types: launches of 4 sweeps, the remainder (1, 2 or 3) as one shorter launch."""
    assert K == 4
    lay = layout(dtype=dtype)
    want = {0: 0, 1: 1, K - 1: 1, K: 1, K + 1: 2, 100: 25, 101: 26}
    for iterations, launches in want.items():
        assert source_plan(lay, iterations) == (launches, 4), iterations
    assert lib().stencil_source_plan(ctypes.byref(lay), 7, None, None) == 0  # outputs are optional
    # large planes keep K = 4 (the plain fp32 job goes to K = 5 there)
    assert source_plan(layout(dtype=dtype, nx=1024, ny=1024, nz=8), 100) == (25, 4)
    assert source_plan(layout(dtype=dtype, kernel=_lib.KERNEL_TEMPORALK), 5) == (2, 4)


def ref(lay):
    return ctypes.byref(lay) if lay is not None else None


def sweepk(lay, a, b, s, begin, end, steps):
    return lib().stencil_sweepk_source(ref(lay), a, b, s, begin, end, steps, None)


def iterate(lay, a, b, s, n=3):
    return lib().stencil_iterate_source(ref(lay), a, b, s, n, None, None, None)


def until(lay, a, b, s, cap=10, every=5, norm=_lib.NORM_MAX, tol=1e-3):
    return lib().stencil_iterate_until_source(ref(lay), a, b, s, cap, every, norm, tol, None, None, None, None,
                                              None, None)


def test_einval():
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
               until(lay, A, B, S, every=0), until(lay, A, B, S, tol=-1.0), until(lay, A, B, S, tol=float("nan")),
               until(lay, A, B, S, norm=2), until(None, A, B, S)):
        assert rc == EINVAL, lib().stencil_last_error_message()
        assert lib().stencil_last_error_message()
    assert lib().stencil_source_plan(None, 3, None, None) == EINVAL


def test_nothing_to_do_needs_no_device():
    lay = layout()
    fin = ctypes.c_int(-1)
    assert lib().stencil_iterate_source(ctypes.byref(lay), A, B, S, 0, None, ctypes.byref(fin), None) == 0
    assert fin.value == 0
    done, conv, last = ctypes.c_uint32(7), ctypes.c_int(7), ctypes.c_double(0.0)
    rc = lib().stencil_iterate_until_source(ctypes.byref(lay), A, B, S, 0, 5, _lib.NORM_MAX, 1e-3, None,
                                            ctypes.byref(done), ctypes.byref(fin), ctypes.byref(last), ctypes.byref(conv), None)
    assert rc == 0 and (done.value, conv.value, fin.value) == (0, 0, 0) and last.value == float("inf")


@pytest.mark.parametrize("kw,word", [(dict(dims=2, nx=300, ny=300, nz=1), "3D"), (dict(shape=_lib.BOX), "box"),
                                     (dict(radius=2), "radius"),
                                     (dict(halo=3, flags=_lib.HALO_LO), "halo"), (dict(halo=3, flags=_lib.HALO_HI), "halo"),
                                     (dict(kernel=_lib.KERNEL_DIRECT), "kernel"), (dict(kernel=_lib.KERNEL_ZMARCH), "kernel"),
                                     (dict(kernel=_lib.KERNEL_TEMPORAL2), "kernel")])
def test_eunsupported_names_the_restriction(kw, word):
    lay = layout(**kw)
    slow = int(lib().stencil_slow_extent(ctypes.byref(lay)))
    for rc in (sweepk(lay, A, B, S, 0, slow, 1), iterate(lay, A, B, S), until(lay, A, B, S),
               lib().stencil_source_plan(ctypes.byref(lay), 3, None, None)):
        assert rc == EUNSUPPORTED
        assert word in lib().stencil_last_error_message().decode()


def test_dma_order_is_unsupported():
    lay = layout(dims=2, nx=64, ny=64, nz=1, order=_lib.ORDER_DMA)
    assert iterate(lay, A, B, S) == EUNSUPPORTED  # (a 2D problem: the DMA order exists only there)


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "stencil_hip.h")).read()
    sigs = _lib.signatures()
    for dbg in (False, True):
        loaded = _lib.load(debug=dbg)
        for name in NAMES:
            assert re.search(r"^int %s\(" % name, header, flags=re.M), name
            assert name in _lib.EXPORTED_SYMBOLS and hasattr(loaded, name)
            res, args = sigs[name]
            assert getattr(loaded, name).restype is res and list(getattr(loaded, name).argtypes) == list(args)
    c, P = ctypes, ctypes.POINTER
    L = P(_lib.Layout)
    assert sigs["stencil_sweepk_source"][1] == [L, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int32,
                                                c.c_void_p]
    assert sigs["stencil_source_plan"][1] == [L, c.c_uint32, P(c.c_int64), P(c.c_int32)]
    assert len(sigs["stencil_iterate_source"][1]) == 8 and len(sigs["stencil_iterate_until_source"][1]) == 14
    assert "#define STENCIL_SOURCE_MAX_STEPS %d" % K in header


def test_plain_plans_are_unchanged():
    """Three answers of tests/test_until_plan.py's layouts, and stencil_plan's behind them."""
    lay = layout()
    launches, fused = ctypes.c_int64(-1), ctypes.c_int32(-1)

    def until_plan(l, block):
        assert lib().stencil_until_plan(ctypes.byref(l), block, _lib.NORM_MAX, ctypes.byref(launches), ctypes.byref(fused)) == 0
        return launches.value, fused.value

    def plan(l, n):
        assert lib().stencil_plan(ctypes.byref(l), n, ctypes.byref(launches), None) == 0
        return launches.value

    assert until_plan(lay, 100) == (25, 1)
    assert until_plan(lay, 7) == (3, 1)
    assert until_plan(layout(dtype=_lib.F32, nx=1024, ny=1024, nz=8), 100) == (20, 1)
    assert plan(lay, 4) == 1 and plan(lay, 5) == 2 and plan(lay, 100) == 25


# ---- the CLI on the CPU method ----------------------------------------------
def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


SUM_LINE = r"^\[stencil-amd\] CPU: source 0\.25, (\d+) sweeps, interior sum = (\S+)$"


def test_cli_cpu_source_equals_the_helper():
    """-m CPU --dims 3 --source 0.25 -s 8 -i 5 -c (-b is a required option of the
    reference's surface): the check passes, and the final grid's interior sum --
    printed with every digit -- is the helper's."""
    p = run("-m", "CPU", "--dims", "3", "--source", "0.25", "-s", "8", "-b", "4", "-i", "5", "-c")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "The results of method CPU is correct." in p.stdout
    prob = sr.problem("fp32", 8, 8, 8)
    u = ob.init(prob)
    src = np.full_like(u, np.float32(0.25))
    want = sr.interior_sum(sr.sweeps(prob, u, src, 5))
    found = re.findall(SUM_LINE, p.stdout, flags=re.M)
    assert len(found) == 2 and all(int(n) == 5 and float(v) == want for n, v in found), (found, want)
    # and it is not the plain job's
    assert want != sr.interior_sum(sr.sweeps(prob, u, np.zeros_like(u), 5))


def test_cli_cpu_source_with_tol():
    prob = sr.problem("fp64", 8, 8, 8)
    u = ob.init(prob)
    grid, done, conv, _ = sr.until(prob, u, np.full_like(u, 1e-3), 1e-3, 200, 7)
    assert conv and 7 < done < 200
    p = run("-m", "CPU", "--dims", "3", "--dtype", "fp64", "--source", "0.001", "-s", "8", "-b", "4", "-i", "200", "--tol",
            "1e-3", "--check-every", "7", "-c")
    assert p.returncode == 0, p.stdout + p.stderr
    counts = re.findall(r"^\[stencil-amd\] CPU: converged after (\d+) sweeps", p.stdout, flags=re.M)
    assert counts and all(int(n) == done for n in counts)
    sums = re.findall(r"interior sum = (\S+)$", p.stdout, flags=re.M)
    assert sums and all(float(v) == sr.interior_sum(grid) for v in sums)


@pytest.mark.parametrize("args", [("-m", "CPU"), ("--dims", "3", "-m", "DMA"), ("--dims", "3", "-m", "HIPZMarch"),
                                  ("--dims", "3", "-m", "CPU", "HIPMultiGPU"), ("--dims", "3", "-m", "HIP", "--gpus", "2"),
                                  ("--dims", "3", "-m", "CPU", "--shape", "box"), ("--dims", "3", "-m", "CPU", "-r", "2"),
                                  ("--dims", "3", "-m", "HIP", "--kernel", "zmarch")])
def test_cli_refuses_other_combinations(args):
    p = run("-s", "8", "-b", "4", "-i", "2", "--source", "0.5", *args)
    assert p.returncode == 1 and "--source" in p.stderr and "Method spent" not in p.stdout


def test_cli_bad_value_and_print_config():
    assert run("-s", "8", "-b", "4", "-i", "2", "--dims", "3", "-m", "CPU", "--source", "abc").returncode == 1
    p = run("-s", "8", "-b", "4", "-i", "2", "--dims", "3", "-m", "CPU", "--source", "-0.5", "--print-config")
    assert p.returncode == 0 and p.stdout.split()[-1] == "source=-0.5"
    # absent: the line is what it was
    p = run("-s", "8", "-b", "4", "-i", "2", "--dims", "3", "-m", "CPU", "--print-config")
    assert "source" not in p.stdout and p.stdout.split()[-1] == "norm=max"


def test_cli_stdout_without_source_is_unchanged():
    p = run("-s", "8", "-b", "4", "-i", "5", "--dims", "3", "-m", "CPU", "-c")
    assert p.returncode == 0 and "source" not in p.stdout and "interior sum" not in p.stdout
    lines = [l for l in p.stdout.splitlines() if not l.startswith("[stencil-amd]")]
    assert lines[0] == "Start to check the correctness of method CPU." and lines[1] == "The results of method CPU is correct."
    assert re.fullmatch(r"CPU Method spent \S+ms for 5 iterations\.", lines[2])
    assert re.fullmatch(r"The average time taken by CPU method is \S+ms for 5 iterations\.", lines[3]) and len(lines) == 4
