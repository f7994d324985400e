"""stencil_until_plan: the launches of one block of stencil_iterate_until and
whether its check rides in the block's last launch -- on the host, no GPU.

A block of `block` sweeps checked the un-fused way is stencil_iterate's plan
for block - 1 sweeps, one single sweep and the norm's two launches; checked by
the K-step launch itself (max norm, a job of K-step 7-point launches, block
>= K) it is the plan for block - K sweeps and one checking launch.
"""
import ctypes
import os
import subprocess
import sys

import pytest

from stencil_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def layout(**kw):
    base = dict(dims=3, dtype=_lib.F64, nx=64, ny=40, nz=24)
    base.update(kw)
    return _lib.make_layout(_lib.make_problem(**base))


def until_plan(lay, block, norm=_lib.NORM_MAX, lib=None):
    lib = lib or _lib.load(debug=False)
    launches, fused = ctypes.c_int64(-1), ctypes.c_int32(-1)
    rc = lib.stencil_until_plan(ctypes.byref(lay), block, norm, ctypes.byref(launches), ctypes.byref(fused))
    assert rc == 0, lib.stencil_last_error_message()
    return launches.value, fused.value


def plan(lay, iterations):
    lib = _lib.load(debug=False)
    launches = ctypes.c_int64(-1)
    assert lib.stencil_plan(ctypes.byref(lay), iterations, ctypes.byref(launches), None) == 0
    return launches.value


def unfused(lay, block):
    # block - 1 sweeps, a single sweep, the norm kernel and its combine launch (one batch at these sizes)
    return plan(lay, block - 1) + 1 + 2


def test_k4_blocks_of_the_7_point_star():
    lay = layout()  # fp64: K = 4
    assert plan(lay, 4) == 1 and plan(lay, 5) == 2
    assert until_plan(lay, 100) == (25, 1)  # 24 plain K-step launches and the checking one
    assert until_plan(lay, 3) == (unfused(lay, 3), 0)  # shorter than one launch
    assert unfused(lay, 3) == 4                        # a pair, a single, two norm launches
    assert until_plan(lay, 4) == (1, 1)
    assert until_plan(lay, 5) == (2, 1)
    assert until_plan(lay, 7) == (1 + 1 + 1, 1)        # 3 sweeps as a pair and a single, then the launch
    assert until_plan(lay, 100)[0] < unfused(lay, 100) == 24 + 1 + 1 + 1 + 2


def test_fp32_steps_follow_the_job():
    small, wide = layout(dtype=_lib.F32), layout(dtype=_lib.F32, nx=1024, ny=1024, nz=8)
    assert until_plan(small, 4) == (1, 1)               # K = 4 on small fp32 planes
    assert until_plan(wide, 4) == (unfused(wide, 4), 0)  # K = 5 from 1024^2 cells per plane
    assert until_plan(wide, 5) == (1, 1)
    assert until_plan(wide, 100) == (20, 1)


@pytest.mark.parametrize("kw", [dict(shape=_lib.BOX), dict(dims=2, nx=300, ny=300, nz=1), dict(radius=2),
                                dict(kernel=_lib.KERNEL_ZMARCH), dict(kernel=_lib.KERNEL_TEMPORAL2)])
def test_other_families_keep_the_unfused_check(kw):
    lay = layout(**kw)
    for block in (1, 3, 10, 100):
        assert until_plan(lay, block) == (unfused(lay, block), 0)


def test_l2_keeps_the_unfused_check():
    lay = layout()
    for block in (4, 100):
        assert until_plan(lay, block, _lib.NORM_L2) == (unfused(lay, block), 0)


def test_explicit_temporalk_is_fused():
    assert until_plan(layout(kernel=_lib.KERNEL_TEMPORALK), 100) == (25, 1)


def test_documented_steps_knob(monkeypatch):
    lay = layout()
    monkeypatch.setenv("STENCIL_TK_STEPS", "3")
    assert until_plan(lay, 3) == (1, 1)
    assert until_plan(lay, 100) == (plan(lay, 97) + 1, 1)
    monkeypatch.setenv("STENCIL_TK_STEPS", "5")
    assert until_plan(lay, 4) == (unfused(lay, 4), 0)
    assert until_plan(lay, 100) == (20, 1)


def test_invalid_arguments():
    lib = _lib.load(debug=False)
    lay = layout()
    out, fused = ctypes.c_int64(), ctypes.c_int32()
    assert lib.stencil_until_plan(ctypes.byref(lay), 0, _lib.NORM_MAX, ctypes.byref(out), ctypes.byref(fused)) == -1
    assert lib.stencil_until_plan(ctypes.byref(lay), 10, 2, ctypes.byref(out), ctypes.byref(fused)) == -1
    assert lib.stencil_until_plan(None, 10, _lib.NORM_MAX, ctypes.byref(out), ctypes.byref(fused)) == -1
    assert lib.stencil_last_error_message()
    assert lib.stencil_until_plan(ctypes.byref(lay), 10, _lib.NORM_MAX, None, None) == 0  # outputs are optional


def test_the_knob_is_a_documented_one():
    """STENCIL_UNTIL_FUSED is read by the product library: setting it must not
    select the debug twin."""
    assert "STENCIL_UNTIL_FUSED" in _lib.API_KNOBS
    for name in ("stencil_sweepk_update_max", "stencil_until_plan"):
        assert name in _lib.EXPORTED_SYMBOLS and not name.startswith("stencil_slab_")


CHILD = """
import ctypes, json, sys
sys.path.insert(0, {root!r})
from stencil_amd import _lib
out = {{}}
for debug in (False, True):
    lib = _lib.load(debug=debug)
    lay = _lib.make_layout(_lib.make_problem(dims=3, dtype=_lib.F64, nx=64, ny=40, nz=24))
    launches, fused = ctypes.c_int64(-1), ctypes.c_int32(-1)
    assert lib.stencil_until_plan(ctypes.byref(lay), 100, _lib.NORM_MAX, ctypes.byref(launches), ctypes.byref(fused)) == 0
    out["debug" if debug else "product"] = [launches.value, fused.value, _lib.load() is _lib.load(debug=False)]
print(json.dumps(out))
"""


@pytest.mark.parametrize("value,want", [("0", [29, 0]), ("1", [25, 1]), (None, [25, 1])])
def test_knob_in_a_child_process(value, want):
    import json
    env = {k: v for k, v in os.environ.items() if not k.startswith("STENCIL_")}
    if value is not None:
        env["STENCIL_UNTIL_FUSED"] = value
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, env=env,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    # both libraries read it, and it leaves the product library selected
    assert got["product"] == want + [True] and got["debug"] == want + [True]
