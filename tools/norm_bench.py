#!/usr/bin/env python3
"""What the convergence check costs, at 512^3 fp64 7-point.

    python tools/norm_bench.py [--out profiles/norm_bench_512_fp64.json]

Prints one JSON line:
  (a) norm   -- the byte rate of stencil_diff_norms over the whole grid (both
                interiors read once, nothing written), device time between
                events on the stream, next to stencil_copy_bandwidth moving the
                same bytes (half read, half written), 5 runs each, in one
                process after the same settle; and the same call over one unit,
                the part of a call that is not streaming (streaming_GBps is
                the rate of the rest);
  (b) checks -- iterate_until(tol=0, 1000 sweeps, a check every 100) against
                stencil_iterate(1000), device time of each, overhead in percent.

    python tools/norm_bench.py --fused-ab [--rounds 3] [--parent-lib PATH] [--out FILE]

The check that rides in the K-step launch against the un-fused one (DESIGN.md
§5.6): the same checked jobs (a check every 100, 20 and 4 sweeps) with
STENCIL_UNTIL_FUSED=0 and =1 -- and, with --parent-lib, with another build of
libstencil_hip.so, e.g. the parent commit's -- each in a fresh child process,
the arms alternating, `--rounds` children per arm.  Every child also times the
checking launch against the plain launch of the same shape, interleaved.
--nx/--ny/--nz give a grid that is not a cube; --launch-only skips the jobs.

    python tools/norm_bench.py --slab-ab [--rounds 3] [--parent-lib PATH] [--out FILE]

The same protocol for stencil_slab_run_until on a one-slab
PERIODIC job (the interior-rank rehearsal): per child SlabJob.run(sweeps) and
run_until with a tol it never meets, a check every 100, 20 and 4 sweeps, host
wall time of each; arms: the check in the launch, STENCIL_UNTIL_FUSED=0, the
same two on a boundary + interior job (STENCIL_SLAB_SIGNAL=0: its checking
rounds are slab_round's form), and -- with --parent-lib -- run() alone on
another build.  Every child of this build also times the face-signalled checking
launch against the plain face-signalled launch, between events.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stencil_amd import _lib
from stencil_amd.engine import JacobiEngine, SlabJob, StencilSpec, _stream_handle


EVERY = (100, 20, 4)


def child(a):
    """One arm in this (fresh) process: the fixed-count job, the checked jobs,
    and the checking launch beside the plain one.  Prints one JSON line."""
    if a.lib:  # another build of the library: bind what it exports
        _lib.LIB_PATH = a.lib
        probe, sigs = ctypes.CDLL(a.lib), _lib.signatures()
        _lib.signatures = lambda: {k: v for k, v in sigs.items() if hasattr(probe, k)}
    torch.cuda.set_device(0)
    nx, ny, nz = a.nx or a.size, a.ny or a.size, a.nz or a.size
    e = JacobiEngine(StencilSpec(dims=3, dtype=a.dtype), nx, ny, nz, device=0)
    has = hasattr(e.lib, "stencil_sweepk_update_max")
    out = {"fused_check": {str(ev): e.until_plan(ev) for ev in EVERY} if has else None, "steps": e.fuse_steps}

    def fixed():
        e.reset("reference")
        e.prepare()
        return e.iterate(a.sweeps, timed=True)[1]

    def checked(every):
        e.reset("reference")
        e.prepare()
        r = e.iterate_until(0.0, a.sweeps, check_every=every, timed=True)
        assert r.iterations == a.sweeps and not r.converged
        return r.ms

    if not a.launch_only:
        fixed(), [checked(ev) for ev in EVERY]  # first use: the shape's schedule trials
        fixed_ms, checked_ms = [], {ev: [] for ev in EVERY}
        for _ in range(a.reps):
            fixed_ms.append(fixed())
            for ev in EVERY:
                checked_ms[ev].append(checked(ev))
        out["iterate_ms"] = [round(t, 3) for t in fixed_ms]
        out["iterate_until_ms"] = {str(ev): [round(t, 3) for t in v] for ev, v in checked_ms.items()}
    if has:
        k, n = e.fuse_steps, e.slow_extent
        stream = torch.cuda.current_stream()
        word = torch.zeros(1, dtype=torch.int64, device=e.device)

        def launches(check, count=20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(count):
                if check:
                    _lib.check(e.lib.stencil_sweepk_update_max(ctypes.byref(e.layout), ctypes.c_void_p(e.a.data_ptr()),
                                                               ctypes.c_void_p(e.b.data_ptr()), 0, n, k,
                                                               ctypes.c_void_p(word.data_ptr()), _stream_handle(stream)),
                               "stencil_sweepk_update_max", lib=e.lib)
                else:
                    e.sweepk(e.a, e.b, 0, n, k, stream=stream)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / count

        e.reset("random", 7)
        launches(False, 2), launches(True, 2)  # the schedule trials
        e.prepare()
        plain, check = [], []
        for _ in range(5):
            plain.append(launches(False))
            check.append(launches(True))
        out["launch_ms"] = {"plain": [round(t, 4) for t in plain], "checking": [round(t, 4) for t in check]}
    print(json.dumps(out))


def slab_child(a):
    """One arm of --slab-ab in this (fresh) process.  Prints one JSON line."""
    if a.lib:
        _lib.LIB_PATH = a.lib
        probe, sigs, more = ctypes.CDLL(a.lib), _lib.signatures(), _lib.slab_until_signatures()
        _lib.signatures = lambda: {k: v for k, v in sigs.items() if hasattr(probe, k)}
        _lib.slab_until_signatures = lambda: {k: v for k, v in more.items() if hasattr(probe, k)}
    torch.cuda.set_device(0)
    nx, ny, nz = a.nx or a.size, a.ny or a.size, a.nz or a.size
    job = SlabJob(StencilSpec(dims=3, dtype=a.dtype), nx, ny, nz, [0], exchange="copy", periodic=True)
    has = hasattr(job.lib, "stencil_slab_run_until")
    k = job.info(0)["sweeps_per_round"]
    out = {"round_info": job.round_info(), "steps": k,
           "until_plan": {str(ev): job.until_plan(ev) for ev in EVERY} if has else None}

    def fixed():
        job.fill_initial("reference")
        job.run(5 * k)  # the clock up, the shape's one-time choices
        return job.run(a.sweeps)

    def checked(every):
        job.fill_initial("reference")
        job.run(5 * k)
        r = job.run_until(0.0, a.sweeps, check_every=every)
        assert r.iterations == a.sweeps and not r.converged
        return r.ms

    fixed()
    if has:
        [checked(ev) for ev in EVERY]
    fixed_ms, checked_ms = [], {ev: [] for ev in EVERY}
    for _ in range(a.reps):
        fixed_ms.append(fixed())
        if has:
            for ev in EVERY:
                checked_ms[ev].append(checked(ev))
    out["run_ms"] = [round(t, 3) for t in fixed_ms]
    if has:
        out["run_until_ms"] = {str(ev): [round(t, 3) for t in v] for ev, v in checked_ms.items()}
    job.close()
    if has and not a.lib:
        # the face-signalled checking launch beside the plain face-signalled one: a slab with both halos
        e = JacobiEngine(StencilSpec(dims=3, dtype=a.dtype, halo=k), nx, ny, nz, device=0, flags=_lib.HALO_LO | _lib.HALO_HI)
        e.reset("random", 7)
        stream = torch.cuda.current_stream()
        word = torch.zeros(1, dtype=torch.int64, device=e.device)
        sig = torch.zeros(4, dtype=torch.int32, device=e.device)
        n32 = ctypes.c_int32(0)

        def launches(check, count=20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(count):
                if check:
                    _lib.check(e.lib.stencil_sweepk_signal_update_max(
                        ctypes.byref(e.layout), ctypes.c_void_p(e.a.data_ptr()), ctypes.c_void_p(e.b.data_ptr()), 0, nz, k,
                        ctypes.c_void_p(sig.data_ptr()), None, ctypes.c_void_p(word.data_ptr()), ctypes.byref(n32),
                        _stream_handle(stream)), "stencil_sweepk_signal_update_max", lib=e.lib)
                else:
                    e.sweepk_signal(e.a, e.b, 0, nz, k, sig, stream=stream)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / count

        launches(False, 2), launches(True, 2)
        for _ in range(3):
            launches(False)
        plain, check = [], []
        for _ in range(5):
            plain.append(launches(False))
            check.append(launches(True))
        out["launch_ms"] = {"plain_signalled": [round(t, 4) for t in plain],
                            "checking_signalled": [round(t, 4) for t in check]}
    print(json.dumps(out))


def slab_ab(a):
    arms = [("fused", {"STENCIL_UNTIL_FUSED": "1"}, None), ("unfused", {"STENCIL_UNTIL_FUSED": "0"}, None),
            ("fused_boundary_interior", {"STENCIL_UNTIL_FUSED": "1", "STENCIL_SLAB_SIGNAL": "0"}, None),
            ("unfused_boundary_interior", {"STENCIL_UNTIL_FUSED": "0", "STENCIL_SLAB_SIGNAL": "0"}, None)]
    if a.parent_lib:
        arms.append(("parent", {}, a.parent_lib))
    runs = {name: [] for name, _, _ in arms}
    base = [sys.executable, os.path.abspath(__file__), "--slab-child", "--size", str(a.size), "--dtype", a.dtype,
            "--reps", str(a.reps), "--sweeps", str(a.sweeps), "--nx", str(a.nx), "--ny", str(a.ny), "--nz", str(a.nz)]
    for _ in range(a.rounds):
        for name, env, lib in arms:
            full = {k: v for k, v in os.environ.items() if k not in ("STENCIL_UNTIL_FUSED", "STENCIL_SLAB_SIGNAL")}
            full.update(env)
            p = subprocess.run(base + (["--lib", lib] if lib else []), capture_output=True, text=True, env=full)
            if p.returncode != 0:
                raise SystemExit(f"{name}: child failed\n{p.stdout}{p.stderr}")
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = {"tool": "norm_bench --slab-ab", "grid": [a.nx or a.size, a.ny or a.size, a.nz or a.size], "dtype": a.dtype,
            "sweeps": a.sweeps, "rounds": a.rounds, "job": "one slab, periodic, device copies", "arms": {}}
    for name, rs in runs.items():
        f = [t for r in rs for t in r["run_ms"]]
        arm = {"round_info": rs[0]["round_info"], "steps": rs[0]["steps"], "until_plan": rs[0]["until_plan"],
               "run_ms": {"median": statistics.median(f), "spread_percent": spread(f), "all": f}}
        if "run_until_ms" in rs[0]:
            arm["run_until_ms"] = {}
            for ev in EVERY:
                c = [t for r in rs for t in r["run_until_ms"][str(ev)]]
                arm["run_until_ms"][str(ev)] = {
                    "median": statistics.median(c), "spread_percent": spread(c), "all": c,
                    "overhead_percent": round(100.0 * (statistics.median(c) / statistics.median(f) - 1.0), 2)}
        if "launch_ms" in rs[0]:
            pl = [t for r in rs for t in r["launch_ms"]["plain_signalled"]]
            ck = [t for r in rs for t in r["launch_ms"]["checking_signalled"]]
            arm["launch_ms"] = {"plain_signalled_median": statistics.median(pl), "plain_spread_percent": spread(pl),
                                "checking_signalled_median": statistics.median(ck), "checking_spread_percent": spread(ck),
                                "checking_vs_plain_percent":
                                    round(100.0 * (statistics.median(ck) / statistics.median(pl) - 1.0), 2)}
        line["arms"][name] = arm
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


def spread(v):
    return round(100.0 * (max(v) - min(v)) / statistics.median(v), 2)


def fused_ab(a):
    arms = [("unfused", {"STENCIL_UNTIL_FUSED": "0"}, None), ("fused", {"STENCIL_UNTIL_FUSED": "1"}, None)]
    if a.parent_lib:
        arms.append(("parent", {}, a.parent_lib))
    runs = {name: [] for name, _, _ in arms}
    base = [sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--dtype", a.dtype,
            "--reps", str(a.reps), "--sweeps", str(a.sweeps), "--nx", str(a.nx), "--ny", str(a.ny), "--nz", str(a.nz)]
    if a.launch_only:
        base.append("--launch-only")
    for _ in range(a.rounds):  # alternating: every arm sees the same box at about the same time
        for name, env, lib in arms:
            full = {k: v for k, v in os.environ.items() if k != "STENCIL_UNTIL_FUSED"}
            full.update(env)
            p = subprocess.run(base + (["--lib", lib] if lib else []), capture_output=True, text=True, env=full)
            if p.returncode != 0:
                raise SystemExit(f"{name}: child failed\n{p.stdout}{p.stderr}")
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = {"tool": "norm_bench --fused-ab", "grid": [a.nx or a.size, a.ny or a.size, a.nz or a.size], "dtype": a.dtype,
            "sweeps": a.sweeps, "rounds": a.rounds, "arms": {}}
    for name, rs in runs.items():
        arm = {"fused_check": rs[0]["fused_check"], "steps": rs[0]["steps"]}
        if not a.launch_only:
            f = [t for r in rs for t in r["iterate_ms"]]
            arm["iterate_ms"] = {"median": statistics.median(f), "spread_percent": spread(f), "all": f}
            arm["iterate_until_ms"] = {}
            for ev in EVERY:
                c = [t for r in rs for t in r["iterate_until_ms"][str(ev)]]
                arm["iterate_until_ms"][str(ev)] = {
                    "median": statistics.median(c), "spread_percent": spread(c), "all": c,
                    "overhead_percent": round(100.0 * (statistics.median(c) / statistics.median(f) - 1.0), 2)}
        if "launch_ms" in rs[0]:
            pl = [t for r in rs for t in r["launch_ms"]["plain"]]
            ck = [t for r in rs for t in r["launch_ms"]["checking"]]
            arm["launch_ms"] = {"plain_median": statistics.median(pl), "plain_spread_percent": spread(pl),
                                "checking_median": statistics.median(ck), "checking_spread_percent": spread(ck),
                                "checking_vs_plain_percent":
                                    round(100.0 * (statistics.median(ck) / statistics.median(pl) - 1.0), 2)}
        line["arms"][name] = arm
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--nx", type=int, default=0)
    ap.add_argument("--ny", type=int, default=0)
    ap.add_argument("--nz", type=int, default=0)
    ap.add_argument("--fused-ab", action="store_true", help="the fused check against the un-fused one, in child processes")
    ap.add_argument("--rounds", type=int, default=3, help="--fused-ab: children per arm")
    ap.add_argument("--parent-lib", default=None, help="--fused-ab: a third arm, another build of libstencil_hip.so")
    ap.add_argument("--launch-only", action="store_true", help="--fused-ab: only the launch timing")
    ap.add_argument("--slab-ab", action="store_true", help="stencil_slab_run_until on a one-slab periodic job, in child processes")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--slab-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dtype", default="fp64", choices=["fp32", "fp64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=1000)
    ap.add_argument("--check-every", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.slab_child:
        return slab_child(a)
    if a.slab_ab:
        return slab_ab(a)
    if a.fused_ab:
        return fused_ab(a)
    torch.cuda.set_device(0)
    n = a.size
    e = JacobiEngine(StencilSpec(dims=3, dtype=a.dtype), n, n, n, device=0)
    es = e.spec.elem_bytes
    moved = 2 * n * n * n * es  # both interiors; the copy reads half of it and writes half
    src = torch.ones(moved // 2 // 4, dtype=torch.float32, device=e.device)
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream()

    def copy_ms():
        ms = ctypes.c_float(0.0)
        _lib.check(e.lib.stencil_copy_bandwidth(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                                moved // 2, 1, _stream_handle(stream), ctypes.byref(ms)),
                   "stencil_copy_bandwidth", lib=e.lib)
        return ms.value

    def norm_ms(end=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        e.diff_norms(e.a, e.b, 0, end, stream=stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    e.reset("random", 7)
    e.sweep(e.a, e.b, 0, e.slow_extent)  # b = one sweep of a: a real update to take the norm of
    copy_ms(), norm_ms()                 # first use: code load, the stream's memory pool
    e.prepare()                          # the clock settled by ~25 ms of launches
    copies, norms, fixed_part = [], [], []
    for _ in range(a.reps):              # interleaved, so both see the same clock
        copies.append(copy_ms())
        norms.append(norm_ms())
        # one unit of n: what a call costs between the events besides streaming the grids (the submit latency on an
        # idle queue, the scratch allocation, the combine launch, the copy of the results)
        fixed_part.append(norm_ms(1))
    gbps = lambda ms: moved / (ms * 1e-3) / 1e9
    copy_rates, norm_rates = [gbps(t) for t in copies], [gbps(t) for t in norms]
    copy_med, norm_med = statistics.median(copy_rates), statistics.median(norm_rates)
    stream_ms = statistics.median(norms) - statistics.median(fixed_part)
    stream_rate = gbps(stream_ms) * (n - 1) / n

    def fixed():
        e.reset("reference")
        e.prepare()
        return e.iterate(a.sweeps, timed=True)[1]

    def checked():
        e.reset("reference")
        e.prepare()
        r = e.iterate_until(0.0, a.sweeps, check_every=a.check_every, timed=True)
        assert r.iterations == a.sweeps and not r.converged
        return r.ms

    fixed(), checked()
    fixed_ms, checked_ms = [], []
    for _ in range(3):
        fixed_ms.append(fixed())
        checked_ms.append(checked())
    f, c = statistics.median(fixed_ms), statistics.median(checked_ms)
    line = {
        "tool": "norm_bench", "size": n, "dtype": a.dtype, "device": torch.cuda.get_device_name(0),
        "bytes_moved": moved,
        "norm": {"GBps": [round(v, 1) for v in norm_rates], "median_GBps": round(norm_med, 1),
                 "ms": [round(t, 4) for t in norms], "one_unit_ms": [round(t, 4) for t in fixed_part],
                 "streaming_GBps": round(stream_rate, 1)},
        "copy": {"GBps": [round(v, 1) for v in copy_rates], "median_GBps": round(copy_med, 1),
                 "spread_percent": round(100.0 * (max(copy_rates) - min(copy_rates)) / copy_med, 2),
                 "ms": [round(t, 4) for t in copies]},
        "norm_vs_copy_percent": round(100.0 * (norm_med / copy_med - 1.0), 2),
        "norm_streaming_vs_copy_percent": round(100.0 * (stream_rate / copy_med - 1.0), 2),
        "checks": {"sweeps": a.sweeps, "check_every": a.check_every,
                   "iterate_ms": [round(t, 3) for t in fixed_ms], "iterate_until_ms": [round(t, 3) for t in checked_ms],
                   "overhead_percent": round(100.0 * (c / f - 1.0), 2)},
    }
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
