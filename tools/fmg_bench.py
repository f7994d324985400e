#!/usr/bin/env python3
"""What the full multigrid pass costs, and what it gains over the zero-start
multigrid solve.

    python tools/fmg_bench.py [--out profiles/fmg_bench.json] [--rounds 3] [--small]

tools/mg_bench.py's procedure: one process on one GPU; every path runs untimed
first (code objects, the strip kernel's schedule trials, the clock);
`--rounds` alternating rounds; device time between events; every round kept.

1. The two transfer kernels of the pass, at 255^3 and 511^3, fp32 and fp64:
     restrict_source    stencil_restrict_source: one read of g per fine cell,
                        one write per coarse cell
     prolong_cubic      stencil_prolong_cubic: one write of u per fine cell,
                        one read of e per coarse cell
   Achieved bytes per second are those compulsory bytes over the time, against
   stencil_copy_bandwidth in the same run; stencil_restrict_residual and
   stencil_prolong_add of profiles/mg_bench.json (same shapes) are set beside
   them where that file has the shape.
2. The pass against the zero-start solve, 255^3 and 511^3 fp64, the problem of
   §5.9 (the reference initial field's ghost cells, a seeded uniform(-1, 1) *
   1e-3 source; V(2,2), omega = 6/7, 8 coarse sweeps, every level): one
   fmg(cycles=2); then stencil_mg_solve from a zero interior until the fine
   residual's max norm is at or below the residual the pass reached (a check
   after every cycle, as §5.9 timed it), and the same number of V-cycles
   without the checks.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stencil_amd import multigrid as mgm
from stencil_amd.engine import JacobiEngine, StencilSpec, copy_bandwidth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("fp64", 255), ("fp64", 511), ("fp32", 255), ("fp32", 511))
CYCLES = 2


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(v):
    return [round(min(v), 4), round(max(v), 4)]


def mg_bench_beside(dtype, n):
    """restrict_fused / prolong_fused of profiles/mg_bench.json at this shape, or None."""
    path = os.path.join(ROOT, "profiles", "mg_bench.json")
    if not os.path.exists(path):
        return None
    for t in json.load(open(path)).get("transfers", []):
        if t["dtype"] == dtype and t["n"] == n:
            return {k: {"ms": t["ms"][k], "achieved_GBps": t["achieved_GBps"][k], "fraction_of_copy": t["fraction_of_copy"][k]}
                    for k in ("restrict_fused", "prolong_fused")}
    return None


def bench_transfers(dtype, n, rounds, reps):
    fine = JacobiEngine(StencilSpec(dims=3, dtype=dtype), n, n, n, device=0)
    coarse = mgm.coarsen(fine)
    rng = np.random.default_rng(7)
    m = (n - 1) // 2
    for grid in (fine.a, fine.b, coarse.a, coarse.b):
        grid.zero_()
    fine.interior(fine.b).copy_(torch.from_numpy(rng.uniform(-1, 1, (n, n, n))).to(fine.torch_dtype))
    coarse.with_ghosts(coarse.b).copy_(torch.from_numpy(rng.standard_normal((m + 2, m + 2, m + 2))).to(fine.torch_dtype))
    torch.cuda.synchronize()
    es = fine.spec.elem_bytes
    cells, ccells = float(n) ** 3, float(m) ** 3
    paths = {"restrict_source": lambda: mgm.restrict_source(fine, fine.b, coarse, coarse.a),
             "prolong_cubic": lambda: mgm.prolong_cubic(coarse, coarse.b, fine, fine.a)}
    for fn in paths.values():  # untimed
        fn()
        fn()
    torch.cuda.synchronize()
    copy = copy_bandwidth(int(cells * es) // 16 * 16, reps=10)
    ms = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            ms[name].append(timed(fn, reps))
    moved = (cells + ccells) * es
    gbps = {k: [round(moved / (t * 1e-3) / 1e9, 1) for t in v] for k, v in ms.items()}
    return {"dtype": dtype, "n": n, "reps_per_timing": reps, "ms": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "compulsory_bytes": moved, "achieved_GBps": gbps, "copy_kernel_GBps": round(copy, 1),
            "fraction_of_copy": {k: [round(x / copy, 3) for x in v] for k, v in gbps.items()},
            "mg_bench_json": mg_bench_beside(dtype, n)}


def bench_pass(n, rounds):
    spec = StencilSpec(dims=3, dtype="fp64")
    mg = mgm.PoissonMultigrid(spec, n, n, n, device=0)
    e = JacobiEngine(spec, n, n, n, device=0)
    e.reset("reference")
    start = e.to_numpy(e.a)
    start[1:-1, 1:-1, 1:-1] = 0.0   # the zero start; the ghost shell is the reference's boundary data
    del e
    torch.cuda.empty_cache()
    mg.set_source(np.random.default_rng(20260).uniform(-1.0, 1.0, (n, n, n)) * 1e-3)

    def reset():
        mg.set_field(start)
        torch.cuda.synchronize()

    reset()
    residual_start = mg.residual_norm("max")
    mg.fmg(cycles=CYCLES)          # untimed: every launch shape of the pass and of the cycles
    target = mg.residual_norm("max")
    reset()
    first = mg.solve(target, 100, check_every=1, timed=True)   # untimed round; fixes the cycle count
    cycles = first.iterations
    ms = {"fmg": [], "solve_with_checks": [], "vcycles_alone": []}
    for _ in range(rounds):
        reset()
        ms["fmg"].append(timed(lambda: mg.fmg(cycles=CYCLES)))
        assert mg.residual_norm("max") == target   # bitwise defined: every round ends on the same residual
        reset()
        r = mg.solve(target, 100, check_every=1, timed=True)
        assert (r.iterations, r.converged) == (cycles, first.converged) and r.norm == first.norm
        ms["solve_with_checks"].append(r.ms)
        reset()
        ms["vcycles_alone"].append(timed(lambda: mg.vcycle(cycles=cycles)))
    plan, cyc = mg.fmg_plan(cycles=CYCLES), mg.plan()
    out = {"dtype": "fp64", "n": n, "levels": mg.levels, "cycles_per_level": CYCLES, "residual_zero_start": residual_start,
           "residual_after_fmg": target, "fmg_launches": plan["launches"], "vcycle_launches": cyc["launches"],
           "solve_cycles_to_the_same_residual": cycles, "solve_converged": bool(first.converged),
           "solve_residual": first.norm, "solve_launches_without_checks": cycles * cyc["launches"],
           "ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
           "ms_min_max": {k: spread(v) for k, v in ms.items()},
           "solve_over_fmg_per_round": [round(s / f, 2) for s, f in zip(ms["solve_with_checks"], ms["fmg"])],
           "vcycles_over_fmg_per_round": [round(s / f, 2) for s, f in zip(ms["vcycles_alone"], ms["fmg"])],
           "fmg_in_vcycle_times_per_round": [round(f / (s / cycles), 2) for s, f in zip(ms["vcycles_alone"], ms["fmg"])],
           "fmg_faster_than_vcycles_every_round": max(ms["fmg"]) < min(ms["vcycles_alone"])}
    mg.close()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fmg_bench.json")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="launches per timing of a transfer kernel")
    ap.add_argument("--small", action="store_true", help="a rehearsal at small sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fmg_bench needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "transfers": [], "pass": []}
    for dtype, n in ((("fp64", 63), ("fp32", 63)) if a.small else SHAPES):
        out["transfers"].append(bench_transfers(dtype, n, a.rounds, a.reps))
        torch.cuda.empty_cache()
    for n in ((63,) if a.small else (255, 511)):
        out["pass"].append(bench_pass(n, a.rounds))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
