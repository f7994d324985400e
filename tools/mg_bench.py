#!/usr/bin/env python3
"""What the fused multigrid transfers gain, and what a multigrid solve gains
over Chebyshev Jacobi.

    python tools/mg_bench.py [--out profiles/mg_bench.json] [--rounds 3] [--small]

One process on one GPU; every path runs untimed first (code objects, the
strip kernel's schedule trials, the clock); `--rounds` alternating rounds;
device time between events.

1. Transfer kernels, at 511^3 and 255^3 fp64 and 511^3 fp32:
     restrict fused     stencil_restrict_residual (the residual stays on chip)
     restrict unfused   stencil_sweepk_source with steps = 1 into a scratch
                        grid, a torch subtract, torch slicing and adds for the
                        full weighting
     prolong fused      stencil_prolong_add
     prolong unfused    torch slicing, adds and multiplies, then an add
   torch's element-wise ops are the IEEE ops: the two paths are first checked
   bitwise equal at a small shape.  Achieved bytes per second are the
   compulsory bytes (restriction: one read of u and of g per fine cell, one
   write per coarse cell; prolongation: one read and one write of u per fine
   cell, one read per coarse cell) over the time, against
   stencil_copy_bandwidth in the same run.
2. Whole solve, 255^3 fp64, from the reference initial field with a seeded
   uniform(-1, 1) * 1e-3 source: stencil_mg_solve (all levels, V(2,2),
   omega = 6/7, 8 coarse sweeps) until the fine residual's max norm has fallen
   by 1e-6, against stencil_iterate_until_relax with the P = 64 Chebyshev
   schedule run for the number of sweeps (a multiple of 64, found in an
   untimed pass) after which residual_norm is at or below what multigrid
   reached.
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
from stencil_amd.engine import JacobiEngine, StencilSpec, chebyshev_weights, copy_bandwidth

SHAPES = (("fp64", 511), ("fp64", 255), ("fp32", 511))
CHEBY_PERIOD = 64
REDUCTION = 1e-6


def weigh(v, axis):
    """The 1-D full weighting along `axis` with torch slicing: (lo + hi) + (mid + mid)."""
    n = v.shape[axis]
    lo, mid, hi = (v.narrow(axis, first, n - 2)[(slice(None),) * axis + (slice(None, None, 2),)] for first in (0, 1, 2))
    return (lo + hi) + (mid + mid)


def restrict_unfused(fine, coarse, dst):
    """J into fine.b by a single source sweep, r = J - u, the full weighting by slices; into dst's interior."""
    fine.sweepk_source(fine.a, fine.b, 0, fine.slow_extent, 1)
    r = fine.interior(fine.b) - fine.interior(fine.a)
    coarse.interior(dst).copy_(0.0625 * weigh(weigh(weigh(r, 2), 1), 0))


def interp(e, axis):
    """The 1-D interpolation along `axis` with torch slicing: m + 2 -> 2 m + 1."""
    m = e.shape[axis] - 2
    shape = list(e.shape)
    shape[axis] = 2 * m + 1
    out = torch.empty(shape, dtype=e.dtype, device=e.device)
    pre = (slice(None),) * axis
    out[pre + (slice(0, None, 2),)] = 0.5 * (e.narrow(axis, 0, m + 1) + e.narrow(axis, 1, m + 1))
    out[pre + (slice(1, None, 2),)] = e.narrow(axis, 1, m)
    return out


def prolong_unfused(coarse, e, fine, u):
    fine.interior(u).add_(interp(interp(interp(coarse.with_ghosts(e), 2), 1), 0))


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def pair(dtype, size, seed=7):
    fine = JacobiEngine(StencilSpec(dims=3, dtype=dtype), *size, device=0)
    coarse = mgm.coarsen(fine)
    rng = np.random.default_rng(seed)
    nx, ny, nz = size
    for grid in (fine.a, fine.b, coarse.a, coarse.b):
        grid.zero_()
    fine.with_ghosts(fine.a).copy_(torch.from_numpy(rng.standard_normal((nz + 2, ny + 2, nx + 2))).to(fine.torch_dtype))
    fine.set_source(torch.from_numpy(rng.uniform(-1, 1, (nz, ny, nx))).to(fine.torch_dtype))
    cz, cy, cx = (int(coarse.prob.nz), int(coarse.prob.ny), int(coarse.prob.nx))
    coarse.with_ghosts(coarse.b).copy_(torch.from_numpy(rng.standard_normal((cz + 2, cy + 2, cx + 2))).to(fine.torch_dtype))
    torch.cuda.synchronize()
    return fine, coarse


def same_result_check():
    """Fused and un-fused transfers give the same bits (a small grid with ragged tiles)."""
    out = {}
    for dtype in ("fp32", "fp64"):
        fine, coarse = pair(dtype, (131, 61, 29))
        it = torch.int32 if dtype == "fp32" else torch.int64
        mgm.restrict_residual(fine, fine.a, fine.source, coarse, coarse.a)
        other = torch.zeros_like(coarse.a)
        restrict_unfused(fine, coarse, other)
        torch.cuda.synchronize()
        out[f"restrict_{dtype}"] = bool(torch.equal(coarse.a.view(it), other.view(it)))
        u2 = fine.a.clone()
        mgm.prolong_add(coarse, coarse.b, fine, fine.a)
        prolong_unfused(coarse, coarse.b, fine, u2)
        torch.cuda.synchronize()
        out[f"prolong_{dtype}"] = bool(torch.equal(fine.a.view(it), u2.view(it)))
    return out


def bench_transfers(dtype, n, rounds, reps):
    size = (n, n, n)
    fine, coarse = pair(dtype, size)
    es = fine.spec.elem_bytes
    cells, ccells = float(n) ** 3, float((n - 1) // 2) ** 3
    other = torch.zeros_like(coarse.a)
    paths = {"restrict_fused": lambda: mgm.restrict_residual(fine, fine.a, fine.source, coarse, coarse.a),
             "restrict_unfused": lambda: restrict_unfused(fine, coarse, other),
             "prolong_fused": lambda: mgm.prolong_add(coarse, coarse.b, fine, fine.a),
             "prolong_unfused": lambda: prolong_unfused(coarse, coarse.b, fine, fine.a)}
    # the prolongation adds to u in place; a small e keeps u finite over every repetition
    coarse.b.mul_(1e-6)
    for fn in paths.values():  # untimed
        fn()
        fn()
    torch.cuda.synchronize()
    copy = copy_bandwidth(int(cells * es) // 16 * 16, reps=10)  # the copy kernel moves whole 16-B vectors
    ms = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            ms[name].append(timed(fn, reps))
    bytes_moved = {"restrict": (2 * cells + ccells) * es, "prolong": (2 * cells + ccells) * es}
    gbps = {k: [round(bytes_moved[k.split("_")[0]] / (t * 1e-3) / 1e9, 1) for t in v] for k, v in ms.items()}
    return {"dtype": dtype, "n": n, "reps_per_timing": reps, "ms": {k: [round(t, 4) for t in v] for k, v in ms.items()},
            "compulsory_bytes": bytes_moved, "achieved_GBps": gbps, "copy_kernel_GBps": round(copy, 1),
            "fraction_of_copy": {k: [round(x / copy, 3) for x in v] for k, v in gbps.items()},
            "restrict_fused_over_unfused_per_round": [round(u / f, 2) for u, f in
                                                      zip(ms["restrict_unfused"], ms["restrict_fused"])],
            "prolong_fused_over_unfused_per_round": [round(u / f, 2) for u, f in
                                                     zip(ms["prolong_unfused"], ms["prolong_fused"])],
            "restrict_fused_range_above_unfused_every_round": min(gbps["restrict_fused"]) > max(gbps["restrict_unfused"]),
            "prolong_fused_range_above_unfused_every_round": min(gbps["prolong_fused"]) > max(gbps["prolong_unfused"])}


def bench_solve(dtype, n, rounds, max_sweeps):
    spec = StencilSpec(dims=3, dtype=dtype)
    mg = mgm.PoissonMultigrid(spec, n, n, n, device=0)
    e = JacobiEngine(spec, n, n, n, device=0)
    src = torch.from_numpy(np.random.default_rng(20260).uniform(-1.0, 1.0, (n, n, n)) * 1e-3).to(e.torch_dtype)
    e.set_source(src)
    e.reset("reference")
    start_field = e.to_numpy(e.a)
    mg.set_source(src)
    weights = chebyshev_weights(spec, n, n, n, CHEBY_PERIOD)

    def mg_reset():
        mg.set_field(start_field)

    def cheby_reset():
        e.reset("reference")
        torch.cuda.synchronize()

    mg_reset()
    start = mg.residual_norm("max")
    tol = start * REDUCTION
    # untimed: the cycle's launches on every level; then the solve whose residual sets the target
    mg.vcycle()
    mg_reset()
    first = mg.solve(tol, 100, check_every=1, timed=True)
    target = first.norm
    # untimed: the sweeps (a multiple of the period) after which Chebyshev's residual is at or below the target
    cheby_reset()
    cur, sweeps, cheby_res = e.a, 0, float("inf")
    while sweeps < max_sweeps:
        # iterate_relax runs from e.a: keep the field there
        if cur is not e.a:
            e.a.copy_(cur)
        cur, _ = e.iterate_relax(CHEBY_PERIOD, weights, phase=sweeps)
        sweeps += CHEBY_PERIOD
        cheby_res = mgm._scalar_norm(*mgm.residual_norms(e, cur, e.source), "max")
        if cheby_res <= target:
            break
    reached = cheby_res <= target
    ms = {"multigrid": [], "chebyshev": []}
    cycles, checks = [], []
    for _ in range(rounds):
        mg_reset()
        r = mg.solve(tol, 100, check_every=1, timed=True)
        ms["multigrid"].append(r.ms)
        cycles.append(r.iterations)
        assert r.norm == target, (r.norm, target)  # bitwise defined: every round ends on the same residual
        cheby_reset()
        # tol = 0: never met, so the call runs exactly `sweeps` sweeps with its update check every period
        c = e.iterate_until_relax(0.0, sweeps, weights, check_every=CHEBY_PERIOD, norm="max", timed=True)
        ms["chebyshev"].append(c.ms)
        checks.append(mgm._scalar_norm(*mgm.residual_norms(e, c.grid, e.source), "max"))
    out = {"dtype": dtype, "n": n, "levels": mg.levels, "cycle_plan": mg.plan(), "residual_start": start,
           "residual_target": target, "reduction_asked": REDUCTION, "multigrid_cycles": cycles,
           "chebyshev_period": CHEBY_PERIOD, "chebyshev_sweeps": sweeps, "chebyshev_reached_target": reached,
           "chebyshev_residual": checks, "ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
           "chebyshev_over_multigrid_per_round": [round(c / m, 2) for c, m in zip(ms["chebyshev"], ms["multigrid"])]}
    mg.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mg_bench.json")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="launches per timing of a transfer path")
    ap.add_argument("--max-sweeps", type=int, default=64 * 400, help="cap of the Chebyshev run")
    ap.add_argument("--small", action="store_true", help="a rehearsal at small sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mg_bench needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "same_bits_fused_unfused": same_result_check(), "transfers": []}
    assert all(out["same_bits_fused_unfused"].values()), out
    for dtype, n in ((("fp64", 63), ("fp32", 63)) if a.small else SHAPES):
        out["transfers"].append(bench_transfers(dtype, n, a.rounds, a.reps))
        torch.cuda.empty_cache()
    out["solve"] = bench_solve("fp64", 63 if a.small else 255, a.rounds, a.max_sweeps)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
