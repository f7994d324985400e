#!/usr/bin/env python3
"""What relaxing the source sweeps costs per sweep and what a Chebyshev
schedule saves in sweeps.

    python tools/relax_bench.py [--out profiles/relax_bench.json] [--sweeps 200] [--rounds 3]

In one process on one GPU, at 512^3 fp64 and 1024^3 fp32, after every path's
untimed launches and stencil_prepare, `--rounds` alternating rounds, device
time between the job's own events, min-max reported:

  rate      Gcell/s of stencil_iterate_relax (constant weight 0.8) beside
            stencil_iterate_source, `--sweeps` sweeps per job.
  solve     sweeps and device time to max-norm 1e-6 from the reference field
            with g = 0, check_every = 64: stencil_iterate_until_source against
            stencil_iterate_until_relax with the P = 64 Chebyshev schedule.

Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stencil_amd.engine import JacobiEngine, StencilSpec, chebyshev_weights

SHAPES = (("fp64", 512, 512, 512), ("fp32", 1024, 1024, 1024))
TOL, EVERY, PERIOD = 1e-6, 64, 64


def bench(dtype, nx, ny, nz, sweeps, rounds, cap):
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), nx, ny, nz, device=0)
    e.set_source(torch.zeros((nz, ny, nx), dtype=e.torch_dtype, device=e.device))
    cheb = chebyshev_weights(e.spec, nx, ny, nz, PERIOD)
    # untimed: every path's launches, the schedule trials, the clock
    e.reset("reference")
    e.prepare()
    e.iterate_source(30)
    e.iterate_relax(30, 0.8)
    e.iterate_until_source(0.0, 2 * EVERY, check_every=EVERY)
    e.iterate_until_relax(0.0, 2 * EVERY, cheb, check_every=EVERY)
    torch.cuda.synchronize()
    ms = {"source": [], "relax": []}
    solve = {"source": [], "chebyshev": []}
    for _ in range(rounds):
        e.reset("reference")
        ms["source"].append(e.iterate_source(sweeps, timed=True)[1])
        e.reset("reference")
        ms["relax"].append(e.iterate_relax(sweeps, 0.8, timed=True)[1])
        e.reset("reference")
        r = e.iterate_until_source(TOL, cap, check_every=EVERY, timed=True)
        solve["source"].append({"sweeps": r.iterations, "converged": r.converged, "norm": r.norm, "ms": round(r.ms, 3)})
        e.reset("reference")
        r = e.iterate_until_relax(TOL, cap, cheb, check_every=EVERY, timed=True)
        solve["chebyshev"].append({"sweeps": r.iterations, "converged": r.converged, "norm": r.norm, "ms": round(r.ms, 3)})
    cells = float(nx) * ny * nz * sweeps
    rate = {k: [round(cells / (t * 1e-3) / 1e9, 1) for t in v] for k, v in ms.items()}
    return {"dtype": dtype, "nx": nx, "ny": ny, "nz": nz, "sweeps": sweeps, "cap": cap, "tol": TOL, "check_every": EVERY,
            "period": PERIOD, "relax_plan": e.relax_plan(sweeps), "ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
            "gcells_per_s": rate, "gcells_per_s_min_max": {k: [min(v), max(v)] for k, v in rate.items()},
            "relax_over_source_per_round": [round(s / r, 3) for s, r in zip(ms["source"], ms["relax"])], "solve": solve}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/relax_bench.json")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cap", type=int, default=4096, help="most sweeps of a solve")
    ap.add_argument("--small", action="store_true", help="a rehearsal at small sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("relax_bench needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    shapes = (("fp64", 96, 64, 40), ("fp32", 128, 64, 40)) if a.small else SHAPES
    out = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for dtype, nx, ny, nz in shapes:
        out["shapes"].append(bench(dtype, nx, ny, nz, a.sweeps, a.rounds, a.cap))
        torch.cuda.empty_cache()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
