#!/usr/bin/env python3
"""What relaxing the source rounds costs a slab job per sweep, and what a
Chebyshev schedule saves it in sweeps and wall time.

    python tools/slab_relax_bench.py [--out profiles/slab_relax_bench.json] [--sweeps 200] [--rounds 3]

In one process on one GPU (tools/relax_bench.py's method), on a one-slab
periodic RCCL ring -- the rehearsal of an interior rank: the slab's halo planes,
the exchange's kernels and the round forms, but the transfer goes to the same
GPU -- at 512^2 x 128 fp64 and 1024^2 x 128 fp32, after every path's untimed
launches, `--rounds` alternating rounds, min-max reported:

  rate      Gcell/s of stencil_slab_run_relax (constant weight 0.8) beside
            stencil_slab_run_source, `--sweeps` sweeps per job; the forms of
            both jobs' full rounds are reported.
  solve     sweeps and wall time to max-norm 1e-6 from the reference field with
            g = 0, check_every = 64: stencil_slab_run_until_source against
            stencil_slab_run_until_relax with a P = 64 Chebyshev schedule.  The
            ring has no Dirichlet ends in z, so the schedule is
            stencil_chebyshev_weights' for the same plane with an unbounded z
            extent (cos(pi / (nz + 1)) -> 1): the ring's own spectral radius.

Every time is the host wall time of the whole call (stencil_slab_run*'s
elapsed_ms: all streams synchronised at both ends).  There is no pass / fail
threshold.  Runs across distinct GPUs and real xGMI exchange are not measured
here.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stencil_amd.engine import SlabJob, StencilSpec, chebyshev_weights

SHAPES = (("fp64", 512, 512, 128), ("fp32", 1024, 1024, 128))
TOL, EVERY, PERIOD = 1e-6, 64, 64
UNBOUNDED = 1 << 40  # the z extent handed to stencil_chebyshev_weights for a ring
FORMS = {0: "boundary + interior", 1: "face-signalled", 3: "serial"}


def bench(dtype, nx, ny, nz, sweeps, rounds, cap):
    spec = StencilSpec(dims=3, dtype=dtype)
    job = SlabJob(spec, nx, ny, nz, [0], exchange="rccl", periodic=True)
    job.set_source(np.zeros((nz, ny, nx), dtype=np.float64 if dtype == "fp64" else np.float32))
    cheb = chebyshev_weights(spec, nx, ny, UNBOUNDED, PERIOD)

    def fresh(fn):
        job.fill_initial("reference")
        return fn()
    # untimed: every path's launches, schedules and connections, the clock
    fresh(lambda: job.run_source(24))
    fresh(lambda: job.run_relax(24, 0.8))
    fresh(lambda: job.run_until_source(0.0, 2 * EVERY, check_every=EVERY))
    fresh(lambda: job.run_until_relax(0.0, 2 * EVERY, cheb, check_every=EVERY))
    torch.cuda.synchronize()
    ms = {"source": [], "relax": []}
    solve = {"source": [], "chebyshev": []}
    for _ in range(rounds):
        ms["source"].append(fresh(lambda: job.run_source(sweeps)))
        ms["relax"].append(fresh(lambda: job.run_relax(sweeps, 0.8)))
        r = fresh(lambda: job.run_until_source(TOL, cap, check_every=EVERY))
        solve["source"].append({"sweeps": r.iterations, "converged": r.converged, "norm": r.norm, "ms": round(r.ms, 3)})
        r = fresh(lambda: job.run_until_relax(TOL, cap, cheb, check_every=EVERY))
        solve["chebyshev"].append({"sweeps": r.iterations, "converged": r.converged, "norm": r.norm, "ms": round(r.ms, 3)})
    info = dict(job.round_info(), sweeps_per_round=job.info(0)["sweeps_per_round"], relax_plan=job.relax_plan(sweeps),
                forms={"source": FORMS.get(job.source_round_form(), "?"), "relax": FORMS.get(job.relax_round_form(), "?")})
    job.close()
    cells = float(nx) * ny * nz * sweeps
    rate = {k: [round(cells / (t * 1e-3) / 1e9, 1) for t in v] for k, v in ms.items()}
    return {"dtype": dtype, "nx": nx, "ny": ny, "nz": nz, "sweeps": sweeps, "cap": cap, "tol": TOL, "check_every": EVERY,
            "period": PERIOD, "job": info, "ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
            "gcells_per_s": rate, "gcells_per_s_min_max": {k: [min(v), max(v)] for k, v in rate.items()},
            "relax_over_source_per_round": [round(s / r, 3) for s, r in zip(ms["source"], ms["relax"])], "solve": solve}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/slab_relax_bench.json")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cap", type=int, default=32768, help="most sweeps of a solve")
    ap.add_argument("--small", action="store_true", help="a rehearsal at small sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("slab_relax_bench needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    shapes = (("fp64", 130, 64, 40), ("fp32", 130, 64, 40)) if a.small else SHAPES
    out = {"device": torch.cuda.get_device_name(0), "method": "one process, one-slab periodic RCCL ring, untimed launches "
           "first, alternating rounds, wall time per whole call", "shapes": []}
    for dtype, nx, ny, nz in shapes:
        out["shapes"].append(bench(dtype, nx, ny, nz, a.sweeps, a.rounds, a.cap))
        torch.cuda.empty_cache()
    out["unmeasured"] = "runs across distinct GPUs and real xGMI exchange"
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
