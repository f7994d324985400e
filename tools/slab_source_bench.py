#!/usr/bin/env python3
"""What the source term costs in a slab job, and which form its full rounds
should take.

    python tools/slab_source_bench.py [--out profiles/slab_source_bench.json] [--sweeps 200] [--rounds 3]

In one process on one GPU (tools/source_bench.py's method), `--sweeps` sweeps
per job, `--rounds` alternating rounds (1, 2, 3, 4, 1, 2, 3, 4, ...):

  ring      a one-slab periodic RCCL ring (the rehearsal of an interior rank:
            the slab's halo planes, the exchange's kernels, the round forms --
            but the transfer goes to the same GPU), at 512^3 fp64, 1024^3 fp32
            and 512^3 fp32:
              1 plain        stencil_slab_run -- no source term;
              2 signalled    stencil_slab_run_source, full rounds as one
                             face-signalled source launch where the job's rounds
                             allow it (the form is reported: a job of K = 5
                             rounds or staged rounds has none);
              3 boundary     stencil_slab_run_source with
                             STENCIL_SLAB_SOURCE_SIGNAL=0: boundary + interior;
              4 single grid  stencil_iterate_source on one grid of the same
                             size, for reference.
  shared    two slabs sharing the device (copy exchange) against the single
            grid, 512^3 fp64: a REHEARSAL ONLY -- both slabs' launches take
            turns on one GPU, so the job can at best match the single grid.

Paths 1-3 report the host wall time of the whole job (stencil_slab_run*'s
elapsed_ms: all streams synchronised at both ends), path 4 device time between
events.  Everything runs untimed first (code objects, schedules, RCCL's lazy
connections, stencil_prepare for the single grid, the clock).  Runs across
distinct GPUs and real xGMI exchange are not measured here: every box has one
GPU.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stencil_amd.engine import JacobiEngine, SlabJob, StencilSpec

SHAPES = (("fp64", 512, 512, 512), ("fp32", 1024, 1024, 1024), ("fp32", 512, 512, 512))
KNOB = "STENCIL_SLAB_SOURCE_SIGNAL"
FORMS = {0: "boundary + interior", 1: "face-signalled", 3: "serial"}


def source_array(dtype, nx, ny, nz):
    a = np.zeros((nz + 2, ny + 2, nx + 2), dtype=np.float64 if dtype == "fp64" else np.float32)
    a[1:-1, 1:-1, 1:-1] = 1e-3
    return a


def stats(ms, cells):
    rate = [cells / (t * 1e-3) / 1e9 for t in ms]
    return {"ms": [round(t, 3) for t in ms], "gcells_per_s": [round(r, 1) for r in rate],
            "gcells_per_s_min_max": [round(min(rate), 1), round(max(rate), 1)]}


def with_knob(value, fn):
    old = os.environ.get(KNOB)
    os.environ[KNOB] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[KNOB]
        else:
            os.environ[KNOB] = old


def bench(dtype, nx, ny, nz, sweeps, rounds, devices, exchange, periodic):
    spec = StencilSpec(dims=3, dtype=dtype)
    job = SlabJob(spec, nx, ny, nz, devices, exchange=exchange, periodic=periodic)
    job.set_source(source_array(dtype, nx, ny, nz))
    e = JacobiEngine(spec, nx, ny, nz, device=0)
    e.set_source(torch.full((nz, ny, nx), 1e-3, dtype=e.torch_dtype, device=e.device))

    def single():
        e.reset("reference")
        torch.cuda.synchronize()
        return e.iterate_source(sweeps, timed=True)[1]

    def slab(run):
        job.fill_initial("reference")
        return run(sweeps)
    paths = {"plain": lambda: slab(job.run),
             "source_signalled": lambda: with_knob("1", lambda: slab(job.run_source)),
             "source_boundary": lambda: with_knob("0", lambda: slab(job.run_source)),
             "single_grid_source": single}
    forms = {"plain": job.round_form(), "source_signalled": with_knob("1", job.source_round_form),
             "source_boundary": with_knob("0", job.source_round_form)}
    # untimed: every path's launches, schedules and connections, the clock
    e.reset("reference")
    e.prepare()
    e.iterate_source(24)
    job.fill_initial("reference")
    job.run(24)
    with_knob("1", lambda: job.run_source(24))
    with_knob("0", lambda: job.run_source(24))
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            ms[name].append(fn())
    info = dict(job.round_info(), sweeps_per_round=job.info(0)["sweeps_per_round"], source_plan=job.source_plan(sweeps),
                forms={k: FORMS.get(v, str(v)) for k, v in forms.items()})
    job.close()
    cells = float(nx) * ny * nz * sweeps
    res = {k: stats(v, cells) for k, v in ms.items()}
    sig, bnd = res["source_signalled"]["gcells_per_s_min_max"], res["source_boundary"]["gcells_per_s_min_max"]
    out = {"dtype": dtype, "nx": nx, "ny": ny, "nz": nz, "sweeps": sweeps, "slabs": len(devices), "exchange": exchange,
           "periodic": periodic, "job": info, "paths": res,
           "source_over_plain_per_round": [round(p / s, 3) for p, s in zip(ms["plain"], ms["source_signalled"])],
           "forms_differ": forms["source_signalled"] != forms["source_boundary"],
           "signalled_range_at_or_above_boundary_range": sig[0] >= bnd[1]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/slab_source_bench.json")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a rehearsal at small sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("slab_source_bench needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    shapes = (("fp64", 130, 64, 40), ("fp32", 130, 64, 40)) if a.small else SHAPES
    out = {"device": torch.cuda.get_device_name(0), "method": "one process, untimed launches first, alternating rounds, "
           "wall time per whole job (single grid: device time)", "ring": [], "shared": []}
    for dtype, nx, ny, nz in shapes:
        out["ring"].append(bench(dtype, nx, ny, nz, a.sweeps, a.rounds, [0], "rccl", True))
        torch.cuda.empty_cache()
    dtype, nx, ny, nz = shapes[0]
    out["shared"].append(dict(bench(dtype, nx, ny, nz, a.sweeps, a.rounds, [0, 0], "copy", False),
                              note="rehearsal only: two slabs take turns on one GPU"))
    deciding = [s for s in out["ring"] if s["forms_differ"]]
    out["signalled_default"] = bool(deciding) and all(s["signalled_range_at_or_above_boundary_range"] for s in deciding)
    out["unmeasured"] = "runs across distinct GPUs and real xGMI exchange (every box has one GPU)"
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
