#!/usr/bin/env python3
"""What the source term costs and what fusing it gains.

    python tools/source_bench.py [--out profiles/source_bench.json] [--sweeps 200] [--rounds 3]

In one process on one GPU, at 512^3 fp64, 2048^2 x 512 fp64 and 1024^3 fp32,
`--sweeps` sweeps per job, three paths, `--rounds` alternating rounds (1, 2,
3, 1, 2, 3, ...), device time between events around each whole job:

  1 plain     stencil_iterate -- no source term; the context number.
  2 unfused   what a source term took before the fused launches: per sweep one
              stencil_sweep and an element-wise torch add of the source over
              the interior (the same two roundings: bitwise path 3's result,
              checked once at a small size before anything is timed).
  3 fused     stencil_iterate_source.

Every path runs its launches untimed first (code objects, the strip kernel's
one-time schedule trial, the clock: stencil_prepare for path 1, a short job
for the others).  Prints one JSON line and writes it to --out.  The byte
model (fp64, per cell and sweep, purely memory-bound): path 1 moves 16 / K1,
path 3 24 / K3, path 2 at least 16 + 24 = 40.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stencil_amd.engine import JacobiEngine, StencilSpec

SHAPES = (("fp64", 512, 512, 512), ("fp64", 2048, 2048, 512), ("fp32", 1024, 1024, 1024))


def unfused_job(e, sweeps):
    """Path 2: returns the grid that holds the result."""
    n = e.slow_extent
    cur, nxt = e.a, e.b
    src = e.interior(e.source)
    for _ in range(sweeps):
        e.sweep(cur, nxt, 0, n)
        e.interior(nxt).add_(src)
        cur, nxt = nxt, cur
    return cur


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def same_result_check():
    """Paths 2 and 3 give the same bits (a small grid with ragged tiles)."""
    out = {}
    for dtype in ("fp32", "fp64"):
        e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), 131, 61, 29, device=0)
        rng = np.random.default_rng(3)
        e.set_source(rng.uniform(-1, 1, (29, 61, 131)))
        e.reset("random", 5)
        fused = e.iterate_source(11)[0].clone()
        e.reset("random", 5)
        unfused = unfused_job(e, 11)
        torch.cuda.synchronize()
        it = torch.int32 if dtype == "fp32" else torch.int64
        out[dtype] = bool(torch.equal(fused.view(it), unfused.view(it)))
    return out


def bench(dtype, nx, ny, nz, sweeps, rounds):
    e = JacobiEngine(StencilSpec(dims=3, dtype=dtype), nx, ny, nz, device=0)
    e.set_source(torch.full((nz, ny, nx), 1e-3, dtype=e.torch_dtype, device=e.device))
    paths = {"plain": lambda: e.iterate(sweeps), "unfused": lambda: unfused_job(e, sweeps),
             "fused": lambda: e.iterate_source(sweeps)}
    # untimed: every path's launches, the schedule trials, the clock
    e.reset("reference")
    e.prepare()
    e.iterate(12)
    e.iterate_source(30)
    unfused_job(e, 4)
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            e.reset("reference")
            torch.cuda.synchronize()
            ms[name].append(timed(fn))
    cells = float(nx) * ny * nz * sweeps
    rate = {k: [round(cells / (t * 1e-3) / 1e9, 1) for t in v] for k, v in ms.items()}
    spread = {k: round((max(v) - min(v)) / min(v), 4) for k, v in ms.items()}
    return {"dtype": dtype, "nx": nx, "ny": ny, "nz": nz, "sweeps": sweeps, "plain_steps": e.fuse_steps,
            "source_plan": e.source_plan(sweeps), "ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
            "gcells_per_s": rate, "spread_between_rounds": spread,
            "fused_over_unfused_per_round": [round(u / f, 3) for u, f in zip(ms["unfused"], ms["fused"])],
            "fused_over_plain_per_round": [round(p / f, 3) for p, f in zip(ms["plain"], ms["fused"])],
            "fused_beats_unfused_every_round_by_more_than_spread":
                all(f * (1 + max(spread["fused"], spread["unfused"])) < u for u, f in zip(ms["unfused"], ms["fused"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/source_bench.json")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a rehearsal at small sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("source_bench needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    shapes = (("fp64", 96, 64, 40), ("fp32", 128, 64, 40)) if a.small else SHAPES
    out = {"device": torch.cuda.get_device_name(0), "same_bits_fused_unfused": same_result_check(), "shapes": []}
    assert all(out["same_bits_fused_unfused"].values()), out
    for dtype, nx, ny, nz in shapes:
        out["shapes"].append(bench(dtype, nx, ny, nz, a.sweeps, a.rounds))
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
