#!/usr/bin/env python3
"""Known answers of the full multigrid pass on the model problem of
tests/fmg_ref.py GOLDEN (DESIGN.md §5.10's table): for 15^3 and 31^3 fp64 the
discretization error disc = max |u_h - u*|, and for the cubic and the
trilinear prolongation at 1 and 2 cycles per level the algebraic error
alg = max |u_FMG - u_h|, alg / disc, and the zero-start V-cycles that reach
the same alg.  Computed by the numpy statement of the pass (tests/fmg_ref.py)
over the CPU oracle's sweeps.  Writes tests/golden/fmg_known_answers.json;
tests/test_fmg_ref.py checks the helper against it and tests/test_gpu_fmg.py
the GPU pass.

usage: make oracle && python tests/golden/make_fmg_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import fmg_ref as fr  # noqa: E402


def main():
    g = fr.GOLDEN
    meta = {"_source": "tests/fmg_ref.py: the numpy statement of include/stencil_hip.h's full multigrid pass over the "
                       "CPU oracle's sweeps, on -Laplace u = f, u* = sin(pi x) cos(pi y) e^z on the unit cube; "
                       "Python floats (repr round-trips a double exactly).",
            "setup": {k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items()},
            "problems": [fr.golden_ratios(n) for n in g["sizes"]]}
    with open(os.path.join(HERE, "fmg_known_answers.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    for p in meta["problems"]:
        print(p["n"], "disc", p["disc"], {k: (v["ratio"], v["zero_start_cycles"]) for k, v in p.items()
                                          if isinstance(v, dict)})


if __name__ == "__main__":
    main()
