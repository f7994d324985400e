#!/usr/bin/env python3
"""Known answers of the multigrid solve tests/mg_ref.py GOLDEN describes: the
fine residual's max norm before the first and after every V-cycle, computed by
the numpy statement of the cycle (tests/mg_ref.py) over the CPU oracle's
sweeps.  Writes tests/golden/mg_known_answers.json; tests/test_mg_ref.py
checks the helper against it and tests/test_gpu_mg.py the GPU solve.

usage: make oracle && python tests/golden/make_mg_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import mg_ref as mr  # noqa: E402


def main():
    g = mr.GOLDEN
    h = mr.golden_hierarchy()
    start = mr.residual_norm(h.p[0], h.u[0], h.g[0])
    _, _, _, history = mr.solve(h, 0.0, g["cycles"], 1, g["pre"], g["post"], g["coarse_sweeps"], g["omegas"])
    meta = {"_source": "tests/mg_ref.py: V-cycles of the numpy statement of include/stencil_hip.h's multigrid "
                       "definitions over the CPU oracle's sweeps; max |residual| of the fine level, as Python floats "
                       "(repr round-trips a double exactly) and as hex.",
            "setup": {k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items()},
            "residual_start": start, "residual_start_hex": start.hex(),
            "residual_after_cycle": history, "residual_after_cycle_hex": [v.hex() for v in history]}
    with open(os.path.join(HERE, "mg_known_answers.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    ratios = [b / a for a, b in zip([start] + history[:-1], history)]
    print("residuals:", [start] + history)
    print("ratios:", ratios)


if __name__ == "__main__":
    main()
