"""The CLI's convergence-controlled runs (--tol, --check-every, --norm) on the
CPU method: parsing, --print-config, the stopping rule against the oracle, the
exit status.  No GPU."""
import os
import re
import subprocess

import numpy as np

from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "build", "bin", "stencil_main")
BASE = ("-s", "32", "-b", "4", "-m", "CPU")


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def oracle_count(p, tol, every, cap):
    """Sweeps at which the stopping rule ends a run from the reference initial
    condition: blocks of `every` sweeps (the last one shorter), max |update| in
    double after each; (count, converged)."""
    cur = ob.init(p)
    old = cur.copy()
    done = 0
    while done < cap:
        block = min(every, cap - done)
        for _ in range(block):
            ob.sweep(p, cur, old, 0, p.ny)
            cur, old = old, cur
        done += block
        d = ob.interior(p, cur).astype(np.float64) - ob.interior(p, old).astype(np.float64)
        if np.abs(d).max() <= tol:
            return done, True
    return done, False


def test_print_config_shows_defaults_after_existing_keys():
    p = run(*BASE, "-i", "1", "--print-config")
    assert p.returncode == 0, p.stderr
    keys = [kv.split("=", 1)[0] for kv in p.stdout.split()]
    c = dict(kv.split("=", 1) for kv in p.stdout.split())
    assert keys[-3:] == ["tol", "check_every", "norm"] and keys[-4] == "methods" and keys[0] == "matrix_size"
    assert (c["tol"], c["check_every"], c["norm"]) == ("off", "100", "max")
    p = run(*BASE, "-i", "1", "--tol", "1e-3", "--check-every=7", "--norm", "l2", "--print-config")
    c = dict(kv.split("=", 1) for kv in p.stdout.split())
    assert (float(c["tol"]), c["check_every"], c["norm"]) == (1e-3, "7", "l2")


def test_bad_values_exit_1():
    for bad in (("--tol", "-1"), ("--tol", "abc"), ("--check-every", "0"), ("--norm", "l1")):
        p = run(*BASE, "-i", "5", *bad)
        assert p.returncode == 1, bad
        assert p.stderr and "converged" not in p.stdout


def test_tol_with_several_gpus_is_refused():
    p = run("-s", "32", "-b", "4", "-i", "5", "--tol", "1e-3", "--gpus", "2", "-m", "HIP")
    assert p.returncode == 1
    assert "--tol" in p.stderr and "converged" not in p.stdout


def test_cpu_method_stops_where_the_oracle_does():
    prob = ob.problem(2, "fp32", "star", 1, "naive", 32, 32)
    want, conv = oracle_count(prob, 1e-3, 7, 500)
    assert conv and 7 < want < 500 and want % 7 == 0
    p = run(*BASE, "-i", "500", "--tol", "1e-3", "--check-every", "7", "-c")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "The results of method CPU is correct." in p.stdout
    counts = re.findall(r"^\[stencil-amd\] CPU: converged after (\d+) sweeps, max\|delta\| = \S+ \(tol 0\.001, every 7\)$",
                        p.stdout, flags=re.M)
    assert counts and all(int(n) == want for n in counts), (counts, want)
    # the reference's own lines still print -i
    assert "for 500 iterations." in p.stdout


def test_cap_reached_exits_5():
    prob = ob.problem(2, "fp32", "star", 1, "naive", 32, 32)
    assert oracle_count(prob, 1e-3, 7, 20) == (20, False)
    p = run(*BASE, "-i", "20", "--tol", "1e-3", "--check-every", "7", "-c")
    assert p.returncode == 5, p.stdout + p.stderr
    assert "The results of method CPU is correct." in p.stdout
    assert re.search(r"^\[stencil-amd\] CPU: not converged after 20 sweeps, ", p.stdout, flags=re.M)


def test_without_tol_nothing_changes():
    p = run(*BASE, "-i", "20", "-c")
    assert p.returncode == 0
    assert "converged" not in p.stdout
