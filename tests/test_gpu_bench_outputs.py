"""bench.py's plain run, --full and --dump-outputs on the GPU: what the timed
path left after its last step, file for file against the oracle and from run
to run; what a plain run leaves out and --full keeps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 96^3 fp64 is 7 MB: written whole.  No warm-up sweeps: every stencil_iterate call starts from grid a, and which
# grid a warm-up call leaves its last sweep in depends on how its sweeps fuse, so only then is the timed call's
# input the seeded field itself (the settle leaves grid a unchanged)
N, STEPS, WARMUP = 96, 10, 0


def _bench(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--n", str(N), "--init", "random"] + argv,
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """One plain and one --full run of the same job, each with its dump."""
    plain_dir, full_dir = tmp_path_factory.mktemp("plain") / "out", tmp_path_factory.mktemp("full") / "out"
    plain = _bench(["--dump-outputs", str(plain_dir)])
    full = _bench(["--full", "--cpu-seconds", "0.2", "--dump-outputs", str(full_dir)])
    return plain, plain_dir, full, full_dir


def test_plain_line_keeps_the_headline_fields(runs):
    plain = runs[0]
    assert plain["steps"] == STEPS and plain["warmup"] == WARMUP
    assert plain["unit"] == "Gcell-updates/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["ms_per_step"] > 0
    # value is the timed steps' rate: the two are one measurement, each rounded (5 and 3 decimals)
    rel = 0.5e-5 / plain["ms_per_step"] + 0.5e-3 / plain["value"] + 1e-9
    assert plain["value"] == pytest.approx(N ** 3 / (plain["ms_per_step"] * 1e-3) / 1e9, rel=rel)
    assert plain["roofline"]["launches"] > 0 and plain["roofline"]["mean_launch_ms"] > 0


def test_plain_run_leaves_the_extra_runs_to_full(runs):
    plain, _, full, _ = runs
    assert plain["cpu_baseline"] is None and "cpu_baseline_all_cores" not in plain
    assert "copy_kernel_GBps" not in plain["roofline"]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline_all_cores"]["value"] > 0
    assert full["roofline"]["copy_kernel_GBps"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[key] == full[key]


def test_dump_is_the_grid_after_the_last_timed_step(runs):
    """The settle leaves grid a unchanged, so the final grid is STEPS sweeps
    of the seeded field: bitwise the oracle's."""
    _, plain_dir, _, _ = runs
    assert sorted(os.listdir(plain_dir)) == ["final_grid.npy", "plane_sums.npy"]
    got = np.load(plain_dir / "final_grid.npy")
    p = ob.problem(3, "fp64", "star", 1, "naive", N, N, N)
    want = np.ascontiguousarray(ob.interior(p, ob.run(p, STEPS, "random", 1)))
    assert got.dtype == np.float64 and got.shape == (N, N, N)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    sums = np.load(plain_dir / "plane_sums.npy")
    assert sums.dtype == np.float64 and sums.shape == (N,)
    # a device reduction in another order than numpy's: n = 96^2 non-negative fp64 terms, so either order is
    # within (n - 1) * 2^-53 = 1.0e-12 of the exact sum, relative
    assert np.allclose(sums, want.sum(axis=(1, 2)), rtol=2 * (N * N - 1) * 2.0 ** -53, atol=0)


def test_dump_is_the_same_from_run_to_run(runs):
    _, plain_dir, _, full_dir = runs
    for name in ("final_grid.npy", "plane_sums.npy"):
        a, b = np.load(plain_dir / name), np.load(full_dir / name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64)), name


def test_sampled_dump_of_a_grid_over_the_block_size(gpu, tmp_path):
    """A 168^3 fp64 grid (38 MB) is over the 32 MB block: whole x rows at the
    seeded (z, y), gathered on the device, bitwise the oracle's."""
    import bench
    from stencil_amd.engine import JacobiEngine, StencilSpec
    n, it = 168, 5
    eng = JacobiEngine(StencilSpec(dims=3, dtype="fp64"), n, n, n, device=gpu)
    eng.reset("random", 7)
    fin, _ = eng.iterate(it)
    bench.dump_grid(str(tmp_path), eng.interior(fin), eng.plane_sums(fin))
    assert sorted(os.listdir(tmp_path)) == ["final_grid_sample.npy", "final_grid_sample_y.npy",
                                            "final_grid_sample_z.npy", "plane_sums.npy"]
    zs = np.load(tmp_path / "final_grid_sample_z.npy").astype(np.int64)
    ys = np.load(tmp_path / "final_grid_sample_y.npy").astype(np.int64)
    got = np.load(tmp_path / "final_grid_sample.npy")
    assert len(zs) == bench.DUMP_PLANES and {0, n - 1} <= set(zs) and got.shape == (len(zs), len(ys), n)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20
    p = ob.problem(3, "fp64", "star", 1, "naive", n, n, n)
    want = ob.interior(p, ob.run(p, it, "random", 7))[zs[:, None], ys[None, :]]
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
