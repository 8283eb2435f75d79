"""`python bench.py --gpus N` must really start N ranks (round-1 finding: the flag was parsed and ignored).
Checked here without a GPU: TC_BENCH_LAUNCH_TEST makes every rank stop after the rendezvous and the 3-float
all-reduce (gloo), so this exercises exactly the launcher, the WORLD_SIZE cross-check and the one-line
output contract."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        if k not in env_extra:
            env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=300)


def test_gpus_flag_spawns_that_many_ranks():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"TC_BENCH_LAUNCH_TEST": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["weight"] == 2 * 38400.0


def test_mismatch_between_flag_and_launcher_fails_loudly():
    r = _run(["--gpus", "4"], {"TC_BENCH_LAUNCH_TEST": "1", "WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_steps_below_one_are_refused():
    r = _run(["--steps", "0"], {})
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_dump_outputs_of_the_timed_path(tmp_path):
    """--dump-outputs DIR: the last timed step's outputs as float32 / float64 .npy files under 64 MB, the same on a
    second run with the same arguments; --steps is the number of timed steps and the line carries ms_per_step."""
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        r = _run(["--config", "C1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-extras",
                  "--dump-outputs", str(d)], {})
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        files = sorted(os.listdir(str(d)))
        assert files == sorted(n + ".npy" for n in out["dump_outputs"]["arrays"])
        assert sum(os.path.getsize(str(d / f)) for f in files) <= 64 * 10 ** 6
        arrays = {f[:-4]: np.load(str(d / f)) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        dumps.append(arrays)
    a, b = dumps
    S, T, P = 16, 50, 200  # C1: every row is in the sample
    assert a["deriv_sample"].shape == (S * T, P) and np.array_equal(a["deriv_sample_rows"], np.arange(S * T))
    np.testing.assert_allclose(a["deriv_row_sums"], a["deriv_sample"].astype(np.float64).sum(axis=1), rtol=1e-5, atol=1e-5)
    assert a["status"][0] == 0 and np.isfinite(a["den_logprob"][0]) and np.abs(a["deriv_sample"]).max() > 0
    assert sorted(a) == sorted(b)
    for name in a:
        np.testing.assert_allclose(a[name], b[name], rtol=1e-6, atol=0, err_msg=name)
