"""bench.py's multi-rank path on CPU (no GPU): `--gpus N` re-launches itself under
torch.distributed.run with N ranks, the ranks time a dummy step with the barrier +
max-over-ranks protocol over gloo (`--selftest`), and rank 0 alone prints one JSON line
reporting the world size the process group saw.  Also the CPU-baseline leg on a tiny
budget (the reference's CPU path through oracle/torch_replica.py), and --dump-outputs:
rank 0's float32 file after the last timed step, the same in every run, at fixed positions."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=180):
    e = dict(os.environ, MASTER_ADDR="127.0.0.1")
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout, env=e, cwd=ROOT)


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_flag_launches_n_ranks(n):
    r = _run(["--gpus", str(n), "--selftest", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout  # rank 0 only
    assert lines[0]["n_gpus"] == n and lines[0]["steps"] == 3 and lines[0]["selftest"]


def test_world_size_mismatch_fails_loudly():
    r = _run(["--gpus", "2", "--selftest"], env={"WORLD_SIZE": "1"})
    assert r.returncode != 0
    assert "WORLD_SIZE" in r.stderr


def test_dump_outputs_writes_float32_and_repeats(tmp_path):
    import numpy as np
    got = []
    for d in ("a", "b"):
        r = _run(["--gpus", "2", "--selftest", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        line, = _json_lines(r.stdout)
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert os.listdir(tmp_path / d) == ["selftest.npy"]  # rank 0 only
        got.append(np.load(tmp_path / d / "selftest.npy"))
    assert got[0].dtype == np.float32 and got[0].shape == (1 << 16,)
    want = np.float32(1.0)
    for _ in range(1 + 3):  # warmup + steps of the dummy step
        want = np.float32(want * np.float32(1.0000001))
    assert np.array_equal(got[0], np.full(1 << 16, want, np.float32))
    assert np.array_equal(got[0], got[1])


def test_dump_positions_fixed_sorted_and_bounded():
    sys.path.insert(0, ROOT)
    import bench

    small = bench.dump_positions(5, 1000, [0, 400])
    assert small.tolist() == list(range(5, 1000))  # a small range whole
    lo, hi = 7, 7 + 16 * bench.DUMP_MAX_ELEMS
    bounds = [0, lo, 10 ** 7, hi, 10 ** 9]
    p = bench.dump_positions(lo, hi, bounds)
    # M draws from 16 M positions: about M / 32 of them repeat an earlier one
    assert p.dtype == torch.int64 and 0.95 * bench.DUMP_MAX_ELEMS < p.numel() <= bench.DUMP_MAX_ELEMS
    assert int(p[0]) == lo and int(p[-1]) == hi - 1 and bool((p[1:] > p[:-1]).all())
    near = set(range(10 ** 7 - 32, 10 ** 7 + 32))
    assert near <= set(p[(p >= 10 ** 7 - 32) & (p < 10 ** 7 + 32)].tolist())
    assert p.equal(bench.dump_positions(lo, hi, bounds))  # the same positions in every run


@pytest.mark.parametrize("wd", [0.0, None])
def test_cpu_baseline_leg_runs(wd):
    sys.path.insert(0, ROOT)
    import bench

    cb = bench.cpu_baseline(3.0, wd)
    assert cb["kind"] == "port" and cb["unit"] == "GB/s" and cb["value"] > 0
    # one single-thread process per CPU this job may use; the host's count beside it
    assert cb["cores"] == bench.usable_cpus()[0] and cb["nproc"] == os.cpu_count()
    assert ("all_host_cores_extrapolated" in cb) == (cb["cores"] < cb["nproc"])
    sp = cb["single_process"]
    # linear in N: the per-(seed*param) cost at 2^22 and 2^24 params agrees within 2x
    assert 0.5 < sp["ns_per_seed_param_2^22"] / sp["ns_per_seed_param_2^24"] < 2.0
