"""bench.py's plain run, --full and --dump-outputs on one GPU, at a small buffer
(--params 2^18 + 37: 421 MT blocks, a ragged tail; K = 64, 63 non-zero seeds).

* A plain run prints the headline keys and none of the legs that take runs of their own;
  --full adds all four (alt_weight_decay, alt_stream, hd_inclusive, cpu_baseline).
* --dump-outputs writes the buffer as the last timed step left it: float32, every element
  at this size, bit for bit what the CPU oracle computes from the same seeded buffer over
  warmup + steps reconstructs -- and the same file with --full, whose legs run after it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fks_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, STEPS, WARMUP = (1 << 18) + 37, 64, 2, 1
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
LEGS = ("alt_weight_decay", "alt_stream", "hd_inclusive", "cpu_baseline")


def _bench(extra, out_dir):
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FKS_BENCH_SHARE_GPU"):
        env.pop(v, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--params", str(N), "--k", str(K), "--dump-outputs", str(out_dir)] + extra,
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0], np.load(os.path.join(out_dir, "params.npy"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return {"plain": _bench([], tmp_path_factory.mktemp("plain")),
            "full": _bench(["--full", "--cpu-budget", "2"], tmp_path_factory.mktemp("full"))}


def test_plain_run_has_the_headline_and_no_extra_leg(runs):
    out, _ = runs["plain"]
    assert all(k in out for k in HEADLINE) and not [k for k in LEGS if k in out]
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["params"] == N and out["dtype"] == "bf16" and out["higher_is_better"] is True
    # value is the buffer's bytes over one timed step (both rounded in the line)
    assert out["value"] == pytest.approx(N * 2 / (out["ms_per_step"] * 1e-3) / 1e9, rel=0.05)


def test_full_run_adds_every_leg(runs):
    out, _ = runs["full"]
    assert all(k in out for k in HEADLINE + LEGS)
    assert out["alt_weight_decay"]["weight_decay"] == 0.01 and out["alt_stream"]["stream"] == "torch_rocm"
    assert set(out["hd_inclusive"]) == {"torch_cpu", "torch_rocm"} and out["cpu_baseline"]["value"] > 0
    assert out["metric"] == runs["plain"][0]["metric"] and out["steps"] == STEPS


def test_dump_is_the_buffer_after_the_last_timed_step(runs):
    sys.path.insert(0, ROOT)
    import bench

    dev = torch.device("cuda", 0)
    flat = torch.empty(N, dtype=torch.bfloat16, device=dev)
    flat.normal_(0.0, 0.02, generator=torch.Generator(device=dev).manual_seed(0))  # bench.py's buffer
    ref = [flat.cpu().view(torch.int16).numpy().view(np.uint16).copy()]
    seeds, scalars = bench.synthetic_seeds(K)
    keep = [(s, g) for s, g in zip(seeds, scalars) if g != 0.0]
    for _ in range(WARMUP + STEPS):
        O.reconstruct(ref, [O.BF16], [1e-5], [0.0], [s for s, _ in keep], [g for _, g in keep])
    want = (ref[0].astype(np.uint32) << 16).view(np.float32)
    for name in ("plain", "full"):
        got = runs[name][1]
        assert got.dtype == np.float32 and got.shape == (N,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert not np.array_equal(want, flat.float().cpu().numpy())
