"""The seed-basis projection's cost on the 7B bf16 layout (one MI355X), beside its adjoint.

Times one 32-seed codec.project launch (fks_project: fks_project_kernel and its reduce, one
pass) over the 291 tensors of the Llama-2-7B layout, and in the same process one 32-seed
codec.delta_accumulate launch on the torch_rocm stream over the same layout -- the same
generator; the projection reads the 4-byte vector element and writes nothing, the delta
reads and writes 4 bytes.  HIP events around each call on the current stream, warm-ups
first, then the median of --calls timed calls.  No threshold: the figures go to DESIGN.md.

Prints one JSON line.  python tools/project_rate.py [--calls 20] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fate-llm_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

SEEDS = 32  # one pass (kPhxSeeds)


def _timed(fn, calls, warmup):
    last = None
    for _ in range(warmup):
        last = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        last = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls must be at least 10 (the figure is a median)")
    from fate_llm.algo.fedkseed import _native, codec
    dev = torch.device("cuda", 0)
    # the parameters are never read by either call (their addresses key the plan): one
    # buffer cut into the layout's tensors
    shapes = bench.llama7b_shapes()
    numels = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numels)
    store = torch.empty(total, dtype=torch.bfloat16, device=dev)
    views, at = [], 0
    for n in numels:
        views.append(store[at:at + n])
        at += n
    specs = [codec.ParamSpec(v) for v in views]
    vec = torch.empty(total, dtype=torch.float32, device=dev).normal_()
    g = torch.Generator().manual_seed(1)
    seeds = torch.randint(0, 2**32, (SEEDS,), generator=g).tolist()
    coefs = torch.randn(SEEDS, generator=g, dtype=torch.float64).tolist()

    first = codec.project(specs, seeds, vec, stream_mode="torch_rocm").cpu()
    p_ms, last = _timed(lambda: codec.project(specs, seeds, vec, stream_mode="torch_rocm"), args.calls, args.warmup)
    if not torch.equal(first.view(torch.int64), last.cpu().view(torch.int64)):
        raise SystemExit("project_rate: two calls over the same inputs gave different bits")
    # the delta launch accumulates into the same buffer (its values are not looked at)
    d_ms, _ = _timed(lambda: codec.delta_accumulate(specs, seeds, coefs, vec, stream_mode="torch_rocm"),
                     args.calls, args.warmup)
    pm, dm = statistics.median(p_ms), statistics.median(d_ms)
    out = {"what": "fks_project vs fks_delta_accumulate, torch_rocm stream, Llama-2-7B layout, bf16, 32 seeds",
           "tensors": len(views), "params": total, "seeds": SEEDS, "calls": args.calls, "warmup": args.warmup,
           "project_ms_median": round(pm, 3), "project_ms_min": round(min(p_ms), 3), "project_ms_max": round(max(p_ms), 3),
           "delta_ms_median": round(dm, 3), "delta_ms_min": round(min(d_ms), 3), "delta_ms_max": round(max(d_ms), 3),
           "project_over_delta": round(pm / dm, 4),
           "project_ns_per_param_seed": round(pm * 1e6 / total / SEEDS, 5),
           "delta_ns_per_param_seed": round(dm * 1e6 / total / SEEDS, 5),
           "projection_seed0": float(last[0]), "build_id": _native.build_id(), "source_id": _native.source_id()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
