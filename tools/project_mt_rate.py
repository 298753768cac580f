"""The MT19937-stream projection's cost beside its adjoint (one MI355X).

Per layout -- the 291 bf16 tensors of Llama-2-7B, one fp32 tensor of 2^28 elements, and one f16
tensor of 2^26 elements -- and in one process, one 19-seed pass each of
  codec.project_mt                      (fks_project_mt: jumps, fks_project_mt_kernel, reduce)
  codec.delta_accumulate on torch_cpu   (fks_delta_accumulate: jumps, fks_apply_kernel kModeDelta)
the like-for-like 19-seed kernels on the same plan: the projection reads the 4-byte vector
element and writes nothing, the delta reads and writes 4 bytes.  Every f16 run is irregular, so
the third layout times fks_project_mt_irr_kernel and fks_irregular_kernel<kModeDelta>.  For scale, one 32-seed
codec.project launch on the torch_rocm stream over the same layout, as ms per seed.
HIP events around each call on the current stream, warm-ups first, then the median of --calls
timed calls with their minimum and maximum (the run-to-run spread).  No threshold: the figures
go to DESIGN.md.

Prints one JSON line per layout.  python tools/project_mt_rate.py [--calls 20] [--warmup 3] [--layout all|7b|f32|f16]"""
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
from project_rate import _timed  # noqa: E402

MT_SEEDS = 19    # one pass (kMaxSeedsPerPass)
PHX_SEEDS = 32   # one pass (kPhxSeeds)


def _stats(ms, seeds):
    med = statistics.median(ms)
    return {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "ms_per_seed": round(med / seeds, 4)}


def _layout(name, numels, dtype, dev, calls, warmup):
    from fate_llm.algo.fedkseed import _native, codec
    total = sum(numels)
    # the parameters are never read by any of the calls (their addresses key the plans): one
    # buffer cut into the layout's tensors
    store = torch.empty(total, dtype=dtype, device=dev)
    views, at = [], 0
    for n in numels:
        views.append(store[at:at + n])
        at += n
    specs = [codec.ParamSpec(v) for v in views]
    vec = torch.empty(total, dtype=torch.float32, device=dev).normal_()
    g = torch.Generator().manual_seed(1)
    seeds = torch.randint(0, 2**32, (PHX_SEEDS,), generator=g).tolist()
    coefs = torch.randn(PHX_SEEDS, generator=g, dtype=torch.float64).tolist()

    first = codec.project_mt(specs, seeds[:MT_SEEDS], vec).cpu()
    p_ms, last = _timed(lambda: codec.project_mt(specs, seeds[:MT_SEEDS], vec), calls, warmup)
    if not torch.equal(first.view(torch.int64), last.cpu().view(torch.int64)):
        raise SystemExit("project_mt_rate: two calls over the same inputs gave different bits")
    r_ms, _ = _timed(lambda: codec.project(specs, seeds, vec, stream_mode="torch_rocm"), calls, warmup)
    # the delta launch accumulates into the same buffer (its values are not looked at): last
    d_ms, _ = _timed(lambda: codec.delta_accumulate(specs, seeds[:MT_SEEDS], coefs[:MT_SEEDS], vec,
                                                    stream_mode="torch_cpu"), calls, warmup)
    p, d, r = _stats(p_ms, MT_SEEDS), _stats(d_ms, MT_SEEDS), _stats(r_ms, PHX_SEEDS)
    out = {"what": f"fks_project_mt vs fks_delta_accumulate (torch_cpu, {MT_SEEDS} seeds) and fks_project "
                   f"(torch_rocm, {PHX_SEEDS} seeds), {name}",
           "tensors": len(views), "params": total, "calls": calls, "warmup": warmup,
           "project_mt": p, "delta_mt": d, "project_rocm": r,
           "project_mt_over_delta_mt": round(p["ms_median"] / d["ms_median"], 4),
           "project_mt_over_project_rocm_per_seed": round(p["ms_per_seed"] / r["ms_per_seed"], 4),
           "project_mt_ns_per_param_seed": round(p["ms_median"] * 1e6 / total / MT_SEEDS, 5),
           "delta_mt_ns_per_param_seed": round(d["ms_median"] * 1e6 / total / MT_SEEDS, 5),
           "cpu_fp32_flavour": codec.cpu_fp32_flavour(), "projection_seed0": float(last[0]),
           "build_id": _native.build_id(), "source_id": _native.source_id()}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layout", choices=("all", "7b", "f32", "f16"), default="all")
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls must be at least 10 (the figure is a median)")
    dev = torch.device("cuda", 0)
    if args.layout in ("all", "7b"):
        numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
        _layout("Llama-2-7B layout, bf16", numels, torch.bfloat16, dev, args.calls, args.warmup)
        torch.cuda.empty_cache()
    if args.layout in ("all", "f32"):
        _layout("one fp32 tensor of 2^28 elements", [1 << 28], torch.float32, dev, args.calls, args.warmup)
        torch.cuda.empty_cache()
    if args.layout in ("all", "f16"):
        _layout("one f16 tensor of 2^26 elements (irregular kernels)", [1 << 26], torch.float16, dev, args.calls,
                args.warmup)


if __name__ == "__main__":
    main()
