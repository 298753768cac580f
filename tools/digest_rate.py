"""The model fingerprint's cost on the 7B bf16 layout (one MI355X).

Times codec.model_digest (fks_digest: the FKSD-1 kernel, include/fks.h) over the 291
tensors of the Llama-2-7B layout, 13.5 GB -- larger than the 256 MB Infinity Cache, so every
call streams from HBM.  HIP events around each call on the current stream, warm-ups first,
then the median of --calls timed calls.  The digest is on by default in ClientTrainer, so
it is held against a budget: 1 % of the default-stream 7B reconstruct the README records
(17.47 s: 175 ms).  The read rate is reported beside the time, as bytes / time and as a
fraction of the HBM peak, with no threshold.

Prints one JSON line.  python tools/digest_rate.py [--calls 20] [--warmup 3]"""
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

RECONSTRUCT_7B_DEFAULT_STREAM_S = 17.47  # README: the default-stream (torch_rocm) 7B reconstruct
BUDGET_FRACTION = 0.01
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E, specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls must be at least 10 (the figure is a median)")
    from fate_llm.algo.fedkseed import _native, codec
    dev = torch.device("cuda", 0)
    params = [torch.empty(s, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02) for s in bench.llama7b_shapes()]
    nbytes = sum(p.numel() * p.element_size() for p in params)
    first = None
    for _ in range(args.warmup):
        first = codec.model_digest(params)
    torch.cuda.synchronize(dev)
    ms, last = [], None
    for _ in range(args.calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        last = codec.model_digest(params)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    if first is not None and codec.digest_bytes(first) != codec.digest_bytes(last):
        raise SystemExit("digest_rate: two calls over the same parameters gave different digests")
    med = statistics.median(ms)
    budget_ms = RECONSTRUCT_7B_DEFAULT_STREAM_S * 1e3 * BUDGET_FRACTION
    gbps = nbytes / (med * 1e-3) / 1e9
    out = {"what": "fks_digest, Llama-2-7B layout, bf16", "tensors": len(params),
           "params": sum(p.numel() for p in params), "bytes": nbytes, "calls": args.calls, "warmup": args.warmup,
           "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
           "read_GBps": round(gbps, 1), "fraction_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4),
           "hbm_peak_GBps": HBM_PEAK_GBPS, "budget_ms": round(budget_ms, 2),
           "fraction_of_budget": round(med / budget_ms, 4), "within_budget": med < budget_ms,
           "digest": codec.digest_bytes(last).hex(), "build_id": _native.build_id(), "source_id": _native.source_id()}
    print(json.dumps(out), flush=True)
    if not out["within_budget"]:
        raise SystemExit(f"digest_rate: {med:.2f} ms is over the {budget_ms:.1f} ms budget")


if __name__ == "__main__":
    main()
