"""Host time per cached call: back-to-back codec.perturb calls on one small bf16 tensor.

One bf16 tensor of 16,384 elements (27 MT blocks, fast path only) and one seed: after the
first call every call finds its plan, its windows and its z indices cached, so the device
work is tiny and the wall time is the host path of a call (the codec's Python, the C ABI,
plan lookup, cache hand-off, launches).  --calls calls are queued back to back and the
device is synchronised once at the end; the figure is the median of --reps repetitions.
FKS_LIB_OVERRIDE selects the library (A/B against another build).

Prints one JSON line.  python tools/host_call_rate.py [--calls 2000] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fate-llm_amd", "python"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from fate_llm.algo.fedkseed import _native, codec
    dev = torch.device("cuda", 0)
    p = (torch.randn(16384, generator=torch.Generator().manual_seed(0)) * 0.02).to(torch.bfloat16).to(dev)
    for _ in range(50):  # plan, window cache and z-index buffer in place
        codec.perturb([p], 11, 5e-4, stream_mode="torch_cpu")
    torch.cuda.synchronize()
    us = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            codec.perturb([p], 11, 5e-4, stream_mode="torch_cpu")
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / args.calls * 1e6)
    print(json.dumps({"metric": "host-bound cached codec.perturb, 16,384 bf16 elements", "unit": "us/call",
                      "calls": args.calls, "reps": [round(x, 2) for x in us], "median": round(statistics.median(us), 2),
                      "source_id": _native.source_id(), "build_id": _native.build_id()}))


if __name__ == "__main__":
    main()
