"""The tiled bit-sliced MT-stream projection's cost (one MI355X) beside fks_project_mt_bs of the same
library on the same list and vectors in the same process.

The 291 tensors of the Llama-2-7B layout in bf16; nvec distinct bf16 vector buffers (one buffer
aliased nvec times would let the cache hide the vector traffic); K = 32 and 256, nvec = 1, 4, 8.

HIP events around each call on the current stream; warm-ups first, then codec.project_mt_bs_tiled and
codec.project_mt_bs ALTERNATED call by call, every call's time kept and min .. max reported.  The bar
(nvec = 8): the slowest tiled call below the fastest project_mt_bs call.  The largest distance
between the two results is reported as a share of the header's bound against the exact sum,
n 2^-52 sum|v z| <= n 2^-52 |v| |z| with |z|^2 ~ n (two such sums: twice it).

Prints one JSON line.  python tools/project_mt_bs_tiled_rate.py [--calls 5] [--warmup 1] [--k 32 256] [--nvec 1 4 8]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fate-llm_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from tools.gram_mt_rate import _event_ms, _layout  # noqa: E402


def _say(msg):
    print(f"[project_mt_bs_tiled_rate] {msg}", file=sys.stderr, flush=True)


def _case(specs, vecs, total, vnorm, seeds, calls, warmup):
    from fate_llm.algo.fedkseed import codec
    fns = {"tiled": lambda: codec.project_mt_bs_tiled(specs, seeds, vecs), "bs": lambda: codec.project_mt_bs(specs, seeds, vecs)}
    first = fns["tiled"]().cpu()
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms, last = {"tiled": [], "bs": []}, {}
    for i in range(calls):
        for name, fn in fns.items():
            t, last[name] = _event_ms(fn)
            ms[name].append(round(t, 3))
        _say(f"K = {len(seeds)}, nvec = {len(vecs)}: call {i + 1} of {calls}: tiled {ms['tiled'][-1]:.2f} ms, "
             f"project_mt_bs {ms['bs'][-1]:.2f} ms")
    got, ref = last["tiled"].cpu(), last["bs"].cpu()
    if not torch.equal(first.view(torch.int64), got.view(torch.int64)):
        raise SystemExit("project_mt_bs_tiled_rate: two calls over the same inputs gave different bits")
    share = float((got - ref).abs().max() / (2.0 * total * 2.0 ** -52 * vnorm * total ** 0.5))
    return {"seeds": len(seeds), "nvec": len(vecs), "tiled_ms": ms["tiled"], "bs_ms": ms["bs"],
            "tiled_ms_min_max": [min(ms["tiled"]), max(ms["tiled"])], "bs_ms_min_max": [min(ms["bs"]), max(ms["bs"])],
            "slowest_tiled_below_fastest_bs": max(ms["tiled"]) < min(ms["bs"]),
            "tiled_ms_per_seed_and_vector": round(min(ms["tiled"]) / (len(seeds) * len(vecs)), 4),
            "largest_share_of_the_bound_against_project_mt_bs": share}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--k", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--nvec", type=int, nargs="+", default=[1, 4, 8])
    args = ap.parse_args()
    from fate_llm.algo.fedkseed import _native
    dev = torch.device("cuda", 0)
    seeds = torch.randint(0, 2**32, (max(args.k),), generator=torch.Generator().manual_seed(1)).tolist()
    numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
    specs, store = _layout(numels, dev)
    out = {"what": "fks_project_mt_bs_tiled beside fks_project_mt_bs, torch_cpu stream, Llama-2-7B layout in bf16, "
                   "distinct bf16 vectors", "tensors": len(numels), "params": sum(numels), "calls": args.calls,
           "warmup": args.warmup, "build_id": _native.build_id(), "source_id": _native.source_id(), "cases": []}
    vecs, vnorm = [], 0.0
    for nvec in sorted(args.nvec):
        while len(vecs) < nvec:  # one buffer of its own per vector
            flat = torch.empty(sum(numels), dtype=torch.bfloat16, device=dev).normal_()
            vnorm = max(vnorm, float(flat.norm(dtype=torch.float32)))
            vecs.append(list(torch.split(flat, numels)))
        for k in args.k:
            out["cases"].append(_case(specs, vecs[:nvec], sum(numels), vnorm, seeds[:k], args.calls, args.warmup))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
