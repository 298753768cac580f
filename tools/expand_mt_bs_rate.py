"""The bit-sliced MT-stream expansion's cost (one MI355X) beside fks_expand_mt_multi of the same
library on the same list and output in the same process.

Case (a): the 291 tensors of the Llama-2-7B layout in bf16, one bf16 output, beta 0, K = 19, 32, 64, 256.
Case (b): an adapter-sized bf16 layout of 4,194,304 elements in 128 tensors, K = 256.

HIP events around each call on the current stream; warm-ups first, then codec.expand_mt_bs and
codec.expand_mt_multi ALTERNATED call by call, every call's time kept; the medians go to ms per
seed, and the spread (largest - smallest) of either call's times is reported beside their
difference.  The two outputs must hold the same bits.  For information: codec.delta_accumulate into
an f32 buffer at the same K, and one more call of each under codec.profile for the jump launches'
share of its device time.

Prints one JSON line.  python tools/expand_mt_bs_rate.py [--calls 5] [--warmup 1] [--case a|b|both] [--ks 19,32,64,256]"""
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
from tools.gram_mt_rate import _event_ms, _layout  # noqa: E402


def _say(msg):
    print(f"[expand_mt_bs_rate] {msg}", file=sys.stderr, flush=True)


def _case(specs, outs, delta, k, seeds, calls, warmup):
    from fate_llm.algo.fedkseed import codec
    s = seeds[:k]
    coefs = torch.randn(k, dtype=torch.float64, generator=torch.Generator().manual_seed(k)).tolist()
    fns = {"bs": lambda: codec.expand_mt_bs(specs, s, coefs, [outs["bs"]]),
           "multi": lambda: codec.expand_mt_multi(specs, s, coefs, [outs["multi"]]),
           "delta": lambda: codec.delta_accumulate(specs, s, coefs, delta, stream_mode="torch_cpu")}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for i in range(calls):
        for name, fn in fns.items():
            ms[name].append(round(_event_ms(fn)[0], 3))
        _say(f"K = {k}: call {i + 1} of {calls}: bs {ms['bs'][-1]:.2f} ms, expand_mt_multi {ms['multi'][-1]:.2f} ms, "
             f"delta_accumulate {ms['delta'][-1]:.2f} ms")
    for a, b in zip(outs["bs"], outs["multi"]):
        if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
            raise SystemExit("expand_mt_bs_rate: expand_mt_bs and expand_mt_multi gave different bits")
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"seeds": k, "bs_ms": ms["bs"], "multi_ms": ms["multi"], "delta_accumulate_ms": ms["delta"],
           "bs_ms_per_seed": round(med["bs"] / k, 4), "multi_ms_per_seed": round(med["multi"] / k, 4),
           "bs_over_multi": round(med["bs"] / med["multi"], 4), "bs_over_delta_accumulate": round(med["bs"] / med["delta"], 4),
           "multi_minus_bs_ms": round(med["multi"] - med["bs"], 3),
           "spread_ms": {name: round(max(ms[name]) - min(ms[name]), 3) for name in ("bs", "multi")}}
    for name in ("bs", "multi"):
        with codec.profile() as pr:
            fns[name]()
            torch.cuda.synchronize()
        out[name + "_jump_share_of_device_time"] = round(pr.jump_ms / max(pr.jump_ms + pr.apply_ms, 1e-9), 4)
        out[name + "_launches"] = [pr.n_jump, pr.n_apply]
    return out


def _run(numels, ks, seeds, dev, calls, warmup):
    specs, store = _layout(numels, dev)
    outs = {}
    for name in ("bs", "multi"):
        flat = torch.empty(sum(numels), dtype=torch.bfloat16, device=dev)
        outs[name] = list(flat.split(numels))
    delta = torch.zeros(sum(numels), dtype=torch.float32, device=dev)
    return {"tensors": len(numels), "params": sum(numels),
            **{f"k{k}": _case(specs, outs, delta, k, seeds, calls, warmup) for k in ks}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=["a", "b", "both"], default="both")
    ap.add_argument("--ks", default="19,32,64,256")
    args = ap.parse_args()
    from fate_llm.algo.fedkseed import _native
    dev = torch.device("cuda", 0)
    seeds = torch.randint(0, 2**32, (256,), generator=torch.Generator().manual_seed(1)).tolist()
    out = {"what": "fks_expand_mt_bs beside fks_expand_mt_multi, torch_cpu stream, bf16, one bf16 output, beta 0",
           "calls": args.calls, "warmup": args.warmup, "build_id": _native.build_id(), "source_id": _native.source_id()}
    if args.case in ("a", "both"):
        numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
        ks = [int(k) for k in args.ks.split(",")]
        out["a"] = dict(layout="Llama-2-7B", **_run(numels, ks, seeds, dev, args.calls, args.warmup))
        torch.cuda.empty_cache()
    if args.case in ("b", "both"):
        numels = [8 * 4096] * (32 * 2 * 2)  # tools/gram_mt_rate.py's adapter: 4,194,304 elements
        out["b"] = dict(layout="adapter, rank 8 on the q and v projections (4096 x 4096) of 32 layers",
                        **_run(numels, [256], seeds, dev, args.calls, args.warmup))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
