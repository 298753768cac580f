"""The bit-sliced MT-stream projection's cost (one MI355X) beside fks_project_mt_multi of the same
library on the same list and vector in the same process.

Case (a): the 291 tensors of the Llama-2-7B layout in bf16, one bf16 vector, K = 19, 32, 64, 256.
Case (b): an adapter-sized bf16 layout of 4,194,304 elements in 128 tensors, K = 256.

HIP events around each call on the current stream; warm-ups first, then codec.project_mt_bs and
codec.project_mt_multi ALTERNATED call by call, every call's time kept; the medians go to ms per
seed.  One more call of each runs under codec.profile for the jump launches' share of its device
time.  The largest distance between the two results is reported as a share of the header's bound
against the exact sum, n 2^-52 sum|v z| <= n 2^-52 |v| |z| with |z|^2 ~ n (two such sums: twice it).

Prints one JSON line.  python tools/project_mt_bs_rate.py [--calls 3] [--warmup 1] [--case a|b|both]"""
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
    print(f"[project_mt_bs_rate] {msg}", file=sys.stderr, flush=True)


def _case(specs, vec, total, vnorm, k, seeds, calls, warmup):
    from fate_llm.algo.fedkseed import codec
    s = seeds[:k]
    fns = {"bs": lambda: codec.project_mt_bs(specs, s, [vec]), "multi": lambda: codec.project_mt_multi(specs, s, [vec])}
    first = fns["bs"]().cpu()
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms, last = {"bs": [], "multi": []}, {}
    for i in range(calls):
        for name, fn in fns.items():
            t, last[name] = _event_ms(fn)
            ms[name].append(round(t, 3))
        _say(f"K = {k}: call {i + 1} of {calls}: bs {ms['bs'][-1]:.2f} ms, project_mt_multi {ms['multi'][-1]:.2f} ms")
    got, ref = last["bs"].cpu(), last["multi"].cpu()
    if not torch.equal(first.view(torch.int64), got.view(torch.int64)):
        raise SystemExit("project_mt_bs_rate: two calls over the same inputs gave different bits")
    share = float((got - ref).abs().max() / (2.0 * total * 2.0 ** -52 * vnorm * total ** 0.5))
    out = {"seeds": k, "bs_ms": ms["bs"], "multi_ms": ms["multi"],
           "bs_ms_per_seed": round(statistics.median(ms["bs"]) / k, 4),
           "multi_ms_per_seed": round(statistics.median(ms["multi"]) / k, 4),
           "bs_over_multi": round(statistics.median(ms["bs"]) / statistics.median(ms["multi"]), 4),
           "largest_share_of_the_bound_against_project_mt_multi": share}
    for name, fn in fns.items():
        with codec.profile() as pr:
            fn()
            torch.cuda.synchronize()
        out[name + "_jump_share_of_device_time"] = round(pr.jump_ms / max(pr.jump_ms + pr.apply_ms, 1e-9), 4)
        out[name + "_launches"] = [pr.n_jump, pr.n_apply]
    return out


def _run(numels, ks, seeds, dev, calls, warmup):
    specs, store = _layout(numels, dev)
    flat = torch.empty(sum(numels), dtype=torch.bfloat16, device=dev).normal_()
    vec, at = [], 0
    for n in numels:
        vec.append(flat[at:at + n])
        at += n
    vnorm = float(flat.float().norm())
    return {"tensors": len(numels), "params": sum(numels),
            **{f"k{k}": _case(specs, vec, sum(numels), vnorm, k, seeds, calls, warmup) for k in ks}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=["a", "b", "both"], default="both")
    args = ap.parse_args()
    from fate_llm.algo.fedkseed import _native
    dev = torch.device("cuda", 0)
    seeds = torch.randint(0, 2**32, (256,), generator=torch.Generator().manual_seed(1)).tolist()
    out = {"what": "fks_project_mt_bs beside fks_project_mt_multi, torch_cpu stream, bf16, one bf16 vector",
           "calls": args.calls, "warmup": args.warmup, "build_id": _native.build_id(), "source_id": _native.source_id()}
    if args.case in ("a", "both"):
        numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
        out["a"] = dict(layout="Llama-2-7B", **_run(numels, [19, 32, 64, 256], seeds, dev, args.calls, args.warmup))
        torch.cuda.empty_cache()
    if args.case in ("b", "both"):
        numels = [8 * 4096] * (32 * 2 * 2)  # tools/gram_mt_rate.py's adapter: 4,194,304 elements
        out["b"] = dict(layout="adapter, rank 8 on the q and v projections (4096 x 4096) of 32 layers",
                        **_run(numels, [256], seeds, dev, args.calls, args.warmup))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
