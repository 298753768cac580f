"""The seed-basis Gram matrix's cost (one MI355X), beside the projection pass it replaces.

Case (a): codec.gram of K = 32 seeds, symmetric, over the 291 tensors of the Llama-2-7B layout in
bf16 -- eight passes of four row seeds against 32, 28, ..., 4 column seeds --, and in the same
process one codec.project_multi call of four bf16 vectors and 32 seeds over the same layout: the
pass a Gram launch stands in for (fks_normal into buffers of the model's size, then the projection
over them), with the vectors loaded where the Gram pass draws them.
Case (b): codec.gram of K = 4096 seeds, symmetric, over an adapter-sized bf16 layout of 4,194,304
elements in 128 tensors: 66,048 passes, half a minute per call (--small-seeds, --small-calls and
--small-warmup change the case; progress goes to stderr).
HIP events around each call on the current stream, warm-ups first, then the median of the timed
calls.  Also states the memory the call needs above the model (its workspace) against the K
buffers of the model's size of the fks_normal route.  No threshold: the figures go to DESIGN.md.

Prints one JSON line.  python tools/gram_rate.py [--calls 20] [--warmup 3] [--case a|b|both]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fate-llm_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from project_rate import _timed  # noqa: E402

SEEDS = 32  # one column batch (kPhxSeeds), eight row tiles


def _say(msg):
    """progress on stderr (the JSON line is the only thing on stdout): a K = 4096 case takes minutes"""
    print(f"[gram_rate] {msg}", file=sys.stderr, flush=True)


def _layout(numels, dev):
    """specs over one bf16 buffer cut into the layout's tensors (the parameters are never read)"""
    from fate_llm.algo.fedkseed import codec
    store = torch.empty(sum(numels), dtype=torch.bfloat16, device=dev)
    views, at = [], 0
    for n in numels:
        views.append(store[at:at + n])
        at += n
    return [codec.ParamSpec(v) for v in views], store


def _workspace_bytes(specs, k):
    from fate_llm.algo.fedkseed import _native, codec
    b = codec._Batch(specs, "torch_rocm", stage=False)
    nbytes = ctypes.c_size_t(0)
    _native.check(_native.load().fks_gram_workspace_size(ctypes.addressof(b.arr), b.n, k, k, ctypes.byref(nbytes)))
    return int(nbytes.value)


def _stats(ms, key):
    return {f"{key}_ms_median": round(statistics.median(ms), 3), f"{key}_ms_min": round(min(ms), 3),
            f"{key}_ms_max": round(max(ms), 3)}


def _gram_case(specs, seeds, calls, warmup):
    from fate_llm.algo.fedkseed import codec
    t0 = time.perf_counter()
    first = codec.gram(specs, seeds, stream_mode="torch_rocm").cpu()
    _say(f"gram K = {len(seeds)}: first call (plan upload included) {time.perf_counter() - t0:.3f} s; "
         f"{warmup} warm-ups and {calls} timed calls follow")
    slow = time.perf_counter() - t0 > 5.0  # then every call reports: minutes must not pass in silence

    def call():
        out = codec.gram(specs, seeds, stream_mode="torch_rocm")
        if slow:
            torch.cuda.synchronize()
            _say(f"gram K = {len(seeds)}: a call done at {time.perf_counter() - t0:.1f} s")
        return out

    ms, last = _timed(call, calls, warmup)
    _say(f"gram K = {len(seeds)}: median {statistics.median(ms):.3f} ms")
    last = last.cpu()
    if not torch.equal(first.view(torch.int64), last.view(torch.int64)):
        raise SystemExit("gram_rate: two calls over the same inputs gave different bits")
    if not torch.equal(last.view(torch.int64), last.t().contiguous().view(torch.int64)):
        raise SystemExit("gram_rate: the matrix is not exactly symmetric")
    return ms, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["a", "b", "both"], default="both")
    ap.add_argument("--small-seeds", type=int, default=4096)
    ap.add_argument("--small-calls", type=int, default=None, help="timed calls of case (b); default --calls")
    ap.add_argument("--small-warmup", type=int, default=None, help="warm-ups of case (b); default --warmup")
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls must be at least 10 (the figure is a median)")
    from fate_llm.algo.fedkseed import _native, codec
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    out = {"what": "fks_gram, torch_rocm stream, bf16", "calls": args.calls, "warmup": args.warmup,
           "pass_rows": codec.GRAM_PASS_ROWS, "build_id": _native.build_id(), "source_id": _native.source_id()}
    if args.case in ("a", "both"):
        numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
        total = sum(numels)
        specs, store = _layout(numels, dev)
        seeds = torch.randint(0, 2**32, (SEEDS,), generator=g).tolist()
        ms, G = _gram_case(specs, seeds, args.calls, args.warmup)
        # the pass a Gram launch replaces: four bf16 vectors of the model's size, 32 seeds
        vecs = [torch.empty(total, dtype=torch.bfloat16, device=dev).normal_() for _ in range(4)]
        vlists, at = [[] for _ in vecs], 0
        for n in numels:
            for m, v in enumerate(vecs):
                vlists[m].append(v[at:at + n])
            at += n
        p_ms, _ = _timed(lambda: codec.project_multi(specs, seeds, vlists, stream_mode="torch_rocm"),
                         args.calls, args.warmup)
        gm, pm = statistics.median(ms), statistics.median(p_ms)
        ws = _workspace_bytes(specs, SEEDS)
        pairs = SEEDS * (SEEDS + 1) // 2
        out["a"] = {"layout": "Llama-2-7B", "tensors": len(numels), "params": total, "seeds": SEEDS, "passes": 8,
                    **_stats(ms, "gram"), **_stats(p_ms, "project_multi_4x32"),
                    "gram_over_project_multi_4x32": round(gm / pm, 4),
                    "gram_ns_per_param_pair": round(gm * 1e6 / total / pairs, 6),
                    "project_multi_ns_per_param_vector_seed": round(pm * 1e6 / total / (4 * SEEDS), 6),
                    "workspace_bytes": ws, "normal_route_bytes": SEEDS * total * 2,
                    "diag_over_n_min": float(G.diag().min()) / total, "diag_over_n_max": float(G.diag().max()) / total}
        del vecs, vlists, specs, store
    if args.case in ("b", "both"):
        # an adapter: 32 layers x 2 projections (q, v) x (A: 8 x 4096, B: 4096 x 8), rank 8 -- 4,194,304 elements
        numels = [8 * 4096] * (32 * 2 * 2)
        total = sum(numels)
        specs, store = _layout(numels, dev)
        k = args.small_seeds
        seeds = torch.randint(0, 2**32, (k,), generator=g).tolist()
        calls = args.small_calls or args.calls
        warm = args.warmup if args.small_warmup is None else args.small_warmup
        ms, G = _gram_case(specs, seeds, calls, warm)
        gm = statistics.median(ms)
        n = ctypes.c_int32(0)
        _native.check(_native.load().fks_gram_passes(k, k, 1, None, 0, ctypes.byref(n)))
        off = G - torch.diag(G.diag())
        out["b"] = {"layout": "adapter, rank 8 on the q and v projections (4096 x 4096) of 32 layers",
                    "tensors": len(numels), "params": total, "seeds": k, "passes": n.value, "calls": calls,
                    "warmup": warm, **_stats(ms, "gram"),
                    "gram_ns_per_param_pair": round(gm * 1e6 / total / (k * (k + 1) // 2), 6),
                    "gram_us_per_pass": round(gm * 1e3 / max(n.value, 1), 3),
                    "workspace_bytes": _workspace_bytes(specs, k), "normal_route_bytes": k * total * 2,
                    "diag_over_n_min": float(G.diag().min()) / total, "diag_over_n_max": float(G.diag().max()) / total,
                    "offdiag_rms_over_sqrt_n": float(off.pow(2).sum().div(k * (k - 1)).sqrt()) / total ** 0.5}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
