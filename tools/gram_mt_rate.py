"""The MT-stream Gram matrix's cost (one MI355X), beside fks_project_mt on the same list in the same
process.

Case (a): codec.gram_mt, symmetric, K = 19 and K = 64 seeds over the 291 tensors of the Llama-2-7B
layout in bf16.
Case (b): codec.gram_mt, symmetric, K = 256 over an adapter-sized bf16 layout of 4,194,304 elements
in 128 tensors.
The comparison is one fks_project_mt call of 19 seeds (one full pass) on the f32 concatenation of
the same list: its time per (vector, seed) against the Gram call's time per computed cell (the
cells of fks_gram_mt_passes, the few below the diagonal that a diagonal tile recomputes included).
What the arithmetic predicts: a cell needs (NR + NC) / (NR NC) generator evaluations where a
(vector, seed) of the projection needs one.

HIP events around each call on the current stream; warm-ups first, then the two sides ALTERNATED
call by call on the one box, medians of the timed calls.  One more Gram call runs under
codec.profile for the jump launches' share.  A library built with another tile (make
variant_gram_mt) is timed by FKS_LIB_OVERRIDE.  No threshold: the figures go to DESIGN.md.

Prints one JSON line.  python tools/gram_mt_rate.py [--calls 5] [--warmup 1] [--case a|b|both]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fate-llm_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

PROJ_SEEDS = 19  # one full fks_project_mt pass


def _say(msg):
    print(f"[gram_mt_rate] {msg}", file=sys.stderr, flush=True)


def _layout(numels, dev):
    """specs over one bf16 buffer cut into the layout's tensors (the parameters are never read)"""
    from fate_llm.algo.fedkseed import codec
    store = torch.empty(sum(numels), dtype=torch.bfloat16, device=dev)
    views, at = [], 0
    for n in numels:
        views.append(store[at:at + n])
        at += n
    return [codec.ParamSpec(v) for v in views], store


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _cells(k):
    """(passes, cells computed) of a symmetric call of k seeds"""
    from fate_llm.algo.fedkseed import _native
    L = _native.load()
    n = ctypes.c_int32(0)
    _native.check(L.fks_gram_mt_passes(k, k, 1, None, 0, ctypes.byref(n)))
    buf = (ctypes.c_int32 * max(1, 4 * n.value))()
    _native.check(L.fks_gram_mt_passes(k, k, 1, buf, n.value, ctypes.byref(n)))
    return n.value, sum(buf[4 * i + 1] * buf[4 * i + 3] for i in range(n.value))


def _workspace_bytes(specs, k):
    from fate_llm.algo.fedkseed import _native, codec
    b = codec._Batch(specs, "torch_cpu", stage=False)
    nbytes = ctypes.c_size_t(0)
    _native.check(_native.load().fks_gram_mt_workspace_size(ctypes.addressof(b.arr), b.n, k, k, ctypes.byref(nbytes)))
    return int(nbytes.value)


def _stats(ms, key):
    return {f"{key}_ms_median": round(statistics.median(ms), 3), f"{key}_ms_min": round(min(ms), 3),
            f"{key}_ms_max": round(max(ms), 3)}


def _case(specs, total, ks, seeds, vec, calls, warmup):
    """gram_mt at every k of ks alternated call by call with one 19-seed project_mt"""
    from fate_llm.algo.fedkseed import codec
    pseeds = seeds[:PROJ_SEEDS]

    def proj():
        return codec.project_mt(specs, pseeds, vec)

    out = {}
    for k in ks:
        s = seeds[:k]

        def gram():
            return codec.gram_mt(specs, s)

        first = gram().cpu()
        for _ in range(warmup):
            gram()
            proj()
        torch.cuda.synchronize()
        g_ms, p_ms = [], []
        for i in range(calls):
            t, last = _event_ms(gram)
            g_ms.append(t)
            p_ms.append(_event_ms(proj)[0])
            _say(f"K = {k}: call {i + 1} of {calls}: gram_mt {g_ms[-1]:.2f} ms, project_mt {p_ms[-1]:.2f} ms")
        last = last.cpu()
        if not torch.equal(first.view(torch.int64), last.view(torch.int64)):
            raise SystemExit("gram_mt_rate: two calls over the same inputs gave different bits")
        if not torch.equal(last.view(torch.int64), last.t().contiguous().view(torch.int64)):
            raise SystemExit("gram_mt_rate: the matrix is not exactly symmetric")
        with codec.profile() as pr:
            gram()
            torch.cuda.synchronize()
        passes, cells = _cells(k)
        gm, pm = statistics.median(g_ms), statistics.median(p_ms)
        out[f"k{k}"] = {"seeds": k, "passes": passes, "cells": cells, **_stats(g_ms, "gram_mt"),
                        **_stats(p_ms, "project_mt_19"),
                        "gram_mt_ms_per_cell": round(gm / cells, 4),
                        "project_mt_ms_per_vector_seed": round(pm / PROJ_SEEDS, 4),
                        "cell_over_vector_seed": round((gm / cells) / (pm / PROJ_SEEDS), 4),
                        "gram_mt_ns_per_param_cell": round(gm * 1e6 / total / cells, 6),
                        "jump_ms": round(pr.jump_ms, 3), "n_jump": pr.n_jump, "kernel_ms": round(pr.apply_ms, 3),
                        "n_kernel": pr.n_apply,
                        "jump_share_of_device_time": round(pr.jump_ms / max(pr.jump_ms + pr.apply_ms, 1e-9), 4),
                        "workspace_bytes": _workspace_bytes(specs, k),
                        "diag_over_n_min": float(last.diag().min()) / total,
                        "diag_over_n_max": float(last.diag().max()) / total}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=["a", "b", "both"], default="both")
    ap.add_argument("--seeds-a", type=int, nargs="+", default=[19, 64])
    ap.add_argument("--seeds-b", type=int, nargs="+", default=[256])
    args = ap.parse_args()
    from fate_llm.algo.fedkseed import _native, codec
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    NR, NC = codec.GRAM_MT_PASS_ROWS, codec.GRAM_MT_PASS_COLS
    out = {"what": "fks_gram_mt, torch_cpu stream, bf16", "calls": args.calls, "warmup": args.warmup,
           "tile": [NR, NC], "predicted_cell_over_vector_seed": round((NR + NC) / (NR * NC), 4),
           "lib": os.environ.get("FKS_LIB_OVERRIDE", "in tree"), "build_id": _native.build_id(),
           "source_id": _native.source_id()}
    seeds = torch.randint(0, 2**32, (max(args.seeds_a + args.seeds_b + [PROJ_SEEDS]),), generator=g).tolist()
    if args.case in ("a", "both"):
        numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
        total = sum(numels)
        specs, store = _layout(numels, dev)
        vec = torch.empty(total, dtype=torch.float32, device=dev).normal_()
        out["a"] = {"layout": "Llama-2-7B", "tensors": len(numels), "params": total,
                    **_case(specs, total, args.seeds_a, seeds, vec, args.calls, args.warmup)}
        del vec, specs, store
        torch.cuda.empty_cache()
    if args.case in ("b", "both"):
        # an adapter: 32 layers x 2 projections (q, v) x (A: 8 x 4096, B: 4096 x 8), rank 8 -- 4,194,304 elements
        numels = [8 * 4096] * (32 * 2 * 2)
        total = sum(numels)
        specs, store = _layout(numels, dev)
        vec = torch.empty(total, dtype=torch.float32, device=dev).normal_()
        out["b"] = {"layout": "adapter, rank 8 on the q and v projections (4096 x 4096) of 32 layers",
                    "tensors": len(numels), "params": total,
                    **_case(specs, total, args.seeds_b, seeds, vec, args.calls, args.warmup)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
