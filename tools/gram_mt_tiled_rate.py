"""The tiled MT-stream Gram matrix's cost (one MI355X) beside fks_gram_mt on the same list in the
same process.

Case (a): symmetric, K = 64 seeds over the 291 tensors of the Llama-2-7B layout in bf16.
Case (b): symmetric, K = 256 and K = 1024 over an adapter-sized bf16 layout of 4,194,304 elements in
128 tensors; fks_gram_mt runs once at K = 1024.

HIP events around each call on the current stream; warm-ups first, then codec.gram_mt_tiled and
codec.gram_mt ALTERNATED call by call, every call's time kept.  The bar (cases a and b at K = 256):
the slowest tiled call below the fastest gram_mt call.  One more tiled call runs under
codec.profile for the jump launches' share.  The largest distance between the two matrices is
reported as a share of the header's bound, 2 n 2^-52 sqrt(G_rr G_cc).

Prints one JSON line.  python tools/gram_mt_tiled_rate.py [--calls 5] [--warmup 1] [--case a|b|both]"""
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
    print(f"[gram_mt_tiled_rate] {msg}", file=sys.stderr, flush=True)


def _case(specs, total, k, seeds, calls, warmup, mt_calls):
    from fate_llm.algo.fedkseed import codec
    s = seeds[:k]

    def tiled():
        return codec.gram_mt_tiled(specs, s)

    def mt():
        return codec.gram_mt(specs, s)

    first = tiled().cpu()
    for _ in range(warmup):
        tiled()
        if mt_calls > 1:
            mt()
    torch.cuda.synchronize()
    t_ms, m_ms, ref = [], [], None
    for i in range(calls):
        t, last = _event_ms(tiled)
        t_ms.append(round(t, 3))
        if i < mt_calls:
            t, ref = _event_ms(mt)
            m_ms.append(round(t, 3))
        _say(f"K = {k}: call {i + 1} of {calls}: tiled {t_ms[-1]:.2f} ms, gram_mt {m_ms[-1]:.2f} ms")
    last, ref = last.cpu(), ref.cpu()
    if not torch.equal(first.view(torch.int64), last.view(torch.int64)):
        raise SystemExit("gram_mt_tiled_rate: two calls over the same inputs gave different bits")
    if not torch.equal(last.view(torch.int64), last.t().contiguous().view(torch.int64)):
        raise SystemExit("gram_mt_tiled_rate: the matrix is not exactly symmetric")
    d = ref.diag().sqrt()
    share = float(((last - ref).abs() / (2.0 * total * 2.0 ** -52 * torch.outer(d, d))).max())
    with codec.profile() as pr:
        tiled()
        torch.cuda.synchronize()
    return {"seeds": k, "tiled_ms": t_ms, "gram_mt_ms": m_ms, "slowest_tiled_below_fastest_gram_mt": max(t_ms) < min(m_ms),
            "speedup_of_medians": round(sorted(m_ms)[len(m_ms) // 2] / sorted(t_ms)[len(t_ms) // 2], 2),
            "jump_ms": round(pr.jump_ms, 3), "n_jump": pr.n_jump, "kernel_ms": round(pr.apply_ms, 3),
            "n_kernel": pr.n_apply,
            "jump_share_of_device_time": round(pr.jump_ms / max(pr.jump_ms + pr.apply_ms, 1e-9), 4),
            "largest_share_of_the_bound_against_gram_mt": share}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=["a", "b", "both"], default="both")
    args = ap.parse_args()
    from fate_llm.algo.fedkseed import _native
    dev = torch.device("cuda", 0)
    seeds = torch.randint(0, 2**32, (1024,), generator=torch.Generator().manual_seed(1)).tolist()
    out = {"what": "fks_gram_mt_tiled beside fks_gram_mt, torch_cpu stream, bf16", "calls": args.calls,
           "warmup": args.warmup, "build_id": _native.build_id(), "source_id": _native.source_id()}
    if args.case in ("a", "both"):
        numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
        specs, store = _layout(numels, dev)
        out["a"] = {"layout": "Llama-2-7B", "tensors": len(numels), "params": sum(numels),
                    "k64": _case(specs, sum(numels), 64, seeds, args.calls, args.warmup, args.calls)}
        del specs, store
        torch.cuda.empty_cache()
    if args.case in ("b", "both"):
        numels = [8 * 4096] * (32 * 2 * 2)  # tools/gram_mt_rate.py's adapter: 4,194,304 elements
        specs, store = _layout(numels, dev)
        out["b"] = {"layout": "adapter, rank 8 on the q and v projections (4096 x 4096) of 32 layers",
                    "tensors": len(numels), "params": sum(numels),
                    "k256": _case(specs, sum(numels), 256, seeds, args.calls, args.warmup, args.calls),
                    "k1024": _case(specs, sum(numels), 1024, seeds, args.calls, args.warmup, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
