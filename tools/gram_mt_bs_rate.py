"""The bit-sliced MT-stream Gram matrix's cost (one MI355X) beside fks_gram_mt_tiled on the same
list in the same process.

Case (a): symmetric, K = 32, 64 and 256 seeds over the 291 tensors of the Llama-2-7B layout in bf16.
Case (b): symmetric, K = 256 and K = 1024 over an adapter-sized bf16 layout of 4,194,304 elements in
128 tensors.

HIP events around each call on the current stream; warm-ups first, then codec.gram_mt_bs and
codec.gram_mt_tiled ALTERNATED call by call, every call's time kept; medians and spreads (max - min)
are reported.  The bar (case a, every K): the bit-sliced call faster beyond the two calls' combined
spread.  One more bit-sliced call runs under codec.profile for the jump launches' share.  The
largest distance between the two matrices is reported as a share of the header's bound,
2 n 2^-52 sqrt(G_rr G_cc).

Prints one JSON line.  python tools/gram_mt_bs_rate.py [--calls 5] [--warmup 1] [--case a|b|both] [--ks ...]"""
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
    print(f"[gram_mt_bs_rate] {msg}", file=sys.stderr, flush=True)


def _median(v):
    return sorted(v)[len(v) // 2]


def _case(specs, total, k, seeds, calls, warmup):
    from fate_llm.algo.fedkseed import codec
    s = seeds[:k]

    def bs():
        return codec.gram_mt_bs(specs, s)

    def tiled():
        return codec.gram_mt_tiled(specs, s)

    first = bs().cpu()
    for _ in range(warmup):
        bs()
        tiled()
    torch.cuda.synchronize()
    b_ms, t_ms = [], []
    for i in range(calls):
        t, last = _event_ms(bs)
        b_ms.append(round(t, 3))
        t, ref = _event_ms(tiled)
        t_ms.append(round(t, 3))
        _say(f"K = {k}: call {i + 1} of {calls}: bit-sliced {b_ms[-1]:.2f} ms, tiled {t_ms[-1]:.2f} ms")
    last, ref = last.cpu(), ref.cpu()
    if not torch.equal(first.view(torch.int64), last.view(torch.int64)):
        raise SystemExit("gram_mt_bs_rate: two calls over the same inputs gave different bits")
    if not torch.equal(last.view(torch.int64), last.t().contiguous().view(torch.int64)):
        raise SystemExit("gram_mt_bs_rate: the matrix is not exactly symmetric")
    d = ref.diag().sqrt()
    share = float(((last - ref).abs() / (2.0 * total * 2.0 ** -52 * torch.outer(d, d))).max())
    with codec.profile() as pr:
        bs()
        torch.cuda.synchronize()
    spread = (max(b_ms) - min(b_ms)) + (max(t_ms) - min(t_ms))
    return {"seeds": k, "bs_ms": b_ms, "tiled_ms": t_ms, "bs_median_ms": _median(b_ms), "tiled_median_ms": _median(t_ms),
            "bs_spread_ms": round(max(b_ms) - min(b_ms), 3), "tiled_spread_ms": round(max(t_ms) - min(t_ms), 3),
            "bs_over_tiled": round(_median(b_ms) / _median(t_ms), 4),
            "faster_beyond_the_combined_spread": _median(t_ms) - _median(b_ms) > spread,
            "jump_ms": round(pr.jump_ms, 3), "n_jump": pr.n_jump, "kernel_ms": round(pr.apply_ms, 3),
            "n_kernel": pr.n_apply,
            "jump_share_of_device_time": round(pr.jump_ms / max(pr.jump_ms + pr.apply_ms, 1e-9), 4),
            "largest_share_of_the_bound_against_gram_mt_tiled": share}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=["a", "b", "both"], default="both")
    ap.add_argument("--ks", type=int, nargs="*", default=None, help="seed counts of the case (one case only)")
    args = ap.parse_args()
    from fate_llm.algo.fedkseed import _native
    dev = torch.device("cuda", 0)
    seeds = torch.randint(0, 2**32, (1024,), generator=torch.Generator().manual_seed(1)).tolist()
    out = {"what": "fks_gram_mt_bs beside fks_gram_mt_tiled, torch_cpu stream, bf16", "calls": args.calls,
           "warmup": args.warmup, "build_id": _native.build_id(), "source_id": _native.source_id()}
    if args.case in ("a", "both"):
        numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
        specs, store = _layout(numels, dev)
        out["a"] = {"layout": "Llama-2-7B", "tensors": len(numels), "params": sum(numels)}
        for k in args.ks or [32, 64, 256]:
            out["a"][f"k{k}"] = _case(specs, sum(numels), k, seeds, args.calls, args.warmup)
        del specs, store
        torch.cuda.empty_cache()
    if args.case in ("b", "both"):
        numels = [8 * 4096] * (32 * 2 * 2)  # tools/gram_mt_rate.py's adapter: 4,194,304 elements
        specs, store = _layout(numels, dev)
        out["b"] = {"layout": "adapter, rank 8 on the q and v projections (4096 x 4096) of 32 layers",
                    "tensors": len(numels), "params": sum(numels)}
        for k in args.ks or [256, 1024]:
            out["b"][f"k{k}"] = _case(specs, sum(numels), k, seeds, args.calls, args.warmup)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
