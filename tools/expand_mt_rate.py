"""Timing of fks_expand_mt_multi (codec.expand_mt_multi, torch_cpu stream) on the 7B bf16 layout of
the bench, one MI355X, against what a user did before it for the same result, measured in the same
run on the same box:

  python tools/expand_mt_rate.py [LOG]        (default LOG: profiles/expand_mt_rate_7b.log)

HIP events on the current stream, EMT_WARMUP warm-ups (2), then the median of EMT_CALLS calls
(10); the cases of a measurement alternate over EMT_ROUNDS rounds (3).  Every line is JSON and
carries median, min and max; the first line holds the build and source ids.

  1. one bf16 output, 19 seeds (one pass, no staging area):
       delta19          fks_delta_accumulate, 19 seeds, into a zeroed-once f32 buffer of the model's size
       delta19_convert  that launch plus the per-tensor conversion of the buffer to bf16 tensors
       expand19         codec.expand_mt_multi into the same bf16 tensors
     the summary compares expand19 with delta19_convert and gives the baseline's spread over the rounds.
  2. K = 1 into bf16 .grads end to end through zo_utils.seed_expansion_on_stream_: time, and the
     peak of torch's allocator above the model and the gradients.
  3. K = EMT_LONG_K (4055) seeds, one bf16 output, default staging budget: time of one call after
     one warm-up call, internal shard count, peak memory, and the jump time of fks_profile_*;
     fks_delta_accumulate at the same K beside it.  EMT_LONG_K=0 skips it.

No threshold here: the figures go to DESIGN.md."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fate-llm_amd", "python"))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("EMT_CALLS", "10"))
WARMUP = int(os.environ.get("EMT_WARMUP", "2"))
ROUNDS = int(os.environ.get("EMT_ROUNDS", "3"))
LONG_K = int(os.environ.get("EMT_LONG_K", "4055"))


def main():
    import torch

    import bench
    from fate_llm.algo.fedkseed import _native, codec, zo_utils

    log_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "expand_mt_rate_7b.log")
    log = open(log_path, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def timed(fn, calls=CALLS, warmup=WARMUP):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}

    dev = torch.device("cuda", 0)
    codec.set_stream_mode("torch_cpu")
    numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
    total = sum(numels)
    emit(what="ids", build_id=_native.build_id(), source_id=_native.source_id(), device=torch.cuda.get_device_name(dev),
         tensors=len(numels), elements=total, calls=CALLS, warmup=WARMUP, rounds=ROUNDS)
    g = torch.Generator().manual_seed(1)
    seeds = torch.randint(0, 2**32, (max(LONG_K, 19),), generator=g).tolist()
    coefs = (torch.randn(max(LONG_K, 19), generator=g, dtype=torch.float64) * 1e-3).tolist()

    def cut(buf):
        out, at = [], 0
        for n in numels:
            out.append(buf[at:at + n])
            at += n
        return out

    store = torch.empty(total, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
    params = [torch.nn.Parameter(t) for t in cut(store)]
    specs = [codec.ParamSpec(p.data) for p in params]
    outs = cut(torch.zeros(total, dtype=torch.bfloat16, device=dev))

    # ---- 1. one bf16 output, 19 seeds
    delta = torch.zeros(total, dtype=torch.float32, device=dev)
    dcut = cut(delta)

    def delta19():
        codec.delta_accumulate(specs, seeds[:19], coefs[:19], delta)

    def delta19_convert():
        codec.delta_accumulate(specs, seeds[:19], coefs[:19], delta)
        for o, d in zip(outs, dcut):
            o.copy_(d)

    def expand19():
        codec.expand_mt_multi(specs, seeds[:19], [coefs[:19]], [outs])

    med = {}
    for r in range(ROUNDS):
        for name, fn in (("delta19", delta19), ("delta19_convert", delta19_convert), ("expand19", expand19)):
            t = timed(fn)
            med.setdefault(name, []).append(t["ms_median"])
            emit(what=name, round=r, **t)
    delta.zero_()
    delta19()
    expand19()
    torch.cuda.synchronize()
    same = all(torch.equal(o.view(torch.int16), d.bfloat16().view(torch.int16)) for o, d in zip(outs, dcut))
    m = {k: statistics.median(v) for k, v in med.items()}
    emit(what="summary19", expand19_ms=m["expand19"], delta19_ms=m["delta19"], delta19_convert_ms=m["delta19_convert"],
         delta19_convert_ms_over_rounds=[min(med["delta19_convert"]), max(med["delta19_convert"])],
         expand19_ms_over_rounds=[min(med["expand19"]), max(med["expand19"])],
         expand19_over_delta19=round(m["expand19"] / m["delta19"], 4),
         expand19_over_delta19_convert=round(m["expand19"] / m["delta19_convert"], 4),
         expand19_equals_converted_delta=bool(same))
    del delta, dcut

    # ---- 2. K = 1 into bf16 .grads, end to end
    for p, o in zip(params, outs):
        p.grad = o
    groups = [{"params": params}]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    t = timed(lambda: zo_utils.seed_expansion_on_stream_(groups, seeds[:1], coefs[:1], stream_mode="torch_cpu"))
    emit(what="e2e_k1_seed_expansion_on_stream_", peak_bytes_above_model_and_grads=torch.cuda.max_memory_allocated(dev) - before,
         **t)

    # ---- 3. a long sum
    if LONG_K > 19:
        K = LONG_K
        b = codec._Batch(specs, "torch_cpu", stage=False)
        whole = codec._expand_mt_sizes(b, K, 1, 1)[0][1]
        budget = max(codec.EXPAND_MT_STAGING_MIN, -(-whole // codec.EXPAND_MT_STAGING_SPLIT))
        ns = 1
        while max(st for _, st in codec._expand_mt_sizes(b, K, 1, ns)) > budget:
            ns += 1

        def long_expand():
            codec.expand_mt_multi(specs, seeds[:K], [coefs[:K]], [outs])

        long_expand()  # the shards' plans
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        t = timed(long_expand, calls=1, warmup=0)
        peak = torch.cuda.max_memory_allocated(dev) - before
        with codec.profile() as pr:
            long_expand()
            torch.cuda.synchronize()
        emit(what="expand_long", seeds=K, shards=ns, staging_bytes_whole_list=whole, staging_budget=budget,
             peak_bytes_above_model_and_output=peak, profiled_apply_ms=round(pr.apply_ms, 1), profiled_jump_ms=round(pr.jump_ms, 1),
             n_apply=pr.n_apply, n_jump=pr.n_jump, **t)
        delta = torch.zeros(total, dtype=torch.float32, device=dev)

        def long_delta():
            codec.delta_accumulate(specs, seeds[:K], coefs[:K], delta)

        long_delta()
        torch.cuda.synchronize()
        td = timed(long_delta, calls=1, warmup=0)
        with codec.profile() as pd:
            long_delta()
            torch.cuda.synchronize()
        emit(what="delta_long", seeds=K, profiled_apply_ms=round(pd.apply_ms, 1), profiled_jump_ms=round(pd.jump_ms, 1),
             n_apply=pd.n_apply, n_jump=pd.n_jump, **td)
        emit(what="summary_long", seeds=K, shards=ns, expand_over_delta=round(t["ms_median"] / td["ms_median"], 4),
             expand_jump_share=round(pr.jump_ms / max(pr.jump_ms + pr.apply_ms, 1e-9), 4),
             delta_jump_share=round(pd.jump_ms / max(pd.jump_ms + pd.apply_ms, 1e-9), 4))
    log.close()


if __name__ == "__main__":
    main()
