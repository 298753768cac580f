"""Timing of fks_expand_multi against fks_delta_accumulate of the same build on the 7B bf16 layout
of the bench, one MI355X, everything in one process:

  python tools/expand_rate.py            (FKS_LIB_OVERRIDE=ab/libfks_x.so: a variant build)

The C ABI through ctypes (no Python layer in the timed region); HIP events around each call on the
current stream, ER_WARMUP warm-ups (2), then ER_CALLS timed calls (10); every line carries median,
min and max.

  a  one bf16 output, 32 seeds, against one 32-seed fks_delta_accumulate launch into the f32
     concatenation (27 GB), the two alternated ER_ROUNDS times (3): the margin of the ratio is the
     spread of the baseline's own medians over the rounds;
     and once one f32 output with beta 1 into that 27 GB buffer: the baseline's own memory traffic (27 GB
     read, 27 GB written) under the new kernel, which tells the traffic's share of a difference
     from the loop's;
  b  two, three and four bf16 outputs (13.5 GB each) in one call against that many one-output calls;
  c  K = ER_LONG_K (4055) into one bf16 output against fks_delta_accumulate of the same K, one call
     each, with the peak of torch's allocator above the model and the output: the workspace alone
     against the 27 GB buffer (ER_LONG_K=0 skips it).

The summary line at the end holds the ratios.  No threshold here: the figures go to DESIGN.md."""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fate-llm_amd", "python"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from fate_llm.algo.fedkseed import _native as N  # noqa: E402

CALLS, WARMUP = int(os.environ.get("ER_CALLS", "10")), int(os.environ.get("ER_WARMUP", "2"))
ROUNDS, LONG_K = int(os.environ.get("ER_ROUNDS", "3")), int(os.environ.get("ER_LONG_K", "4055"))
Z = ctypes.c_size_t


def emit(what, **kw):
    print(json.dumps(dict({"what": what}, **kw)), flush=True)


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


def main():
    L = N.load()
    dev = torch.device("cuda", 0)
    numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
    total, nt = sum(numels), len(numels)
    g = torch.Generator().manual_seed(1)
    kmax = max(32, LONG_K)
    seeds = torch.randint(0, 2**32, (kmax,), generator=g).numpy().astype("uint64")
    coefs = (torch.randn(4 * kmax, generator=g, dtype=torch.float64) * 1e-3).numpy()
    stream = torch.cuda.current_stream(dev).cuda_stream
    emit("ids", build_id=N.build_id(), source_id=N.source_id(), elements=total, tensors=nt)

    # the parameters are never read by the expansion (their addresses key the plan): one bf16 buffer cut into the layout
    store = torch.empty(total, dtype=torch.bfloat16, device=dev)
    arr = (N.FksTensor * nt)()
    at = 0
    for i, n in enumerate(numels):
        arr[i].data, arr[i].numel, arr[i].dtype, arr[i].flags = store.data_ptr() + 2 * at, n, N.BF16, N.STREAM_ROCM
        at += n
    outs = [torch.empty(total, dtype=torch.bfloat16, device=dev) for _ in range(4)]

    def vecs(bufs):
        v = (N.FksVec * (len(bufs) * nt))()
        for m, b in enumerate(bufs):
            at = 0
            for i, n in enumerate(numels):
                v[m * nt + i].data = b.data_ptr() + b.element_size() * at
                v[m * nt + i].dtype = N.F32 if b.dtype == torch.float32 else N.BF16
                at += n
        return v

    def expand_call(bufs, k, beta=None):
        M, v, n = len(bufs), vecs(bufs), Z(0)
        bt = None if beta is None else np.full(M, beta, dtype=np.float64)
        N.check(L.fks_expand_multi_workspace_size(ctypes.addressof(arr), nt, k, M, ctypes.byref(n)))
        ws = torch.empty(max(n.value, 1), dtype=torch.uint8, device=dev)
        c = np.ascontiguousarray(coefs[:M * k])

        def fn():
            N.check(L.fks_expand_multi(ctypes.addressof(arr), nt, seeds.ctypes.data, c.ctypes.data, k,
                                       ctypes.addressof(v), None if bt is None else bt.ctypes.data, M, 0, 1,
                                       ws.data_ptr(), n.value, stream))
        fn.ws_bytes = n.value
        return fn

    def delta_call(delta, k):
        n = Z(0)
        N.check(L.fks_delta_workspace_size(ctypes.addressof(arr), nt, k, ctypes.byref(n)))
        ws = torch.empty(max(n.value, 1), dtype=torch.uint8, device=dev)
        c = np.ascontiguousarray(coefs[:k])

        def fn():
            N.check(L.fks_delta_accumulate(ctypes.addressof(arr), nt, seeds.ctypes.data, c.ctypes.data, k,
                                           delta.data_ptr(), ws.data_ptr(), n.value, stream))
        fn.ws_bytes = n.value
        return fn

    delta = torch.zeros(total, dtype=torch.float32, device=dev)
    base, one = delta_call(delta, 32), expand_call(outs[:1], 32)
    med = {"delta32": [], "expand32": []}
    for r in range(ROUNDS):  # a: alternated, so that the baseline's spread over the session is seen
        for name, fn in (("delta32", base), ("expand32", one)):
            t = timed(fn)
            med[name].append(t["ms_median"])
            emit(name, round=r, **t)
    emit("expand32_workspace", bytes=one.ws_bytes)
    same_traffic = timed(expand_call([delta], 32, beta=1.0))
    emit("expand32_f32_beta1", **same_traffic)
    multi = {}
    for M in (2, 3, 4):  # b: M outputs in one call against M one-output calls
        multi[M] = timed(expand_call(outs[:M], 32))
        emit("expand32_m%d" % M, **multi[M])
    long_rows = {}
    if LONG_K:  # c: one call each, nothing to warm but the plans the runs above built
        for name, fn in (("delta", delta_call(delta, LONG_K)), ("expand", expand_call(outs[:1], LONG_K))):
            long_rows[name] = timed(fn, calls=1, warmup=0)
            emit("%s_k%d" % (name, LONG_K), **long_rows[name])
        del delta
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        for name in ("expand", "delta"):  # the allocator's peak above the model and the bf16 output, one seed pass
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            if name == "expand":
                expand_call(outs[:1], LONG_K)()
            else:
                d = torch.zeros(total, dtype=torch.float32, device=dev)
                delta_call(d, 32)()
                outs[0].copy_(d)  # the conversion pass a bf16 result costs on this path
                del d
            torch.cuda.synchronize()
            emit("peak_%s" % name, bytes_above_model_and_output=torch.cuda.max_memory_allocated(dev) - before)
    b, e = statistics.median(med["delta32"]), statistics.median(med["expand32"])
    emit("summary", rounds=ROUNDS, delta32_ms=b, delta32_ms_over_rounds=[min(med["delta32"]), max(med["delta32"])],
         expand32_ms=e, expand32_ms_over_rounds=[min(med["expand32"]), max(med["expand32"])],
         expand32_over_delta32=round(e / b, 4),
         expand32_f32_beta1_over_delta32=round(same_traffic["ms_median"] / b, 4),
         baseline_spread=round((max(med["delta32"]) - min(med["delta32"])) / b, 4),
         **{"m%d_over_%d_singles" % (M, M): round(multi[M]["ms_median"] / (M * e), 4) for M in multi},
         **({"delta_k_ms": long_rows["delta"]["ms_median"], "expand_k_ms": long_rows["expand"]["ms_median"],
             "long_k": LONG_K} if long_rows else {}))


if __name__ == "__main__":
    main()
