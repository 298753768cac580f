"""The tiled seed-basis Gram matrix (fks_gram_tiled) against fks_gram, call by call in one process.

fks_gram is untouched by the tiled call's arrival, so it is the parent's kernel on the same build
and the same device: codec.gram_tiled and codec.gram alternate, one call each per round, HIP events
around every call on the current stream, 1 warm-up round and 5 timed ones.

Cases, all bf16 and symmetric:
  7b:K       K seeds over the 291 tensors of the Llama-2-7B layout (K = 32, 64)
  adapter:K  K seeds over the adapter layout of tools/gram_rate.py, 4,194,304 elements in 128 tensors
             (K = 256, 4096; fks_gram at K = 4096 takes half a minute: one timed call, no warm-up)
The bar is the sign of the comparison on 7b:64 and adapter:256: the slowest timed tiled call below
the fastest timed fks_gram call.  Also reports how far the tiled call is from the f64 compute
bound K^2 N flop / 78.6 TF (2 flop per pair and element, the pairs c >= r), and the cycles per
v_mfma_f64_16x16x4_f64 and SIMD that the time would mean if the MFMAs alone filled it.

Prints one JSON line.  python tools/gram_tiled_rate.py [--cases 7b:32,7b:64,adapter:256,adapter:4096]
A tile variant (make -C fate-llm_amd variant_gram_tiled NAME=x DEFS=...) is timed by loading it with
FKS_LIB_OVERRIDE=fate-llm_amd/ab/libfks_x.so."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import bench  # noqa: E402
from gram_rate import _layout, _say  # noqa: E402

F64_PEAK = 78.6e12   # MI355X f64, vector and matrix alike (flop/s)
CLOCK = 2.4e9        # peak engine clock (Hz)
ROUNDS, WARMUP = 5, 1


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ms, key):
    return {f"{key}_ms_median": round(statistics.median(ms), 3), f"{key}_ms_min": round(min(ms), 3),
            f"{key}_ms_max": round(max(ms), 3), f"{key}_calls": len(ms)}


def _count(fn, k):
    n = ctypes.c_int32(0)
    from fate_llm.algo.fedkseed import _native
    _native.check(fn(k, k, 1, None, 0, ctypes.byref(n)))
    return n.value


def _case(name, numels, k, dev, g, skip_gram=False):
    from fate_llm.algo.fedkseed import _native, codec
    L = _native.load()
    total = sum(numels)
    specs, store = _layout(numels, dev)
    seeds = torch.randint(0, 2**32, (k,), generator=g).tolist()
    tiled = lambda: codec.gram_tiled(specs, seeds, stream_mode="torch_rocm")  # noqa: E731
    plain = lambda: codec.gram(specs, seeds, stream_mode="torch_rocm")  # noqa: E731
    t0 = time.perf_counter()
    first = tiled().cpu()
    _say(f"{name}: first tiled call (plan upload included) {time.perf_counter() - t0:.3f} s")
    once = k >= 2048  # fks_gram takes half a minute there: one timed call, no warm-up
    t_ms, g_ms, G = [], [], None
    for r in range(WARMUP + ROUNDS):
        ms, T = _event_ms(tiled)
        if r >= WARMUP:
            t_ms.append(ms)
        if not skip_gram and (not once or r == WARMUP):
            ms, G = _event_ms(plain)
            if r >= WARMUP:
                g_ms.append(ms)
        _say(f"{name}: round {r} done at {time.perf_counter() - t0:.1f} s")
    T = T.cpu()
    if not torch.equal(first.view(torch.int64), T.view(torch.int64)):
        raise SystemExit("gram_tiled_rate: two calls over the same inputs gave different bits")
    if not torch.equal(T.view(torch.int64), T.t().contiguous().view(torch.int64)):
        raise SystemExit("gram_tiled_rate: the matrix is not exactly symmetric")
    b = codec._Batch(specs, "torch_rocm", stage=False)
    nbytes = ctypes.c_size_t(0)
    _native.check(L.fks_gram_tiled_workspace_size(ctypes.addressof(b.arr), b.n, k, k, ctypes.byref(nbytes)))
    passes = _count(L.fks_gram_tiled_passes, k)
    cells = k * (k + 1) // 2
    tm = statistics.median(t_ms)
    tr, tc = codec._gram_tiled_tile()
    # what a pass computes: its live 16-blocks, on the tile grid
    mfma = 0
    n = ctypes.c_int32(0)
    buf = (ctypes.c_int32 * (4 * passes))()
    _native.check(L.fks_gram_tiled_passes(k, k, 1, ctypes.addressof(buf), passes, ctypes.byref(n)))
    for i in range(passes):
        mfma += -(-buf[4 * i + 1] // 16) * -(-buf[4 * i + 3] // 16)
    # a block pair takes 4 MFMAs per quad of items (16 elements): total / 4 MFMAs per block pair
    mfma_total = mfma * (total / 4.0)
    out = {"layout": name, "tensors": len(numels), "params": total, "seeds": k, "tile": [tr, tc],
           "passes": passes, "cells": cells, **_stats(t_ms, "tiled"),
           "tiled_ns_per_cell": round(tm * 1e6 / cells, 3),
           "tiled_us_per_pass": round(tm * 1e3 / passes, 3),
           "compute_bound_ms": round(k * k * total / F64_PEAK * 1e3, 3),
           "tiled_over_compute_bound": round(tm / (k * k * total / F64_PEAK * 1e3), 3),
           "mfma_issued": int(mfma_total),
           "cycles_per_mfma_per_simd_if_mfma_bound": round(tm * 1e-3 * CLOCK * torch.cuda.get_device_properties(dev).multi_processor_count * 4 / mfma_total, 2),
           "workspace_bytes": int(nbytes.value),
           "diag_over_n_min": float(T.diag().min()) / total, "diag_over_n_max": float(T.diag().max()) / total}
    if g_ms:
        G = G.cpu()
        diag = G.diag()
        bound = 2 * total * 2.0 ** -52 * torch.sqrt(torch.outer(diag, diag))
        if not bool(((T - G).abs() <= bound).all()):
            raise SystemExit("gram_tiled_rate: the tiled matrix is not within 2 n 2^-52 sqrt(G_rr G_cc) of fks_gram's")
        gm = statistics.median(g_ms)
        out.update({**_stats(g_ms, "gram"), "gram_passes": _count(L.fks_gram_passes, k),
                    "gram_ns_per_cell": round(gm * 1e6 / cells, 3),
                    "gram_over_tiled": round(gm / tm, 3),
                    "slowest_tiled_below_fastest_gram": max(t_ms) < min(g_ms),
                    "max_abs_diff_over_bound": float(((T - G).abs() / bound).max())})
    del specs, store
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="7b:32,7b:64,adapter:256,adapter:4096")
    ap.add_argument("--skip-gram", action="store_true", help="time the tiled call alone (tile variants)")
    args = ap.parse_args()
    from fate_llm.algo.fedkseed import _native
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    out = {"what": "fks_gram_tiled against fks_gram, torch_rocm stream, bf16, symmetric", "rounds": ROUNDS,
           "warmup": WARMUP, "build_id": _native.build_id(), "source_id": _native.source_id(),
           "lib": os.environ.get("FKS_LIB_OVERRIDE", "libfks.so"), "cases": []}
    for case in args.cases.split(","):
        layout, k = case.split(":")
        if layout == "7b":
            numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
        elif layout == "adapter":
            numels = [8 * 4096] * (32 * 2 * 2)  # rank 8 on q and v of 32 layers: 4,194,304 elements
        else:
            ap.error(f"unknown layout {layout}")
        out["cases"].append(_case(case, numels, int(k), dev, g, args.skip_gram))
        _say(json.dumps(out["cases"][-1]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
