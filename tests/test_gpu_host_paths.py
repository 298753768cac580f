"""Host paths of libfks.so that the parity tests reach but cannot tell apart: whether the
one-seed caches (window cache, z-index cache) and the pass structure of a reconstruct
launch exactly the kernels the launch driver (fks_run.cpp) means to -- a cache that never
hit would still give the right parameters -- and the eviction of the two plan LRUs
(fks_cache.cpp: 32 entries each), which no other test fills.

Launch counts come from codec.profile() (events around every jump and apply launch).
Every sequence is also checked bit for bit against the oracle (torch_cpu stream) or
torch's own ops on the device (torch_rocm stream)."""
import ctypes
import os

import pytest
import torch

from oracle import fks_oracle as O
from oracle import torch_replica as R
from test_gpu_parity import DTC, _dev, from_np, rand_params, to_np

pytestmark = pytest.mark.gpu

# list A: one bf16 tensor of 27 MT blocks (fast path only); B: A and an f32 tensor; C: B and
# an f32 tensor of 7 elements (irregular work)
LISTS = {"A": [("bfloat16", 16384)], "B": [("bfloat16", 16384), ("float32", 1024)],
         "C": [("bfloat16", 16384), ("float32", 1024), ("float32", 7)]}
PERTURBS = [(11, 5e-4), (11, -1e-3), (12, 5e-4)]  # a seed, the same seed with another scale, a new seed


def _clear():
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    codec.zindex_release()
    codec.jwin_release()
    N.check(N.load().fks_plan_cache_clear())


def _arrays(layout, seed=3):
    return [rand_params([n], dt, seed=seed + i)[0] for i, (dt, n) in enumerate(layout)]


def _same(got, want, dt, what):
    a, b = to_np(got), want
    if dt == "float32":
        a, b = a.view("uint32"), b.view("uint32")
    assert (a == b).all(), what


# (list, environment, z-index buffer wanted, jumps, applies)
@pytest.mark.parametrize("name,env,zindex,jumps,applies", [
    ("A", {"FKS_ZCACHE": "0"}, False, 2, 3),                           # the window cache hits on the second call
    ("A", {"FKS_ZCACHE": "0", "FKS_NO_WIN_CACHE": "1"}, False, 3, 3),  # nothing cached: every call jumps
    ("A", {"FKS_NO_WIN_CACHE": "1"}, True, 2, 3),                      # the replay needs no windows
    ("B", {"FKS_NO_WIN_CACHE": "1"}, True, 3, 6),                      # the f32 segments still generate
])
def test_perturb_launch_counts(name, env, zindex, jumps, applies):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    _clear()
    layout = LISTS[name]
    arrays = _arrays(layout)
    os.environ.update(env)
    try:
        params = [from_np(a, dt, dev) for a, (dt, _) in zip(arrays, layout)]
        if zindex and not codec.zindex_reserve(codec._Batch([codec.ParamSpec(p) for p in params], "torch_cpu")):
            pytest.skip("the codec's memory budget does not allow a z-index buffer for this list")
        with codec.profile() as prof:
            for seed, scale in PERTURBS:
                codec.perturb(params, seed, scale)
        torch.cuda.synchronize()
    finally:
        for key in env:
            os.environ.pop(key, None)
        codec.zindex_release()
    print(f"list {name} {env}: jumps {prof.n_jump} applies {prof.n_apply}")
    assert (prof.n_jump, prof.n_apply) == (jumps, applies)
    for seed, scale in PERTURBS:
        O.perturb_params(arrays, [DTC[dt] for dt, _ in layout], seed, scale)
    for i, (p, a, (dt, _)) in enumerate(zip(params, arrays, layout)):
        _same(p, a, dt, f"list {name} {env}: tensor {i}")


def _seeds_values(k, seed=9):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2**32, (k,), generator=g).tolist(),
            (torch.randn(k, generator=g, dtype=torch.float64) * 20 + 0.5).tolist())


# K = 65, wd 0.0, no reconstruct window cache: A one two-slice pass and one split pass of the
# slice kernel; B four 19-seed passes for the f32 segments besides; C four irregular passes besides
@pytest.mark.parametrize("name,jumps,applies", [("A", 2, 2), ("B", 6, 6), ("C", 10, 10)])
def test_reconstruct_launch_counts(name, jumps, applies):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    _clear()
    layout = LISTS[name]
    arrays = _arrays(layout)
    seeds, vals = _seeds_values(65)
    params = [from_np(a, dt, dev) for a, (dt, _) in zip(arrays, layout)]
    specs = [codec.ParamSpec(p, lr=1e-3, weight_decay=0.0) for p in params]
    with codec.profile() as prof:
        codec.directional_step(specs, seeds, vals)
    torch.cuda.synchronize()
    print(f"list {name} K=65: jumps {prof.n_jump} applies {prof.n_apply}")
    assert (prof.n_jump, prof.n_apply) == (jumps, applies)
    O.reconstruct(arrays, [DTC[dt] for dt, _ in layout], [1e-3] * len(arrays), [0.0] * len(arrays), seeds, vals)
    for i, (p, a, (dt, _)) in enumerate(zip(params, arrays, layout)):
        _same(p, a, dt, f"list {name}: tensor {i}")


def test_reconstruct_launch_counts_torch_rocm():
    """List A on the torch_rocm stream, K = 65: three launches of at most 32 seeds, no jump."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    _clear()
    seeds, vals = _seeds_values(65)
    got = from_np(_arrays(LISTS["A"])[0], "bfloat16", dev)
    ref = [got.clone()]
    with codec.profile() as prof:
        codec.directional_step([codec.ParamSpec(got, lr=1e-3, weight_decay=0.0)], seeds, vals, stream_mode="torch_rocm")
    torch.cuda.synchronize()
    print(f"list A torch_rocm K=65: jumps {prof.n_jump} applies {prof.n_apply}")
    assert (prof.n_jump, prof.n_apply) == (0, 3)
    R.reconstruct(ref, seeds, vals, 1e-3, 0.0)
    assert torch.equal(got.view(torch.int16), ref[0].view(torch.int16))


def _gram_pass_list(fn, kr, kc, symmetric):
    """the (row0, nrows, col0, ncols) passes fks_gram*_passes reports for a call"""
    from fate_llm.algo.fedkseed import _native as N
    n = ctypes.c_int32(0)
    N.check(fn(kr, kc, int(symmetric), None, 0, ctypes.byref(n)))
    buf = (ctypes.c_int32 * (4 * n.value))()
    N.check(fn(kr, kc, int(symmetric), buf, n.value, ctypes.byref(n)))
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


def test_seed_basis_launch_counts():
    """The seed-basis calls on list C (two dtypes with fast segments, irregular work): the jumps
    and the timed launches of every driver are what its pass structure prescribes.  Per pass of the
    torch_cpu stream, R + I = 2 jumps (the regular and the irregular chunk starts) and D + I = 3
    launches (one per dtype with fast segments, the irregular one); the torch_rocm stream never
    jumps.  The results themselves are the bit-for-bit tests' (test_gpu_project*.py, test_gpu_gram*.py,
    test_gpu_expand*.py)."""
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    _clear()
    L = N.load()
    layout = LISTS["C"]
    params = [from_np(a, dt, dev) for a, (dt, _) in zip(_arrays(layout), layout)]
    specs = [codec.ParamSpec(p) for p in params]
    k, nvec, jumps, launches = 20, 3, 2, 3
    seeds, _ = _seeds_values(k)
    g = torch.Generator().manual_seed(5)
    vec = torch.randn(sum(n for _, n in layout), generator=g).to(dev)
    vectors = [[torch.randn(n, generator=g).to(dev) for _, n in layout] for _ in range(nvec)]
    coefs = torch.randn(nvec, k, generator=g, dtype=torch.float64).tolist()

    def counts(call):
        with codec.profile() as prof:
            call()
        torch.cuda.synchronize()
        return prof.n_jump, prof.n_apply

    def ceil(a, b):
        return -(-a // b)

    got, want = {}, {}
    # ---- the torch_cpu stream
    got["project_mt"] = counts(lambda: codec.project_mt(specs, seeds, vec))
    want["project_mt"] = (ceil(k, 19) * jumps, ceil(k, 19) * launches)
    # batches of PROJECT_MT_PASS_VECTORS vectors; a batch of one takes 19 seeds per pass, of two 10
    # (csrc/fks_project_mt.h proj_mt_pass_seeds)
    assert codec.PROJECT_MT_PASS_VECTORS == 2
    passes = ceil(k, 10) + ceil(k, 19)
    got["project_mt_multi"] = counts(lambda: codec.project_mt_multi(specs, seeds, vectors))
    want["project_mt_multi"] = (passes * jumps, passes * launches)
    for name, rows, cols in (("gram_mt 6", seeds[:6], None), ("gram_mt 5x7", seeds[:5], seeds[5:12])):
        tiles = _gram_pass_list(L.fks_gram_mt_passes, len(rows), len(cols or rows), cols is None)
        assert len(tiles) >= 2
        got[name] = counts(lambda: codec.gram_mt(specs, rows, cols))
        want[name] = ((len({t[0] for t in tiles}) + len(tiles)) * jumps, len(tiles) * launches)
    outs = [[torch.empty_like(p) for p in params] for _ in range(nvec)]
    got["expand_mt_multi"] = counts(lambda: codec.expand_mt_multi(specs, seeds, coefs, outs))
    want["expand_mt_multi"] = (nvec * ceil(k, 19) * jumps, nvec * ceil(k, 19) * launches)
    got["expand_mt_multi k=0"] = counts(lambda: codec.expand_mt_multi(specs, [], [[]] * nvec, outs))
    want["expand_mt_multi k=0"] = (0, nvec * launches)  # one pass without seeds: nothing to jump
    # ---- the torch_rocm stream: launches of at most 32 seeds, batches of at most four vectors or outputs
    assert nvec <= min(codec.EXPAND_PASS_OUTPUTS, 4)
    for kk in (k, 33):
        s = _seeds_values(kk)[0]
        got[f"project k={kk}"] = counts(lambda: codec.project(specs, s, vec, stream_mode="torch_rocm"))
        got[f"project_multi k={kk}"] = counts(lambda: codec.project_multi(specs, s, vectors, stream_mode="torch_rocm"))
        want[f"project k={kk}"] = want[f"project_multi k={kk}"] = (0, ceil(kk, 32))
    for name, fn, sizes in (("gram", codec.gram, L.fks_gram_passes),
                            ("gram_tiled", codec.gram_tiled, L.fks_gram_tiled_passes)):
        for what, rows, cols in (("6", seeds[:6], None), ("5x7", seeds[:5], seeds[5:12])):
            tiles = _gram_pass_list(sizes, len(rows), len(cols or rows), cols is None)
            got[f"{name} {what}"] = counts(lambda: fn(specs, rows, cols, stream_mode="torch_rocm"))
            want[f"{name} {what}"] = (0, len(tiles))
    assert len(_gram_pass_list(L.fks_gram_passes, 6, 6, True)) >= 2
    b = codec._Batch(specs, "torch_rocm", stage=False)
    for work in (0, 1):  # the call's own bound (one launch here), then a single row per launch
        ncuts, buf = ctypes.c_int32(0), (ctypes.c_int64 * 64)()
        with torch.cuda.device(dev):
            N.check(L.fks_expand_launch_cuts(ctypes.addressof(b.arr), b.n, k, 0, 1, work, 0, buf, 64,
                                             ctypes.byref(ncuts)))
        assert ncuts.value - 1 >= (2 if work else 1)
        if work:
            os.environ["FKS_EXPAND_WORK"] = str(work)
        try:
            got[f"expand_multi work {work}"] = counts(
                lambda: codec.expand_multi(specs, seeds, coefs, outs, stream_mode="torch_rocm"))
        finally:
            os.environ.pop("FKS_EXPAND_WORK", None)
        want[f"expand_multi work {work}"] = (0, ncuts.value - 1)
    for name in want:
        print(f"{name}: jumps, launches {got[name]}, prescribed {want[name]}")
    assert got == want


# ---- plan LRU eviction: 34 distinct lists against 32 entries ----
N_LISTS = 34


def _lru_calls():
    """(list, seeds, values) in call order: every list once, then lists 0 and 1 again (their
    plans were evicted) and list 33 (still cached)."""
    calls = [(i, [100 + i], [1.5 + 0.25 * i]) for i in range(N_LISTS)]
    return calls + [(0, [500], [-2.0]), (1, [501], [3.0]), (33, [502], [0.75])]


def _check_lru(calls, stream_mode):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    _clear()
    arrays = rand_params([16 * (i + 2) for i in range(N_LISTS)], "bfloat16", seed=17)
    params = [from_np(a, "bfloat16", dev) for a in arrays]
    ref = [p.clone() for p in params]
    for i, seeds, vals in calls:
        codec.directional_step([codec.ParamSpec(params[i], lr=1e-3, weight_decay=0.0)], seeds, vals,
                               stream_mode=stream_mode)
        if stream_mode == "torch_rocm":
            one = [ref[i]]
            R.reconstruct(one, seeds, vals, 1e-3, 0.0)
            ref[i] = one[0]
        else:
            O.reconstruct([arrays[i]], [O.BF16], [1e-3], [0.0], seeds, vals)
    torch.cuda.synchronize()
    for i in range(N_LISTS):
        if stream_mode == "torch_rocm":
            assert torch.equal(params[i].view(torch.int16), ref[i].view(torch.int16)), f"list {i}"
        else:
            _same(params[i], arrays[i], "bfloat16", f"list {i}")


def test_plan_lru_eviction_mt_stream():
    _check_lru(_lru_calls(), "torch_cpu")


def test_plan_lru_eviction_torch_rocm_stream():
    _check_lru(_lru_calls(), "torch_rocm")


def test_plan_lru_evicts_non_small_plan_keeps_small_one():
    """A K = 20 call on list 0 (its non-small plan), a K = 1 call on it (its small plan), then
    K = 1 calls on 31 other lists: 33 plans, so the least recently used -- the non-small one --
    goes while the small plan of the same tensor stays; both are then used again."""
    s20, v20 = _seeds_values(20, seed=4)
    calls = [(0, s20, v20), (0, [700], [1.25])] + [(i, [100 + i], [1.5 + 0.25 * i]) for i in range(1, 32)]
    calls += [(0, [701], [-0.5]), (0, [s + 1 for s in s20], v20)]
    _check_lru(calls, "torch_cpu")
