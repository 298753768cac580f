"""Host paths of libfks.so that the parity tests reach but cannot tell apart: whether the
one-seed caches (window cache, z-index cache) and the pass structure of a reconstruct
launch exactly the kernels the launch driver (fks_run.cpp) means to -- a cache that never
hit would still give the right parameters -- and the eviction of the two plan LRUs
(fks_cache.cpp: 32 entries each), which no other test fills.

Launch counts come from codec.profile() (events around every jump and apply launch).
Every sequence is also checked bit for bit against the oracle (torch_cpu stream) or
torch's own ops on the device (torch_rocm stream)."""
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
