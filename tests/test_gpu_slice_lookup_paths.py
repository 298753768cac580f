"""GPU parity of the bf16 slice kernel's table lookups and task addressing
(fks_apply_bs_kernel): the radius lookups of the zero-weight-decay chain that go through
vector memory (3 of every byte column's 8 seeds, loaded at the task head) beside those
that stay on the LDS, the row index of a wave's tasks carried from task to task (+144 mod
624 per 768-word stride) instead of divided out, and the parameter fetch on 32-bit segment
bounds (chunk word offsets) with the segment's address of chunk word 0.

Bar: bit-exact against the CPU oracle, as in test_gpu_slice.py (whose helpers are reused).
Shapes: one-task chunks (16, 48), segments that end inside a task, a wrap of the row index
inside a wave's stride (624*16 + 32), and 2^16 elements, which draw every one of the 256
radius indices in every seed (a missing index has probability below 1e-100).  K = 20, 33,
64, 65, 87: partial slices, a full pass, an empty second slice, a 23-seed remainder;
weight decay 0.0, -0.0, 0.01 and None (the three chains); two-slice passes and
FKS_BS_SLICES=1.  The oracle's result of a (K, wd) pair is computed once and shared.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fks_oracle as O
from test_gpu_parity import _dev, _gpu_reconstruct, from_np, rand_params, to_np
from test_gpu_slice import _seeds
from conftest import as_float, assert_bitwise

pytestmark = pytest.mark.gpu

SHAPES = [16, 48, 624 * 16 + 32, 2**16, 4096 * 3]
WDS = {"0.0": 0.0, "-0.0": -0.0, "0.01": 0.01, "None": None}


@functools.lru_cache(maxsize=None)
def _case(k, wdkey):
    """(initial arrays, seeds, values, the oracle's result) of one (K, wd) pair; read only."""
    init = rand_params(SHAPES, "bfloat16", seed=300 + k)
    seeds, vals = _seeds(k, seed=400 + k)
    want = [a.copy() for a in init]
    n = len(SHAPES)
    O.reconstruct(want, [O.BF16] * n, [1e-3] * n, [WDS[wdkey]] * n, seeds, vals)
    return init, seeds, vals, want


@pytest.mark.parametrize("slices", [None, "1"])
@pytest.mark.parametrize("wdkey", list(WDS))
@pytest.mark.parametrize("k", [20, 33, 64, 65, 87])
def test_lookup_paths_vs_oracle(monkeypatch, k, wdkey, slices):
    if slices is None:
        monkeypatch.delenv("FKS_BS_SLICES", raising=False)
    else:
        monkeypatch.setenv("FKS_BS_SLICES", slices)
    init, seeds, vals, want = _case(k, wdkey)
    n = len(SHAPES)
    got = _gpu_reconstruct([a.copy() for a in init], "bfloat16", [1e-3] * n, [WDS[wdkey]] * n, seeds, vals)
    for i, (a, b) in enumerate(zip(got, want)):
        assert_bitwise(a, b, "bfloat16", f"K={k} wd={wdkey} slices={slices} tensor {i}")


def test_lookup_paths_multiblock_chunks():
    """Many tasks per wave: 2^20 + 624*48 + 32 elements are 1,729 MT blocks, 6 or 7 per
    chunk of a two-slice pass (about 33 tasks, 5 or 6 per wave), so the carried row index wraps
    several times in every wave and each task's lookups run beside the next task's
    parameter prefetch.  K = 70 (a full pass and a 6-seed one), weight decay 0.0."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    shapes = [1 << 20, 624 * 48 + 32]
    arrays = rand_params(shapes, "bfloat16", seed=71)
    seeds, vals = _seeds(70, seed=72)
    ts = [from_np(a, "bfloat16", dev) for a in arrays]
    specs = [codec.ParamSpec(t, lr=1e-5, weight_decay=0.0) for t in ts]
    codec.directional_step(specs, seeds, vals)
    torch.cuda.synchronize()
    O.reconstruct(arrays, [O.BF16] * 2, [1e-5] * 2, [0.0] * 2, seeds, vals)
    for i, (t, a) in enumerate(zip(ts, arrays)):
        assert_bitwise(to_np(t), a, "bfloat16", f"tensor {i}")


@pytest.mark.parametrize("wd", [0.0, -0.0])
def test_lookup_paths_edge_values(wd):
    """The zero-weight-decay edge test's idea at the slice kernel's K = 40: parameters of
    +-0, +-inf, NaN, denormals and 3e38, directional values tiny, huge and negative.  A
    radius taken from the wrong table entry on either lookup path, or a lost sign of
    R[0] C (R[0] = -0), shows in these bits."""
    n = 64 * 1024
    base = rand_params([n], "bfloat16", seed=5)[0]
    f = as_float(base, "bfloat16").astype(np.float32)
    f[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-39, 3e38]
    f[8:16] = np.float32(-1.2e-38) * np.arange(8, dtype=np.float32)
    f[5000:5016] = -0.0
    f[7000:7016] = 0.0
    arr = to_np(torch.from_numpy(f).to(torch.bfloat16))
    seeds, vals = _seeds(40, seed=57)
    for i, e in enumerate([-1e-45, 1e-45, -3e38, -5.0, 1e30, -0.5], start=1):  # seed 0 keeps an ordinary value
        vals[i] = e
    got = _gpu_reconstruct([arr], "bfloat16", [1e-2], [wd], seeds, vals)
    O.reconstruct([arr], [O.BF16], [1e-2], [wd], seeds, vals)
    assert_bitwise(got[0], arr, "bfloat16", f"wd {wd}")
    assert not np.array_equal(got[0][16:4096], base[16:4096])


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_lookup_paths_element_shards(wd):
    """Three element shards whose starts are not task-aligned to a segment: their union
    equals the oracle's whole reconstruct.  Weight decay 0.0 takes the chain with the 32-bit
    segment bounds and the carried row index, 0.01 the one with the 64-bit fetch."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    shapes = [2**17, 624 * 40]
    arrays = rand_params(shapes, "bfloat16", seed=6)
    seeds, vals = _seeds(50, seed=7)
    ts = [from_np(a, "bfloat16", dev) for a in arrays]
    specs = [codec.ParamSpec(t, lr=1e-3, weight_decay=wd) for t in ts]
    for r in range(3):
        codec.directional_step(specs, seeds, vals, shard=r, nshards=3)
    torch.cuda.synchronize()
    O.reconstruct(arrays, [O.BF16] * 2, [1e-3] * 2, [wd] * 2, seeds, vals)
    for i, (t, a) in enumerate(zip(ts, arrays)):
        assert_bitwise(to_np(t), a, "bfloat16", f"wd {wd} tensor {i}")
