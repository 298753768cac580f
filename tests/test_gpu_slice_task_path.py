"""GPU parity of the bf16 slice kernel's task path (fks_apply_bs_kernel, the zero-weight-decay
chain): a lane's two parameters loaded and stored as 16-bit halves (elements toff and toff + 8
of a task from one address, 16 bytes apart, the sink included) instead of as an aligned pair
exchanged with the neighbour lane; two seeds' g per SGPR pair, the half chosen by op_sel; the
twist's row indices carried from task to task and wrapped by unsigned min, lanes past the
chunk's end on in-range rows with only their stores masked; the flip of the tempered planes
as a bitwise mux on a per-lane mask.

Bar: bit-exact against the CPU oracle (assert_bitwise), as in test_gpu_slice.py and
test_gpu_slice_lookup_paths.py, whose helpers are reused.  Shapes: one-task and sub-task
chunks (16, 48: most lanes on the sink), segments that end inside a task (boundaries at
multiples of 16 that are not multiples of 128), a row wrap inside a wave's stride
(624*16 + 32), a tensor whose length is no multiple of 16 (4096*3 + 5) and a view that starts
at an odd element of its storage (2-byte but not 4-byte aligned) beside fast tensors, many
tasks per wave (2^20 + 624*48 + 32 elements, K = 70), K = 20, 33, 64, 65, 87, weight decay
0.0, -0.0, 0.01 and None, two-slice passes and FKS_BS_SLICES=1, edge values, element shards.
The oracle's result of a (K, wd) pair is computed once and shared.
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

# segment boundaries at 12288, 12304, 12352, 77888 (= 16 mod 128 twice, 64 mod 128), then the
# row-wrap shape and the ragged one, whose successor starts off the 16-element grid
SHAPES = [4096 * 3, 16, 48, 2**16, 624 * 16 + 32, 4096 * 3 + 5, 4096]
WDS = {"0.0": 0.0, "-0.0": -0.0, "0.01": 0.01, "None": None}


@functools.lru_cache(maxsize=None)
def _case(k, wdkey):
    """(initial arrays, seeds, values, the oracle's result) of one (K, wd) pair; read only."""
    init = rand_params(SHAPES, "bfloat16", seed=500 + k)
    seeds, vals = _seeds(k, seed=600 + k)
    want = [a.copy() for a in init]
    n = len(SHAPES)
    O.reconstruct(want, [O.BF16] * n, [1e-3] * n, [WDS[wdkey]] * n, seeds, vals)
    return init, seeds, vals, want


@pytest.mark.parametrize("slices", [None, "1"])
@pytest.mark.parametrize("wdkey", list(WDS))
@pytest.mark.parametrize("k", [20, 33, 64, 65, 87])
def test_task_path_vs_oracle(monkeypatch, k, wdkey, slices):
    if slices is None:
        monkeypatch.delenv("FKS_BS_SLICES", raising=False)
    else:
        monkeypatch.setenv("FKS_BS_SLICES", slices)
    init, seeds, vals, want = _case(k, wdkey)
    n = len(SHAPES)
    got = _gpu_reconstruct([a.copy() for a in init], "bfloat16", [1e-3] * n, [WDS[wdkey]] * n, seeds, vals)
    for i, (a, b) in enumerate(zip(got, want)):
        assert_bitwise(a, b, "bfloat16", f"K={k} wd={wdkey} slices={slices} tensor {i}")


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_task_path_odd_view_and_ragged(wd):
    """A bf16 view that starts at element 1 of its storage (2-byte aligned only) between a
    ragged tensor and fast ones.  Whichever kernel takes the unaligned and ragged parts, every
    tensor stays exact and the storage's guard elements on both sides of the view keep their
    bits (a 16-bit store that went 16 bytes too far, or a pair store, would change them)."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    shapes = [4096 * 3 + 5, 4096 * 2 + 16, 16, 48, 4096]
    arrays = rand_params(shapes, "bfloat16", seed=81)
    guard = np.full(16, 0x3F80, dtype=np.uint16)  # 1.0
    store = from_np(np.concatenate([guard[:1], arrays[1], guard]), "bfloat16", dev)
    ts = [from_np(a, "bfloat16", dev) for a in arrays]
    ts[1] = store[1:1 + shapes[1]]
    assert ts[1].data_ptr() % 4 == 2
    seeds, vals = _seeds(40, seed=82)
    specs = [codec.ParamSpec(t, lr=1e-3, weight_decay=wd) for t in ts]
    codec.directional_step(specs, seeds, vals)
    torch.cuda.synchronize()
    n = len(shapes)
    O.reconstruct(arrays, [O.BF16] * n, [1e-3] * n, [wd] * n, seeds, vals)
    for i, (t, a) in enumerate(zip(ts, arrays)):
        assert_bitwise(to_np(t), a, "bfloat16", f"wd {wd} tensor {i}")
    s = to_np(store)
    assert s[0] == 0x3F80 and np.array_equal(s[1 + shapes[1]:], guard)


def test_task_path_many_tasks_per_wave():
    """2^20 + 624*48 + 32 elements are 1,729 MT blocks, 6 or 7 per chunk of a two-slice pass
    (about 33 tasks, 5 or 6 per wave): the carried row wraps several times in every wave, the
    last task of a chunk is partial (lanes past the chunk's end on carried rows), and the
    second tensor's segment begins inside a task.  K = 70: a full pass and a 6-seed one."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    shapes = [1 << 20, 624 * 48 + 32]
    arrays = rand_params(shapes, "bfloat16", seed=91)
    seeds, vals = _seeds(70, seed=92)
    ts = [from_np(a, "bfloat16", dev) for a in arrays]
    specs = [codec.ParamSpec(t, lr=1e-5, weight_decay=0.0) for t in ts]
    codec.directional_step(specs, seeds, vals)
    torch.cuda.synchronize()
    O.reconstruct(arrays, [O.BF16] * 2, [1e-5] * 2, [0.0] * 2, seeds, vals)
    for i, (t, a) in enumerate(zip(ts, arrays)):
        assert_bitwise(to_np(t), a, "bfloat16", f"tensor {i}")


@pytest.mark.parametrize("wd", [0.0, -0.0])
def test_task_path_edge_values(wd):
    """K = 40 on parameters of +-0, +-inf, NaN, denormals and 3e38 with directional values
    -1e-45, 1e-45, -3e38 and 1e30 among ordinary ones.  A 16-bit load that left the register's
    low half non-zero, or a store of the wrong half, shows in these bits; so does the g of the
    wrong half of an SGPR pair (the special values sit on odd and even seeds)."""
    n = 64 * 1024
    base = rand_params([n], "bfloat16", seed=15)[0]
    f = as_float(base, "bfloat16").astype(np.float32)
    f[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-39, 3e38]
    f[8:16] = np.float32(-1.2e-38) * np.arange(8, dtype=np.float32)
    f[5000:5016] = -0.0
    f[7000:7016] = 0.0
    arr = to_np(torch.from_numpy(f).to(torch.bfloat16))
    seeds, vals = _seeds(40, seed=67)
    for i, e in enumerate([-1e-45, 1e-45, -3e38, -5.0, 1e30, -0.5], start=1):  # seed 0 keeps an ordinary value
        vals[i] = e
    got = _gpu_reconstruct([arr], "bfloat16", [1e-2], [wd], seeds, vals)
    O.reconstruct([arr], [O.BF16], [1e-2], [wd], seeds, vals)
    assert_bitwise(got[0], arr, "bfloat16", f"wd {wd}")
    assert not np.array_equal(got[0][16:4096], base[16:4096])


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_task_path_element_shards(wd):
    """Three element shards whose starts are not task-aligned: their union equals the oracle's
    whole reconstruct (a shard's first and last task are partly off its segment, so their
    lanes read and write the sink at both 16-bit offsets)."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    shapes = [2**17, 624 * 40, 48]
    arrays = rand_params(shapes, "bfloat16", seed=16)
    seeds, vals = _seeds(50, seed=17)
    ts = [from_np(a, "bfloat16", dev) for a in arrays]
    specs = [codec.ParamSpec(t, lr=1e-3, weight_decay=wd) for t in ts]
    for r in range(3):
        codec.directional_step(specs, seeds, vals, shard=r, nshards=3)
    torch.cuda.synchronize()
    n = len(shapes)
    O.reconstruct(arrays, [O.BF16] * n, [1e-3] * n, [wd] * n, seeds, vals)
    for i, (t, a) in enumerate(zip(ts, arrays)):
        assert_bitwise(to_np(t), a, "bfloat16", f"wd {wd} tensor {i}")
