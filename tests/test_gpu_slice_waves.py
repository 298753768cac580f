"""GPU parity of the bf16 slice kernel where its wave count enters (fks_apply_bs_kernel<MODE, FULL, W>,
W waves per half: the task stride, the row step W * 128 mod 624, the progress words, the block size).
The count is a compile-time choice of the library (FKS_BS_WAVES_POS0 for the fma-free wd +0 chain, 6
for every other chain), so the cases run on the library as built and are chosen to hold for W = 6, 7
and 8 alike.

Bar: bit-exact against the CPU oracle (assert_bitwise), obtained as test_gpu_slice_pos0.py obtains it;
every case at wd = +0.0 with a finite lr, with and without FKS_BS_KEEP_WD_FMA=1 (the six-wave fma form
beside the fma-free one).  The oracle's result of a case is computed once and shared; it is read only.

Tasks per half.  The plan gives a workgroup whole 624-word MT blocks (fks_layout.cpp: bs_nchunks(),
chunk_table()), and a task is 128 words, so a half of b blocks has ceil(4.875 b) tasks: 0, 5, 10, 15,
20, 25, 30, 35, 39, ...  The counts W, W + 1 and -- but for 15 -- 2 W - 1 and 2 W + 1 of W = 6, 7, 8
are not among them and no layout reaches them.  What those counts stand for is reached, and
_plan_tasks() asserts it from the device's CU count before anything runs:
  *  0 and 5 tasks: waves that never get a task (5 < W for every W), and an empty half (split, "small");
  * 10 tasks: the first 10 - W waves run two tasks and leave the unrolled-by-two loop from its second
    slot, the others run one and leave from the first (W = 6: 4 and 2 waves, 7: 3 and 4, 8: 2 and 6);
  * 15 tasks: 2 W + 1 for W = 7, 2 W - 1 for W = 8, and for W = 6 three tasks in waves 0..2 (the loop
    goes round once and leaves from the first slot);
  * 20 tasks: three and two tasks per wave for W = 7 and 8, four and three for W = 6;
  * 39 tasks: several rounds of the loop, the row step wrapping past 624 more than once.
A half's last task has 112 words (odd b), 64 (b = 4) or exactly 128 (b = 8: 39 tasks).

Layouts (the stream is the tensors back to back, each a multiple of 16 elements: all fast segments):
  * "small", 3 blocks: a tensor boundary on a task boundary (word 384) and one inside a task (592);
  * "mid", 3 blocks per CU: a 4,096-element tensor between two large ones, holding +-0, +-inf, NaN and
    bf16 subnormals (the fma-free chain's fma(0, p, p) is per task, and the task-to-wave map moves);
  * "long", 8 blocks per CU.
K: 64 (FULL, two slices), 65 (a full pass and a one-seed split pass), 33 (partial two-slice, 17 + 16),
32 (FULL split), 23 (partial split), 20 (the smallest call that takes the slice kernel).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fks_oracle as O
from test_gpu_parity import DTC, _dev, from_np, rand_params, to_np
from test_gpu_slice import _seeds
from conftest import as_float, assert_bitwise

pytestmark = pytest.mark.gpu

KEEP = [None, "1"]
KS = [64, 65, 33, 32, 23, 20]
MT_N, TASK = 624, 128
LR = 1e-3
EDGE_INF_AT = (2, 3, 1000, 4001)


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


def _shapes(name, cus):
    if name == "small":  # 1,856 words: 3 blocks
        return [384, 208, 1264]
    if name == "mid":  # 3 blocks per CU, a 4,096-element tensor between two large ones
        total = 3 * cus * MT_N
        first = (total * 5 // 12) // 16 * 16
        return [first, 4096, total - first - 4096]
    assert name == "long"  # 8 blocks per CU
    total = 8 * cus * MT_N
    return [total // 2 // 16 * 16 + 16 * 37, total - (total // 2 // 16 * 16 + 16 * 37)]


def _plan_tasks(nwords, cus, split):
    """Tasks per half of every workgroup, as fks_layout.cpp cuts the stream (bs_nchunks, chunk_table)."""
    nb = max(1, -(-nwords // MT_N))
    wgs = max(1, min(cus, (nb + 1) // 2))
    cb = [nb * c // (2 * wgs) for c in range(2 * wgs + 1)]
    step = 1 if split else 2
    return {-(-MT_N * (cb[c + step] - cb[c]) // TASK) for c in range(0, 2 * wgs, step)}


def _edge_tensor():
    base = rand_params([4096], "bfloat16", seed=41)[0]
    f = as_float(base, "bfloat16").astype(np.float32)
    f[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-39, 3.3895314e38]
    f[8:16] = np.float32(-1.2e-38) * np.arange(8, dtype=np.float32)
    f[16:24] = [-3.3895314e38, 9.2e-41, -9.2e-41, 0.0, -0.0, 1.0, -1.0, 2e-38]
    f[1000], f[4001] = np.inf, -np.inf
    f[2048:2048 + 256] = -0.0
    f[3000:3016] = 0.0
    return to_np(torch.from_numpy(f).to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _init(name, cus):
    shapes = _shapes(name, cus)
    assert all(n % 16 == 0 for n in shapes)
    init = rand_params(shapes, "bfloat16", seed=1700 + len(name))
    if name == "mid":
        init[1] = _edge_tensor()
    return shapes, init


@functools.lru_cache(maxsize=None)
def _case(name, k, cus):
    shapes, init = _init(name, cus)
    seeds, vals = _seeds(k, seed=1710 + k)
    n = len(shapes)
    dts, lrs, wds = ["bfloat16"] * n, [LR] * n, [0.0] * n
    want = [a.copy() for a in init]
    O.reconstruct(want, [DTC[d] for d in dts], lrs, wds, seeds, vals)
    return init, dts, lrs, wds, seeds, vals, want


def _keep(monkeypatch, keep):
    monkeypatch.delenv("FKS_BS_SLICES", raising=False)
    if keep is None:
        monkeypatch.delenv("FKS_BS_KEEP_WD_FMA", raising=False)
    else:
        monkeypatch.setenv("FKS_BS_KEEP_WD_FMA", keep)


def _run(init, dts, lrs, wds, seeds, vals, shards=()):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    ts = [from_np(a, d, dev) for a, d in zip(init, dts)]
    specs = [codec.ParamSpec(t, lr=lr, weight_decay=wd) for t, lr, wd in zip(ts, lrs, wds)]
    if not shards:
        codec.directional_step(specs, list(seeds), list(vals))
    for r, n in shards:
        codec.directional_step(specs, list(seeds), list(vals), shard=r, nshards=n)
    torch.cuda.synchronize()
    return [to_np(t) for t in ts]


def _check(got, want, dts, what):
    for i, (a, b, d) in enumerate(zip(got, want, dts)):
        assert_bitwise(a, b, d, f"{what} tensor {i}")


# the task counts a layout must produce, two-slice passes and split passes
WANT_TASKS = {
    "small": ({5, 10}, {0, 5}),
    "mid": ({15}, {5, 10}),
    "long": ({39}, {20}),
}


@pytest.mark.parametrize("name", list(WANT_TASKS))
def test_waves_layouts_give_the_task_counts(name):
    cus = _cus()
    nwords = sum(_shapes(name, cus))
    two, split = WANT_TASKS[name]
    assert _plan_tasks(nwords, cus, split=False) == two
    assert _plan_tasks(nwords, cus, split=True) == split
    if name == "small":  # a tensor boundary on a task boundary and one inside a task
        s = _shapes(name, cus)
        assert s[0] % TASK == 0 and (s[0] + s[1]) % TASK != 0
    if name == "long":  # a last task of exactly 128 words; "small" and "mid" end on 112
        assert (8 * MT_N) % TASK == 0 and MT_N % TASK == 112


@pytest.mark.parametrize("keep", KEEP)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["small", "mid"])
def test_waves_task_counts(monkeypatch, name, k, keep):
    init, dts, lrs, wds, seeds, vals, want = _case(name, k, _cus())
    if name == "mid":  # the edge values: every planted inf ends as NaN, in the oracle already
        assert np.isnan(as_float(want[1], "bfloat16")[list(EDGE_INF_AT)]).all()
    _keep(monkeypatch, keep)
    _check(_run(init, dts, lrs, wds, seeds, vals), want, dts, f"{name} K={k} keep={keep}")
    assert not np.array_equal(want[0], init[0])


@pytest.mark.parametrize("keep", KEEP)
@pytest.mark.parametrize("k", [64, 32])
def test_waves_many_tasks(monkeypatch, k, keep):
    """39 tasks per half (two slices) and 20 (split): several rounds of the task loop."""
    init, dts, lrs, wds, seeds, vals, want = _case("long", k, _cus())
    _keep(monkeypatch, keep)
    _check(_run(init, dts, lrs, wds, seeds, vals), want, dts, f"long K={k} keep={keep}")


@pytest.mark.parametrize("keep", KEEP)
def test_waves_element_shards(monkeypatch, keep):
    """Shard 1 of 3 alone touches its blocks' words only and gives the oracle's bits there; the three
    shards together give the whole call's result: independent of the chunk plan."""
    cus = _cus()
    init, dts, lrs, wds, seeds, vals, want = _case("mid", 33, cus)
    _keep(monkeypatch, keep)
    nb = -(-sum(a.size for a in init) // MT_N)
    lo, hi = MT_N * (nb * 1 // 3), MT_N * (nb * 2 // 3)  # shard_blocks(): whole blocks
    pos = np.arange(sum(a.size for a in init))
    mine = (pos >= lo) & (pos < hi)
    assert mine.any() and not mine.all()
    expect, off = [], 0
    for a, w in zip(init, want):
        expect.append(np.where(mine[off:off + a.size], w, a))
        off += a.size
    _check(_run(init, dts, lrs, wds, seeds, vals, shards=[(1, 3)]), expect, dts, f"shard 1 of 3 keep={keep}")
    got = _run(init, dts, lrs, wds, seeds, vals, shards=[(0, 3), (1, 3), (2, 3)])
    _check(got, want, dts, f"union of 3 shards keep={keep}")
