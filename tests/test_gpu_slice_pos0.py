"""GPU parity of the bf16 slice kernel's fma-free zero-weight-decay chain (kModeUpdateWdPos0 of
fks_apply_bs_kernel): the host takes it when every bf16 fast segment has wd = +0.0 exactly and a
finite lr and the call's directional values keep |lr g z| <= 1e30 (gmax * 6.67 <= 1e37 and
gmax * 6.67 * max_lr <= 1e30); anything else, and FKS_BS_KEEP_WD_FMA=1, keeps the fma form
(kModeUpdateWd0).  Both forms must give the oracle's bits, so every case runs with and without
FKS_BS_KEEP_WD_FMA=1.

Bar: bit-exact against the CPU oracle (assert_bitwise), the helpers of test_gpu_slice.py and
test_gpu_slice_lookup_paths.py reused.  The oracle's result of a case is computed once and shared
by the runs of that case; the arrays it returns are read only.

A note on the edge-value preconditions.  A -0.0 parameter stays -0.0 through a seed only where
that seed's g z is +0 (p - lr t with t = -0 + g z), and once it is +0.0 or nonzero it never
returns.  With g = +-1e-45 (g z rounds to a zero of the product's sign) that is one chance in two
per seed and element, so among 4,096 elements one that is still -0.0 after all K >= 20 seeds has
probability below 4096 * 0.504^20 = 5e-3 (1e-9 at K = 40): no choice of seeds reaches it.  The
test asserts what can hold: every planted +-inf ends as NaN, among the -0.0 inputs at least one
ends +0.0 after the K seeds, and -- on a one-seed oracle run of the call's first seed -- at least
one is still -0.0 and at least one is +0.0 after that seed, so both signs of zero enter the rest
of the chain.  For the zeros to stay zeros at all, the "tiny" value set has one ordinary
(negative) value and +-1e-45 everywhere else; the "mixed" set has ordinary, negative, large and
1e-45 values and only the inf -> NaN precondition.
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


def _keep(monkeypatch, keep, slices=None):
    for name, v in (("FKS_BS_KEEP_WD_FMA", keep), ("FKS_BS_SLICES", slices)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def _run(init, dts, lrs, wds, seeds, vals, shards=1):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    ts = [from_np(a, d, dev) for a, d in zip(init, dts)]
    specs = [codec.ParamSpec(t, lr=lr, weight_decay=wd) for t, lr, wd in zip(ts, lrs, wds)]
    if shards == 1:
        codec.directional_step(specs, list(seeds), list(vals))
    else:
        for r in range(shards):
            codec.directional_step(specs, list(seeds), list(vals), shard=r, nshards=shards)
    torch.cuda.synchronize()
    return [to_np(t) for t in ts]


def _oracle(init, dts, lrs, wds, seeds, vals):
    want = [a.copy() for a in init]
    O.reconstruct(want, [DTC[d] for d in dts], lrs, wds, seeds, vals)
    return want


def _check(got, want, dts, what):
    for i, (a, b, d) in enumerate(zip(got, want, dts)):
        assert_bitwise(a, b, d, f"{what} tensor {i}")


# ----------------------------------------------------------------------------- the bound's edges
EDGE_SHAPES = [16, 48, 2**16]
EDGE_LR = 1e-3


def _bound_g(above):
    """The largest f32 g with g * 6.67 * f32(lr) <= 1e30 in the host's double arithmetic, or the
    next f32 above it."""
    lr = float(np.float32(EDGE_LR))
    g = np.float32(1e30 / (6.67 * lr))
    while float(g) * 6.67 * lr > 1e30:
        g = np.nextafter(g, np.float32(0))
    while float(np.nextafter(g, np.float32(np.inf))) * 6.67 * lr <= 1e30:
        g = np.nextafter(g, np.float32(np.inf))
    assert float(g) * 6.67 * lr <= 1e30 < float(np.nextafter(g, np.float32(np.inf))) * 6.67 * lr
    return float(np.nextafter(g, np.float32(np.inf)) if above else g)


EDGE_CASES = {
    # name: (dtypes, wds, the value planted at seed 5 or None)
    "ordinary": (["bfloat16"] * 3, [0.0] * 3, None),
    "bound_below": (["bfloat16"] * 3, [0.0] * 3, ("g", False)),
    "bound_above": (["bfloat16"] * 3, [0.0] * 3, ("g", True)),
    "g_inf": (["bfloat16"] * 3, [0.0] * 3, float("inf")),
    "g_nan": (["bfloat16"] * 3, [0.0] * 3, float("nan")),
    "wd_neg0": (["bfloat16"] * 3, [-0.0] * 3, None),
    "wd_pos0_and_neg0": (["bfloat16"] * 3, [0.0, -0.0, 0.0], None),
    "bf16_beside_f32": (["bfloat16", "float32", "bfloat16"], [0.0] * 3, None),
}


@functools.lru_cache(maxsize=None)
def _edge_case(name):
    dts, wds, plant = EDGE_CASES[name]
    init = [rand_params([n], d, seed=500 + i)[0] for i, (n, d) in enumerate(zip(EDGE_SHAPES, dts))]
    seeds, vals = _seeds(40, seed=510)
    if plant is not None:
        vals[5] = _bound_g(plant[1]) if isinstance(plant, tuple) else plant
    lrs = [EDGE_LR] * 3
    return init, dts, lrs, wds, seeds, vals, _oracle(init, dts, lrs, wds, seeds, vals)


@pytest.mark.parametrize("keep", KEEP)
@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_pos0_bound_edges(monkeypatch, name, keep):
    _keep(monkeypatch, keep)
    init, dts, lrs, wds, seeds, vals, want = _edge_case(name)
    _check(_run(init, dts, lrs, wds, seeds, vals), want, dts, f"{name} keep={keep}")


# ----------------------------------------------------------------------------- edge values
N_EDGE = 2**16
INF_AT = (2, 3, 20000, 40001)
NEG0 = slice(8192, 8192 + 4096)


def _edge_values_init():
    base = rand_params([N_EDGE], "bfloat16", seed=5)[0]
    f = as_float(base, "bfloat16").astype(np.float32)
    f[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-39, 3.3895314e38]
    f[8:16] = np.float32(-1.2e-38) * np.arange(8, dtype=np.float32)
    f[16:24] = [-3.3895314e38, 9.2e-41, -9.2e-41, 0.0, -0.0, 1.0, -1.0, 2e-38]
    f[20000], f[40001] = np.inf, -np.inf
    f[NEG0] = -0.0
    f[7000:7016] = 0.0
    return to_np(torch.from_numpy(f).to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _edge_values_case(k, gset):
    init = [_edge_values_init()]
    seeds, vals = _seeds(k, seed=600 + k)
    if gset == "tiny":  # zeros stay zeros but for seed 1: +-1e-45 everywhere else
        sign = np.random.default_rng(k).integers(0, 2, k) * 2 - 1
        vals = [float(s) * 1e-45 for s in sign]
        vals[0] = 1e-45
        vals[1] = -5.0
    else:  # inside the bound for lr = 1e-2: |g| <= 1.4e31
        for i, e in enumerate([-1e-45, 1e-45, -3e30, -5.0, 1e30, -0.5], start=1):
            vals[i] = e
    lrs, wds, dts = [1e-2], [0.0], ["bfloat16"]
    want = _oracle(init, dts, lrs, wds, seeds, vals)
    first = _oracle(init, dts, lrs, wds, seeds[:1], vals[:1])
    return init, dts, lrs, wds, seeds, vals, want, first


@pytest.mark.parametrize("keep", KEEP)
@pytest.mark.parametrize("gset", ["tiny", "mixed"])
@pytest.mark.parametrize("k", [20, 40, 64, 70])
def test_pos0_edge_values(monkeypatch, k, gset, keep):
    init, dts, lrs, wds, seeds, vals, want, first = _edge_values_case(k, gset)
    # preconditions, on the oracle's output alone and before anything runs on the GPU
    w = want[0]
    assert np.isnan(as_float(w, "bfloat16")[list(INF_AT)]).all(), "a planted inf did not end as NaN"
    if gset == "tiny":
        assert (init[0][NEG0] == 0x8000).all()
        assert (w[NEG0] == 0x0000).any(), "no -0.0 input ends +0.0"
        f1 = first[0][NEG0]
        assert (f1 == 0x8000).any() and (f1 == 0x0000).any(), "the first seed does not leave both zeros"
    _keep(monkeypatch, keep)
    _check(_run(init, dts, lrs, wds, seeds, vals), want, dts, f"K={k} {gset} keep={keep}")
    if gset == "mixed":
        assert not np.array_equal(w[4096:8192], init[0][4096:8192])


# ----------------------------------------------------------------------------- partial slices
PART_SHAPES = [16, 48, 624 * 16 + 32, 2**16, 4096 * 3 + 5]


@functools.lru_cache(maxsize=None)
def _part_case(k):
    init = rand_params(PART_SHAPES, "bfloat16", seed=700 + k)
    seeds, vals = _seeds(k, seed=800 + k)
    n = len(PART_SHAPES)
    dts, lrs, wds = ["bfloat16"] * n, [1e-3] * n, [0.0] * n
    return init, dts, lrs, wds, seeds, vals, _oracle(init, dts, lrs, wds, seeds, vals)


@pytest.mark.parametrize("keep", KEEP)
@pytest.mark.parametrize("slices", [None, "1"])
@pytest.mark.parametrize("k", [20, 33, 35, 47, 64, 65, 66, 67, 87])
def test_pos0_partial_slices(monkeypatch, k, slices, keep):
    """Halves of 1, 2, 3, 16..24 and 32 seeds: partial and full passes of both forms."""
    _keep(monkeypatch, keep, slices)
    init, dts, lrs, wds, seeds, vals, want = _part_case(k)
    _check(_run(init, dts, lrs, wds, seeds, vals), want, dts, f"K={k} slices={slices} keep={keep}")


# ----------------------------------------------------------------------------- many tasks per wave
@functools.lru_cache(maxsize=None)
def _long_case(which):
    if which == "multiblock":  # 1,729 MT blocks: many tasks per wave, several row wraps
        shapes, k, lr = [2**20, 624 * 48 + 32], 70, 1e-5
    else:  # three element shards whose chunks start off the task grid
        shapes, k, lr = [2**17, 624 * 40], 50, 1e-3
    init = rand_params(shapes, "bfloat16", seed=900 + k)
    seeds, vals = _seeds(k, seed=910 + k)
    dts, lrs, wds = ["bfloat16"] * 2, [lr] * 2, [0.0] * 2
    return init, dts, lrs, wds, seeds, vals, _oracle(init, dts, lrs, wds, seeds, vals)


@pytest.mark.parametrize("keep", KEEP)
@pytest.mark.parametrize("which", ["multiblock", "shards"])
def test_pos0_many_tasks(monkeypatch, which, keep):
    _keep(monkeypatch, keep)
    init, dts, lrs, wds, seeds, vals, want = _long_case(which)
    got = _run(init, dts, lrs, wds, seeds, vals, shards=3 if which == "shards" else 1)
    _check(got, want, dts, f"{which} keep={keep}")
