"""fks_expand_mt_multi (codec.expand_mt_multi) over the lists of tests/mt_layouts.py, against the
reference of tests/test_gpu_expand_mt.py: torch's CPU draws per tensor in the tensor's dtype (frozen
ones drawn and dropped), widened to f32 and folded by tests/exact_f32.py -- chain32 from +0,
fma32(f32(beta), widen(old), acc) where beta != 0, torch's cast.  Every comparison is bitwise on every
live element; guards, frozen and empty tensors' buffers keep their sentinel
(tests/test_gpu_expand_exact.py's buffers and row check).  tests/test_mt_layouts_host.py asserts, from
a mirror of the layout, that the lists hold what is said here.

  G (G:bfloat16, G:float32, G:float16, G:mixed; 15,088 elements, 25 MT blocks): the fast kernel's
    segment lookup -- three fast segments inside MT block 0 (`while (s1 >= seg_end)` advancing more
    than one segment in a step), block 1 wholly inside a frozen gap (a chunk whose first word lies
    in a gap: the binary search lands on a later segment; lanes before the next segment), fast
    segments after tiny groups, after a ragged pair and after the gap (the fast kernel after
    irregular work).  G:mixed: the per-dtype offset into the table row, one dtype's launch seeing
    the other's segments as gaps, the table's row order with two non-empty dtypes.  Shards of one
    MT block each, and more shards than blocks: cuts in the gap, in tiny groups and in runs, shards
    that own nothing.
  R (800 tensors, 1,132,000 elements, 1,816 MT blocks, 1,200 table entries): more blocks than plan
    chunks, so a workgroup walks several blocks and the lookahead fetch(b + 1) crosses from a
    segment into a gap, into the next segment and over the other dtype's stretches; segment starts
    at every 16-aligned phase of the block; the largest table; K = 38, whose last pass is the
    last-full instance; the staging split; two calls in flight on two streams, each uploading its
    table from the host vector the next call reassigns.
  sweep (32 seeded cases): pass shapes (K = 18, 19, 37, 38, 57 and one of 20 .. 56), output dtypes
    per tensor, betas, alignment and shard counts drawn per case over layouts with gaps, several
    segments in a block, both dtypes' segments, odd-phase runs and tiny elements; more distinct
    spec lists than the plan cache holds, so it evicts while earlier calls are still queued."""
import functools

import numpy as np
import pytest
import torch

import mt_layouts as ML
from exact_f32 import chain32, fma32
from test_gpu_expand import _coefs, _same
from test_gpu_expand_exact import _List, _buffers, _check_row
from test_gpu_expand_mt import SEEDS57 as SEEDS
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

ROWS = ["float32", "bfloat16", "float16"]  # output dtypes
BETAS = [0.0, -0.0, 0.3, 1.0, -1.7]
KMAX = len(SEEDS)


_get = ML.get


@functools.lru_cache(maxsize=None)
def _L(name):
    lst = _get(name)
    return _List(lst.sizes, lst.dts, frozen=lst.frozen)


@functools.lru_cache(maxsize=None)
def _specs(name):
    """one spec list per list, kept for the session (a stable plan key)"""
    return tuple(_L(name).specs(_dev()))


_ZS = {}


def _zs(name, k):
    """the first k seeds' reference draws over the list, on the device; drawn once, shared, never
    written to"""
    have = _ZS.setdefault(name, [])
    for z in ML.zs(name, SEEDS[:k])[len(have):]:
        have.append(z.to(_dev()))
    return have[:k]


def _row(row, scale=1.0):
    return _coefs(KMAX, row, scale)


@functools.lru_cache(maxsize=None)
def _chain(name, row, k, scale=1.0):
    """the exact f32 sums of coefficient row `row` over the first k seeds"""
    return _chain_of(name, tuple(_row(row, scale)[:k]))


def _chain_of(name, coefs):
    if not coefs:
        return torch.zeros(_L(name).off[-1], dtype=torch.float32, device=_dev())
    return chain32(coefs, _zs(name, len(coefs)))


def _names(L, m=0):
    """output dtypes rotating over the tensors of a row"""
    return [ROWS[(i + m) % 3] for i in range(len(L.sizes))]


def _what(name, k):
    lst = _get(name)
    return f"list {name}, sizes {list(lst.sizes)}, dtypes {list(lst.dts)}, frozen {list(lst.frozen)}, K {k}"


def _run(name, rows, row_names, betas=None, offset=0, k=20, scale=1.0, coefs=None, nshards=1, **kw):
    """One expand_mt_multi call (one per shard with nshards > 1: ownership is disjoint, so every
    element still takes its beta once) on fresh buffers, synchronized, every row checked against the
    exact reference; returns the views per row."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _L(name)
    M = len(rows)
    bs = [0.0] * M if betas is None else list(betas)
    made = [_buffers(L, row_names[m], bs[m], offset, dev, 900 + 100 * m) for m in range(M)]
    cs = [_row(r, scale)[:k] for r in rows] if coefs is None else coefs
    for sh in range(nshards):
        codec.expand_mt_multi(_specs(name), SEEDS[:k], cs, [v for _, v, _ in made], betas=betas, shard=sh,
                              nshards=nshards, **kw)
    torch.cuda.synchronize()
    for m in range(M):
        acc = _chain(name, rows[m], k, scale) if coefs is None else _chain_of(name, tuple(cs[m]))
        _check_row(L, row_names[m], bs[m], acc, *made[m], what=f"{_what(name, k)}, shards {nshards}, row {m}")
    return [v for _, v, _ in made]


# ---- 1. the G lists: every pass shape's instance over gaps, several segments a block, mixed dtypes
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("k", [1, 19, 20, 38])
@pytest.mark.parametrize("name", ML.G_NAMES)
def test_G_lists(name, k, offset):
    """Three outputs whose dtypes rotate over the tensors; betas 0 (NaN-filled, never read), 0.3
    and 1 rotating with K; outputs 16-byte aligned, and one element off."""
    L = _L(name)
    r = [1, 19, 20, 38].index(k)
    betas = [(0.0, 0.3, 1.0)[(m + r) % 3] for m in range(3)]
    got = _run(name, [200, 201, 202], [_names(L, m) for m in range(3)], betas=betas, offset=offset, k=k)
    for m in range(3):
        if betas[m] == 0:
            assert all(bool(torch.isfinite(got[m][i]).all()) for i in L.live), m


# ---- 2. the R list: blocks walked by one workgroup, a 1,200-entry table, the last-full instance
def test_R_list():
    """K = 38 (first + last full): a bf16 row with beta 0.3 and an f32 row with beta 0, which also
    equals codec.delta_accumulate on a zeroed buffer."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _L("R")
    got = _run("R", [203, 204], ["bfloat16", "float32"], betas=[0.3, 0.0], k=38)
    delta = torch.zeros(L.off[-1], dtype=torch.float32, device=dev)
    codec.delta_accumulate(_specs("R"), SEEDS[:38], _row(204)[:38], delta, stream_mode="torch_cpu")
    torch.cuda.synchronize()
    for i in L.live:
        assert _same(got[1][i], delta[L.off[i]:L.off[i + 1]]), i


# ---- 3. the sweep
@pytest.mark.parametrize("case", range(ML.SWEEP))
def test_sweep(case):
    name = f"sweep{case}"
    L = _L(name)
    g = np.random.default_rng(9500 + case)
    k = int(g.choice([18, 19, 37, 38, 57, int(g.integers(20, 57))]))
    M = int(g.integers(1, 3))
    names = [[ROWS[int(x)] for x in g.integers(0, 3, len(L.sizes))] for _ in range(M)]
    betas = [BETAS[int(g.integers(0, len(BETAS)))] for _ in range(M)]
    offset = int(g.integers(0, 2))
    nshards = int(g.choice([1, 1, 2, 3]))
    _run(name, [210 + m for m in range(M)], names, betas=betas, offset=offset, k=k, nshards=nshards)


# ---- 4. shards of one MT block, and shards that own nothing
@pytest.mark.parametrize("nshards", [5, 25, 32])
@pytest.mark.parametrize("name", ["G:bfloat16", "G:mixed"])
def test_shards_on_G(name, nshards):
    """tests/test_gpu_expand_mt.py's shard scheme: every shard on sentinel-filled outputs of its
    own -- what it writes is the whole call's element, every live element is written by exactly one
    shard -- and on one shared bf16 output with beta 1 over the sentinel.  At 25 every shard is one
    MT block (the cuts fall in the frozen gap, in tiny groups and in runs; block 1 owns nothing);
    at 32 seven shards hold no block at all: they return without error and write nothing."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _L(name)
    k = 20
    coefs = [_row(220)[:k]]
    sent = 1.0e9  # far outside any sum of 20 N(0, 1) coefficients times |z| <= 7

    def fresh(d=torch.float32):
        return [torch.full((n,), sent, dtype=d, device=dev) for n in L.sizes]

    whole = fresh()
    codec.expand_mt_multi(_specs(name), SEEDS[:k], coefs, [whole])
    count = [torch.zeros(n, dtype=torch.int32, device=dev) for n in L.sizes]
    union = fresh(torch.bfloat16)
    idle = 0
    for sh in range(nshards):
        part = fresh()
        codec.expand_mt_multi(_specs(name), SEEDS[:k], coefs, [part], shard=sh, nshards=nshards)
        codec.expand_mt_multi(_specs(name), SEEDS[:k], coefs, [union], betas=[1.0], shard=sh, nshards=nshards)
        torch.cuda.synchronize()
        wrote_any = False
        for i in range(len(L.sizes)):
            wrote = part[i] != sent
            wrote_any |= bool(wrote.any())
            count[i] += wrote.int()
            assert _same(torch.where(wrote, part[i], whole[i]), whole[i]), (sh, i)
        assert any(bool((part[i] == sent).any()) for i in L.live), sh  # a shard is not the whole call
        idle += not wrote_any
    assert idle >= {5: 0, 25: 1, 32: 8}[nshards]  # the block inside the frozen gap, and 32 - 25 shards without a block
    acc = _chain(name, 220, k)
    for i in range(len(L.sizes)):
        if i in L.live:
            assert bool((count[i] == 1).all()), i
            a = acc[L.off[i]:L.off[i + 1]]
            assert _same(whole[i], a), i
            assert _same(union[i], fma32(1.0, torch.full_like(a, sent).bfloat16().float(), a).bfloat16()), i
        else:
            assert not bool(count[i].any()), i


# ---- 5. the internal split
def test_small_staging_budget_splits_the_R_call():
    """K = 38 under a staging budget that two shards' larger half does not fit, so at least three
    internal shards: the unsplit call's bits (both equal the reference)."""
    from fate_llm.algo.fedkseed import codec
    b = codec._Batch(list(_specs("R")), "torch_cpu", stage=False)
    two = max(st for _, st in codec._expand_mt_sizes(b, 38, 1, 2))
    three = max(st for _, st in codec._expand_mt_sizes(b, 38, 1, 3))
    assert 0 < three < two
    one = _run("R", [221], ["bfloat16"], betas=[0.3], k=38)
    split = _run("R", [221], ["bfloat16"], betas=[0.3], k=38, staging_bytes=two - 1)
    for i in _L("R").live:
        assert _same(split[0][i], one[0][i]), i


# ---- 6. two calls in flight
def test_two_calls_in_flight_on_two_streams():
    """Two side streams, each with outputs of its own, each given an R-list call (K = 20, its own
    coefficients) with no host synchronisation in between, then a G-list call on the first stream:
    every call uploads its table from a host vector that the next call reassigns.  After both
    streams have finished, all three results equal their references."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    k = 20
    plan = [("R", 222, "float32"), ("R", 223, "bfloat16"), ("G:mixed", 224, "float32")]
    refs = [_chain(name, row, k) for name, row, _ in plan]
    outs = [[torch.full((n,), float("nan"), dtype=ML.DT[d], device=dev) for n in _L(name).sizes] for name, _, d in plan]
    specs = [_specs(name) for name, _, _ in plan]
    coefs = [_row(row)[:k] for _, row, _ in plan]
    torch.cuda.synchronize()
    sides = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    for j, s in ((0, 0), (1, 1), (2, 0)):
        with torch.cuda.stream(sides[s]):
            codec.expand_mt_multi(specs[j], SEEDS[:k], [coefs[j]], [outs[j]])
    for s in sides:
        s.synchronize()
    for j, (name, _, d) in enumerate(plan):
        L = _L(name)
        for i in L.live:
            assert _same(outs[j][i], refs[j][L.off[i]:L.off[i + 1]].to(ML.DT[d])), (j, i)


# ---- 7. f32 subnormals
@pytest.mark.parametrize("kind", ["sums", "coefficients"])
def test_subnormals(kind):
    """Coefficients of about 2^-140 make every sum an f32 subnormal; coefficients 2^-149 j, j a small
    integer, are subnormal themselves.  A kernel that flushed either would differ from this
    reference (this compilation unit is not the one where the torch_rocm stream tests it)."""
    k = 20
    if kind == "sums":
        coefs = [_row(225 + m, 2.0 ** -140)[:k] for m in range(2)]
    else:
        coefs = [[(-1) ** (j + m) * (j % 7 + 1) * (1 if j % 2 else 2 ** 17) * 2.0 ** -149 for j in range(k)]
                 for m in range(2)]
        assert all(0 < abs(c) < 2.0 ** -126 for row in coefs for c in row)
    ref = _chain_of("G:mixed", tuple(coefs[0]))
    sub = (ref != 0) & (ref.abs() < 2.0 ** -126)
    assert int(sub.sum()) > ref.numel() // 2  # the reference holds non-zero subnormal f32 sums
    _run("G:mixed", [None, None], ["float32", "bfloat16"], k=k, coefs=coefs)


# ---- 8. the other fp32 flavour
F32_SWEEPS = [c for c in range(ML.SWEEP)
              if any(d == "float32" and n and i not in ML.sweep(c).frozen
                     for i, (n, d) in enumerate(zip(ML.sweep(c).sizes, ML.sweep(c).dts)))]


@pytest.mark.parametrize("name", ["G:float32"] + [f"sweep{c}" for c in F32_SWEEPS])
def test_other_fp32_flavour_equals_delta_accumulate(name):
    """The fp32 flavour that is not this process's (no torch draw of it exists here): the f32 output
    with beta 0 equals fks_delta_accumulate under the same setting, bit for bit."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _L(name)
    k = 38 if name.startswith("G") else 20
    here = codec.cpu_fp32_flavour()
    coefs = _row(230)[:k]
    outs = [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in L.sizes]
    delta = torch.zeros(L.off[-1], dtype=torch.float32, device=dev)
    codec.set_cpu_fp32_flavour("libm" if here == "avx" else "avx")
    try:
        assert codec.cpu_fp32_flavour() != here
        codec.expand_mt_multi(_specs(name), SEEDS[:k], [coefs], [outs])
        codec.delta_accumulate(_specs(name), SEEDS[:k], coefs, delta, stream_mode="torch_cpu")
        torch.cuda.synchronize()
    finally:
        codec.set_cpu_fp32_flavour(None)
    for i in L.live:
        assert _same(outs[i], delta[L.off[i]:L.off[i + 1]]), (_what(name, k), i)
        assert bool(torch.isfinite(outs[i]).all()), i
    for i in range(len(L.sizes)):
        if i not in L.live:
            assert bool(torch.isnan(outs[i]).all()), i
