"""Bit-sliced seed-basis expansion on the torch_cpu stream (fks_expand_mt_bs, codec.expand_mt_bs,
zo_utils.seed_expansions_bitsliced_) against the reference of tests/test_gpu_expand_mt.py: torch's
CPU draws (mt_layouts.zs / draw), widened to f32 and folded by tests/exact_f32.py -- chain32 from
+0, fma32(f32(beta), widen(old), acc) where beta != 0, torch's cast.  Every comparison is bitwise on
every live element; guards, frozen tensors and elements outside the shard keep their sentinel
(tests/test_gpu_expand_exact.py's buffers and row check).

Lists: tests/test_gpu_project_mt_bs.py's -- G in bf16, mixed and f16 (no bf16 fast segment: no
bit-sliced launch), R (tasks wrap the 624-row state, a workgroup walks gaps), one bf16 tensor of 16
elements (one task) and one of 128 W 3 + 48 (every wave of a half has tasks, the last partial).
K: 0 (the 19-seed path), 1 and 19 (single partial), 32 (single full), 33 (first + last partial), 64
(first + last full), 65 and 97 (first + middle + last); on G:mixed and R the 19-seed sequence runs
out of step with the 32-seed one."""
import functools

import pytest
import torch

import mt_layouts as ML
from exact_f32 import chain32, f32, fma32
from test_gpu_expand import _coefs, _same
from test_gpu_expand_exact import _List, _buffers, _check_row
from test_gpu_parity import _dev
from test_gpu_project_mt_bs import S97

pytestmark = pytest.mark.gpu

W = 4  # waves per half (csrc/fks_expand_mt_bs.h FKS_EMBS_WAVES)
KS = [0, 1, 19, 31, 32, 33, 64, 65, 97]
OWN = {"one16": ML.MtList("one16", (16,), ("bfloat16",), ()),
       "waves": ML.MtList("waves", (128 * W * 3 + 48,), ("bfloat16",), ())}
LISTS = ["G:bfloat16", "G:mixed", "G:float16", "R", "one16", "waves"]
ROWS = ["float32", "bfloat16", "float16"]  # output dtypes over the rows of a call
BETAS = [0.0, -0.0, 0.3, 1.0]  # 0 and -0: on NaN-filled outputs, never read
_get = lambda name: OWN.get(name) or ML.get(name)  # noqa: E731


@functools.lru_cache(maxsize=None)
def _L(name):
    lst = _get(name)
    return _List(lst.sizes, lst.dts, frozen=lst.frozen)


@functools.lru_cache(maxsize=None)
def _specs(name):
    return tuple(_L(name).specs(_dev()))


@functools.lru_cache(maxsize=None)
def _zs(name):
    """the 97 seeds' reference draws over the list, on the device; drawn once, never written to"""
    z = ML.zs(name, S97) if name in ML.G_NAMES else [ML.draw(_get(name), s) for s in S97]
    return [x.to(_dev()) for x in z]


def _row(row):
    return _coefs(len(S97), row)


@functools.lru_cache(maxsize=None)
def _sums(name, row):
    """the exact chain of coefficient row `row` at every K of KS: {K: f32 sums}"""
    coefs, zs = _row(row), _zs(name)
    acc = torch.zeros_like(zs[0])
    out = {0: acc}
    for k in range(len(S97)):
        acc = fma32(torch.tensor(f32(coefs[k]), device=acc.device), zs[k], acc)
        if k + 1 in KS:
            out[k + 1] = acc
    assert _same(out[33], chain32(coefs[:33], zs[:33]))  # the fold above is chain32's
    return out


def _run(name, rows, row_names, betas=None, offset=0, k=97, coefs=None, nshards=1, fn=None, **kw):
    """One expand_mt_bs call (one per shard with nshards > 1: ownership is disjoint, so an element
    written twice would take its beta twice and one never written keeps NaN) on fresh buffers, every
    row checked against the exact reference; returns the views per row."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _L(name)
    bs = [0.0] * len(rows) if betas is None else list(betas)
    made = [_buffers(L, row_names[m], bs[m], offset, dev, 300 + 100 * m) for m in range(len(rows))]
    cs = [_row(r)[:k] for r in rows] if coefs is None else coefs
    for sh in range(nshards):
        (fn or codec.expand_mt_bs)(_specs(name), S97[:k], cs, [v for _, v, _ in made], betas=betas, shard=sh,
                                   nshards=nshards, **kw)
    torch.cuda.synchronize()
    for m in range(len(rows)):
        acc = _sums(name, rows[m])[k] if coefs is None else chain32(cs[m], _zs(name)[:k])
        _check_row(L, row_names[m], bs[m], acc, *made[m], what=f"list {name}, K {k}, shards {nshards}, row {m}")
    return [v for _, v, _ in made]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", LISTS)
def test_chain_is_exact(name, k):
    """Three outputs, f32, bf16 and f16, the four betas rotating with K."""
    r = KS.index(k)
    betas = [BETAS[(m + r) % 4] for m in range(3)]
    got = _run(name, [400, 400, 400], ROWS, betas=betas, k=k)
    for m in range(3):
        if betas[m] == 0:
            for i in _L(name).live:
                assert bool(torch.isfinite(got[m][i]).all()), (m, i)
                if k == 0:  # +0, all bits zero
                    assert not bool(got[m][i].view(torch.int32 if m == 0 else torch.int16).any()), (m, i)


@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_outputs_one_element_off_alignment(name):
    L = _L(name)
    names = [[ROWS[(i + m) % 3] for i in range(len(L.sizes))] for m in range(2)]  # dtypes mixed over a row
    _run(name, [400, 401], names, betas=[0.3, 0.0], offset=1, k=65)


@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_every_element_is_written_by_exactly_one_shard(name, nshards):
    _run(name, [400, 400], ["float32", "bfloat16"], betas=[0.0, 0.3], k=65, nshards=nshards)


@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_small_staging_budget_splits_the_call(name):
    """K = 65 under a budget that two shards' larger part does not fit: at least three internal shards."""
    from fate_llm.algo.fedkseed import codec
    b = codec._Batch(list(_specs(name)), "torch_cpu", stage=False)
    two = max(st for _, st in codec._expand_mt_sizes(b, 65, 1, 2, True))
    assert 0 < max(st for _, st in codec._expand_mt_sizes(b, 65, 1, 3, True)) < two
    _run(name, [400], ["bfloat16"], betas=[0.3], k=65, staging_bytes=two - 1)


@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_two_outputs_equal_the_single_calls(name):
    two = _run(name, [401, 402], ["bfloat16", "float32"], betas=[0.3, 0.0], k=65)
    a = _run(name, [401], ["bfloat16"], betas=[0.3], k=65)
    b = _run(name, [402], ["float32"], k=65)
    for i in _L(name).live:
        assert _same(two[0][i], a[0][i]) and _same(two[1][i], b[0][i]), i


@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_subnormal_coefficients_and_the_minus_zero_sum(name):
    """-2^-149 z underflows to -0 where |z| < 1/2, and fma(c, z, +0) keeps that -0: at K = 1 a pass
    padded with zero coefficients would turn it into +0.  The other coefficients are f32 subnormals."""
    coefs = [-2.0 ** -149] + [(-1) ** j * (j % 7 + 1) * 2.0 ** -140 for j in range(1, 33)]
    ref = chain32(coefs[:1], _zs(name)[:1])
    assert bool((ref.view(torch.int32) == -2 ** 31).any())  # the reference holds -0
    for k in (1, 33):
        _run(name, [None, None], ["float32", "bfloat16"], k=k, coefs=[coefs[:k], coefs[:k]])


@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_bits_of_expand_mt_multi(name):
    from fate_llm.algo.fedkseed import codec
    L = _L(name)
    names = [[ROWS[(i + m) % 3] for i in range(len(L.sizes))] for m in range(2)]
    bs = _run(name, [401, 402], names, betas=[1.0, 0.0], k=97)
    multi = _run(name, [401, 402], names, betas=[1.0, 0.0], k=97, fn=codec.expand_mt_multi)
    for m in range(2):
        for i in L.live:
            assert _same(bs[m][i], multi[m][i]), (m, i)


@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_zo_utils_routes_by_stream(name):
    from fate_llm.algo.fedkseed import zo_utils
    dev, lst, L = _dev(), _get(name), _L(name)
    coefs = _row(401)[:65]

    def params():
        ps = [torch.nn.Parameter(torch.zeros(n, dtype=ML.DT[d], device=dev)) for n, d in zip(lst.sizes, lst.dts)]
        for i in lst.frozen:
            ps[i].requires_grad_(False)
        return ps

    got, ref = params(), params()
    zo_utils.seed_expansion_bitsliced_([{"params": got}], S97[:65], coefs, stream_mode="torch_cpu")
    torch.cuda.synchronize()
    acc = _sums(name, 401)[65]
    for i in L.live:
        assert _same(got[i].grad, acc[L.off[i]:L.off[i + 1]].to(got[i].dtype)), i
    assert all(got[i].grad is None for i in lst.frozen)
    for acc_ in (False, True):  # the default stream: seed_expansion_'s call
        zo_utils.seed_expansions_bitsliced_([{"params": got}], S97[:33], [coefs[:33]], [None], accumulate=acc_,
                                            stream_mode="torch_rocm")
        zo_utils.seed_expansion_([{"params": ref}], S97[:33], coefs[:33], accumulate=acc_, stream_mode="torch_rocm")
        torch.cuda.synchronize()
        for i in L.live:  # (the first call overwrote the torch_cpu result)
            assert _same(got[i].grad, ref[i].grad), i
