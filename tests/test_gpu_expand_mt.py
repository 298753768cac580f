"""fks_expand_mt_multi (codec.expand_mt_multi, torch_cpu stream; zo_utils.seed_expansion_on_stream_
routed there) against a reference outside our code: torch's CPU generator -- after
torch.manual_seed(s), torch.normal(0, 1, (n,), dtype) per tensor in list order on the CPU, frozen
ones drawn and dropped --, widened to f32 and folded by tests/exact_f32.py: chain32 gives
acc = RN_f32(f32(c_s) z_s + acc) from +0, fma32(f32(beta), widen(old), acc) the scaled sum where
beta != 0, torch's .to(out dtype) the cast.  Every comparison is bitwise on integer views over every
live element of every output; a NaN matches any NaN only where the test says so.  Outputs lie
inside buffers with guard elements on both sides; guards and the frozen and empty tensors' buffers
keep their sentinel (tests/test_gpu_expand_exact.py's buffers and row check).

The list is tests/test_gpu_project_mt.py's, in each of the three dtypes: 1,048,576 (fast; plan
chunks of 2 and 3 MT blocks), 4,096 (fast), 3 frozen (serial draws, a cached second value left
behind), 1,000 (phase 8: a ragged head, 16 fresh tail words), 7 (its first element takes the cached
value), 65,536 (a run whose 16-blocks straddle MT blocks), 0, 48; for f16 every run is irregular.
K = 0 (a pass without seeds), 1 (a partial pass), 19 (a full pass), 20 (first + last through the
staging area), 39 (first + middle + last): there the last pass has 1 seed.  Four more K reach the
pass shapes those leave out: 18 (a single pass one seed short of full), 37 (first + a last partial
pass of 18 seeds), 38 (first + a last FULL pass: the instance that reads the staged carry and the
old output and writes through beta and the cast with all 19 seeds unrolled) and 57 (first + middle
+ last full).  fma32 runs on the device (test_gpu_expand_exact.py checks that it is the host's
there).  tests/test_gpu_expand_mt_layouts.py runs the same call over the lists of
tests/mt_layouts.py."""
import functools

import pytest
import torch

from exact_f32 import chain32, f32, fma32
from test_gpu_expand import _coefs, _same
from test_gpu_expand_exact import GUARD, _List, _buffers, _check_row
from test_gpu_parity import _dev
from test_gpu_project_mt import DT, DTYPES, FROZEN, SEEDS, SIZES

pytestmark = pytest.mark.gpu

_g = torch.Generator().manual_seed(20261021)
SEEDS40 = SEEDS + torch.randint(0, 2**32, (20,), generator=_g).tolist()
SEEDS57 = SEEDS40 + torch.randint(0, 2**32, (17,), generator=_g).tolist()  # the first 40 are SEEDS40
KMAX = len(SEEDS57)
ROWS = ["float32", "bfloat16", "float16"]  # output dtypes over the rows of a call
KS = [0, 1, 19, 20, 39, 18, 37, 38, 57]  # (appended: a K's place sets its betas in test_chain_is_exact)
KEPT = set(KS) | {7, 40}  # the K at which _sums keeps the chain


@functools.lru_cache(maxsize=None)
def _list(dtype):
    return _List(SIZES, [dtype] * len(SIZES), frozen=(FROZEN,))


@functools.lru_cache(maxsize=None)
def _specs(dtype):
    """one spec list per dtype, kept for the session (a stable plan key)"""
    return tuple(_list(dtype).specs(_dev()))


@functools.lru_cache(maxsize=None)
def _zs(dtype):
    """the 57 seeds' draws over the concatenation as the reference draws them on the CPU (frozen
    tensors too), widened to f32, on the device; drawn once, shared, never written to"""
    out = []
    for s in SEEDS57:
        torch.manual_seed(s)
        z = [torch.normal(mean=0, std=1, size=(n,), dtype=DT[dtype]).float() for n in SIZES]
        out.append(torch.cat(z).to(_dev()))
    return out


@functools.lru_cache(maxsize=None)
def _sums(dtype, row, scale=1.0, special=()):
    """the exact chain of coefficient row `row` at every K of KEPT: {K: f32 sums}"""
    coefs = _row(row, scale, special)
    zs = _zs(dtype)
    acc = torch.zeros_like(zs[0])
    out = {0: acc}
    for k in range(KMAX):
        acc = fma32(torch.tensor(f32(coefs[k]), device=acc.device), zs[k], acc)
        if k + 1 in KEPT:
            out[k + 1] = acc
    assert _same(out[20], chain32(coefs[:20], zs[:20]))  # the fold above is chain32's
    return out


def _row(row, scale=1.0, special=()):
    c = _coefs(40, row, scale) + _coefs(KMAX - 40, 5000 + row, scale)  # (the first 40 as before the list grew)
    for at, v in special:
        c[at] = v
    return c


def _run(dtype, rows, row_names, betas=None, offset=0, k=39, nan_ok=False, check=True, scale=1.0, special=(), **kw):
    """One expand_mt_multi call on fresh buffers, synchronized, every row checked against the exact
    reference; returns (views per row, buffers per row)."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _list(dtype)
    M = len(rows)
    bs = [0.0] * M if betas is None else list(betas)
    made = [_buffers(L, row_names[m], bs[m], offset, dev, 700 + 100 * m) for m in range(M)]
    coefs = [_row(r, scale, special)[:k] for r in rows]
    codec.expand_mt_multi(_specs(dtype), SEEDS57[:k], coefs, [v for _, v, _ in made], betas=betas, **kw)
    torch.cuda.synchronize()
    if check:
        for m in range(M):
            _check_row(L, row_names[m], bs[m], _sums(dtype, rows[m], scale, special)[k], *made[m],
                       what=f"z {dtype}, K {k}, row {m}", nan_ok=nan_ok)
    return [v for _, v, _ in made], [b for b, _, _ in made]


# ---- 1. the chain: every z dtype x every output dtype x every pass structure
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_is_exact(dtype, k):
    """Three outputs, one per dtype, betas 0 (NaN-filled, never read), 0.3 and 1 rotating with K."""
    r = KS.index(k)
    betas = [(0.0, 0.3, 1.0)[(m + r) % 3] for m in range(3)]
    got, _ = _run(dtype, [80, 81, 82], ROWS, betas=betas, k=k)
    for m in range(3):
        if betas[m] == 0:
            for i in _list(dtype).live:
                assert bool(torch.isfinite(got[m][i]).all()), (m, i)
                if k == 0:  # +0, all bits zero
                    assert not bool(got[m][i].view(torch.int32 if m == 0 else torch.int16).any()), (m, i)


# ---- 2. betas and alignment
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_betas_and_alignment(dtype, offset):
    """Outputs 16-byte aligned and one element off; betas 0 and -0 on NaN-filled outputs (never
    read), 1 and 0.3; output dtypes mixed over the tensors of a row.  K = 20: the betas enter in
    the last pass only, after the staged sum."""
    L = _list(dtype)
    names = [[ROWS[(i + m) % 3] for i in range(len(L.sizes))] for m in range(4)]
    betas = [0.0, 1.0, 0.3, -0.0]
    got, _ = _run(dtype, [83, 84, 85, 86], names, betas=betas, offset=offset, k=20)
    for m in (0, 3):
        for i in L.live:
            assert bool(torch.isfinite(got[m][i]).all()), (m, i)
    _run(dtype, [83, 84], ROWS[1:], betas=[0.3, -0.0], offset=offset, k=1)  # one pass


# ---- 3. fks_delta_accumulate's bits
@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_output_equals_delta_accumulate(dtype):
    """K = 40, f32 output, beta 0, against codec.delta_accumulate(stream_mode="torch_cpu") on a
    zeroed buffer, bit for bit (for bf16 that path takes the slice kernel: other code)."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _list(dtype)
    coefs = _row(87)[:40]
    outs = [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in SIZES]
    codec.expand_mt_multi(_specs(dtype), SEEDS40, [coefs], [outs])
    delta = torch.zeros(sum(SIZES), dtype=torch.float32, device=dev)
    codec.delta_accumulate(_specs(dtype), SEEDS40, coefs, delta, stream_mode="torch_cpu")
    torch.cuda.synchronize()
    for i in L.live:
        assert _same(outs[i], delta[L.off[i]:L.off[i + 1]]), i
        assert _same(outs[i], _sums(dtype, 87)[40][L.off[i]:L.off[i + 1]]), i
    assert bool(torch.isnan(outs[FROZEN]).all())


# ---- 4. shards
@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_union_is_the_whole_call(dtype, nshards):
    """Every shard on sentinel-filled outputs of its own: what a shard writes equals the whole
    call's element, what it does not write keeps the sentinel, and every live element is written by
    exactly one shard.  K = 20 (staged per shard), bf16 outputs with beta 1 over the sentinel -- so
    an element written twice would also show in the union call below."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _list(dtype)
    coefs = [_row(88)[:20]]
    sent = 1.0e9  # far outside any sum of 20 N(0, 1) coefficients times |z| <= 7

    def fresh(d=torch.float32):
        return [torch.full((n,), sent, dtype=d, device=dev) for n in SIZES]

    whole = fresh()
    codec.expand_mt_multi(_specs(dtype), SEEDS40[:20], coefs, [whole])
    count = [torch.zeros(n, dtype=torch.int32, device=dev) for n in SIZES]
    union = fresh(torch.bfloat16)
    for sh in range(nshards):
        part = fresh()
        codec.expand_mt_multi(_specs(dtype), SEEDS40[:20], coefs, [part], shard=sh, nshards=nshards)
        codec.expand_mt_multi(_specs(dtype), SEEDS40[:20], coefs, [union], betas=[1.0], shard=sh, nshards=nshards)
        torch.cuda.synchronize()
        for i in range(len(SIZES)):
            wrote = part[i] != sent
            count[i] += wrote.int()
            assert _same(torch.where(wrote, part[i], whole[i]), whole[i]), (sh, i)
        assert any(bool((part[i] == sent).any()) for i in L.live), sh  # a shard is not the whole call
    acc = _sums(dtype, 88)[20]
    for i in range(len(SIZES)):
        if i in L.live:
            assert bool((count[i] == 1).all()), i
            a = acc[L.off[i]:L.off[i + 1]]
            assert _same(whole[i], a), i
            assert _same(union[i], fma32(1.0, torch.full_like(a, sent).bfloat16().float(), a).bfloat16()), i
        else:
            assert not bool(count[i].any()), i


# ---- 5. the internal split
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_small_staging_budget_splits_the_call(dtype):
    """K = 39 under a staging budget that needs at least three internal shards equals the reference
    (and so the one-shard call).  The budget: two shards' larger half cannot fit."""
    from fate_llm.algo.fedkseed import codec
    b = codec._Batch(list(_specs(dtype)), "torch_cpu", stage=False)
    two = max(st for _, st in codec._expand_mt_sizes(b, 39, 1, 2))
    three = max(st for _, st in codec._expand_mt_sizes(b, 39, 1, 3))
    assert three < two
    one, _ = _run(dtype, [89], ["bfloat16"], k=39)
    split, _ = _run(dtype, [89], ["bfloat16"], k=39, staging_bytes=two - 1)
    tiny, _ = _run(dtype, [89], ["bfloat16"], k=39, staging_bytes=three // 4)
    for i in _list(dtype).live:
        assert _same(split[0][i], one[0][i]) and _same(tiny[0][i], one[0][i]), i
    with pytest.raises(ValueError, match="staging_bytes"):
        _run(dtype, [89], ["bfloat16"], k=39, staging_bytes=16, check=False)


# ---- 6. rows
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_outputs_equal_the_single_calls(dtype):
    two, _ = _run(dtype, [90, 91], ["bfloat16", "float32"], betas=[0.3, 0.0], k=39)
    a, _ = _run(dtype, [90], ["bfloat16"], betas=[0.3], k=39)
    b, _ = _run(dtype, [91], ["float32"], k=39)
    for i in _list(dtype).live:
        assert _same(two[0][i], a[0][i]) and _same(two[1][i], b[0][i]), i


# ---- 7. special values
@pytest.mark.parametrize("dtype", DTYPES)
def test_inf_and_nan_coefficients(dtype):
    """An inf coefficient makes +-inf (NaN where z is 0, and inf - inf later on); a NaN one makes
    every sum NaN.  NaN payloads are not part of the contract."""
    inf = ((3, float("inf")),)
    ref = _sums(dtype, 92, 1.0, inf)[20]
    assert bool(torch.isinf(ref).any())
    _run(dtype, [92], ["float32"], k=20, special=inf, nan_ok=True)
    _run(dtype, [92], ["bfloat16"], betas=[1.0], k=39, special=inf, nan_ok=True)
    nan = ((7, float("nan")),)
    got, _ = _run(dtype, [93], ["float16"], k=20, special=nan, nan_ok=True)
    for i in _list(dtype).live:
        assert bool(torch.isnan(got[0][i]).all()), i
    fine, _ = _run(dtype, [93], ["float16"], k=7, special=nan)  # the NaN coefficient is past the call's seeds
    assert all(bool(torch.isfinite(fine[0][i]).all()) for i in _list(dtype).live)


@pytest.mark.parametrize("dtype", DTYPES)
def test_f16_overflow(dtype):
    """Coefficients of about 3e4: the f32 sums are finite, their f16 casts overflow to +-inf."""
    ref = _sums(dtype, 94, 3e4)[20]
    assert bool(torch.isfinite(ref).all()) and bool(torch.isinf(ref.half()).any())
    _run(dtype, [94, 94], ["float16", "float32"], k=20, scale=3e4)


# ---- 8. streams and generators
def test_the_call_runs_on_the_current_stream():
    """The outputs hold NaN; on a side stream they are filled with 2.0 and expanded with beta 1.0:
    fma(1, 2.0, acc) everywhere only if every launch and the table's upload ran on that stream."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _list("bfloat16")
    names = ["float32", "bfloat16"]
    outs = [[torch.full((n,), float("nan"), dtype=DT[d], device=dev) for n in SIZES] for d in names]
    accs = [_sums("bfloat16", r)[39] for r in (95, 96)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for o in outs:
            for t in o:
                t.fill_(2.0)
        codec.expand_mt_multi(_specs("bfloat16"), SEEDS40[:39], [_row(95)[:39], _row(96)[:39]], outs, betas=[1.0, 1.0])
    side.synchronize()
    for m in range(2):
        for i in L.live:
            a = accs[m][L.off[i]:L.off[i + 1]]
            assert _same(outs[m][i], fma32(1.0, torch.full_like(a, 2.0), a).to(DT[names[m]])), (m, i)


def test_torchs_generators_are_left_alone():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    torch.manual_seed(12345)
    torch.cuda.manual_seed(54321)
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    _run("float32", [97], ["bfloat16"], k=20, check=False)
    _run("float32", [97], ["bfloat16"], k=1, check=False)
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(dev), gpu)
    assert codec.get_stream_mode() in codec.STREAM_SETTINGS


# ---- 9. the other fp32 flavour
@pytest.mark.parametrize("k", [19, 20, 38])
def test_other_fp32_flavour_equals_delta_accumulate(k):
    """The fp32 flavour that is not this process's (no torch draw of it exists here) against
    fks_delta_accumulate under the same setting, bit for bit; it differs from this process's."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _list("float32")
    here = codec.cpu_fp32_flavour()
    other = "libm" if here == "avx" else "avx"
    coefs = _row(98)[:k]

    def both():
        outs = [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in SIZES]
        codec.expand_mt_multi(_specs("float32"), SEEDS40[:k], [coefs], [outs])
        delta = torch.zeros(sum(SIZES), dtype=torch.float32, device=dev)
        codec.delta_accumulate(_specs("float32"), SEEDS40[:k], coefs, delta, stream_mode="torch_cpu")
        torch.cuda.synchronize()
        return outs, delta

    codec.set_cpu_fp32_flavour(other)
    try:
        outs, delta = both()
    finally:
        codec.set_cpu_fp32_flavour(None)
    mine, _ = both()
    for i in L.live:
        assert _same(outs[i], delta[L.off[i]:L.off[i + 1]]), i
    big = 0  # the 2^20-element fast tensor and the 65,536-element run draw fp32 in the flavour
    assert not _same(outs[big], mine[big]) and not _same(outs[5], mine[5])


# ---- 10. zo_utils
def _params(dtype, dev, frozen=(FROZEN,)):
    ps = [torch.nn.Parameter(torch.zeros(n, dtype=DT[dtype], device=dev)) for n in SIZES]
    for i in frozen:
        ps[i].requires_grad_(False)
    return ps


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_seed_expansion_on_stream_torch_cpu(dtype):
    """Default outputs are the .grads, created in the parameter's dtype; accumulate adds; the
    result is codec.expand_mt_multi's, which test_chain_is_exact ties to the reference."""
    from fate_llm.algo.fedkseed import codec, zo_utils
    dev, L = _dev(), _list(dtype)
    ps = _params(dtype, dev)
    coefs = _row(99)[:20]
    outs = zo_utils.seed_expansion_on_stream_([{"params": ps}], SEEDS40[:20], coefs, stream_mode="torch_cpu")
    torch.cuda.synchronize()
    acc = _sums(dtype, 99)[20]
    assert ps[FROZEN].grad is None and outs[FROZEN] is None
    for i in L.live:
        assert ps[i].grad is outs[i] and ps[i].grad.dtype == DT[dtype]
        assert _same(ps[i].grad, acc[L.off[i]:L.off[i + 1]].to(DT[dtype])), i
    first = [None if p.grad is None else p.grad.clone() for p in ps]
    zo_utils.seed_expansion_on_stream_([{"params": ps}], SEEDS40[:1], coefs[:1], accumulate=True, stream_mode="torch_cpu")
    want = [None if g is None else g.clone() for g in first]
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in ps]
    codec.expand_mt_multi(specs, SEEDS40[:1], [coefs[:1]], [want], betas=[1.0])
    torch.cuda.synchronize()
    one = _sums(dtype, 99)[1]
    for i in L.live:
        assert _same(ps[i].grad, want[i]), i
        a = one[L.off[i]:L.off[i + 1]]
        assert _same(ps[i].grad, fma32(1.0, first[i].float(), a).to(DT[dtype])), i
    # two output lists in one call equal the single calls
    o2 = [[torch.empty(n, dtype=torch.float32, device=dev) for n in SIZES] for _ in range(2)]
    zo_utils.seed_expansions_on_stream_([{"params": ps}], SEEDS40[:20], [coefs, _row(80)[:20]], o2, stream_mode="torch_cpu")
    torch.cuda.synchronize()
    for i in L.live:
        assert _same(o2[0][i], acc[L.off[i]:L.off[i + 1]]), i
        assert _same(o2[1][i], _sums(dtype, 80)[20][L.off[i]:L.off[i + 1]]), i


def test_seed_expansion_on_stream_torch_rocm_equals_seed_expansion_():
    from fate_llm.algo.fedkseed import zo_utils
    dev = _dev()
    sizes = [4096, 1000, 7]
    coefs = _row(99)[:33]
    got = [torch.nn.Parameter(torch.zeros(n, dtype=torch.bfloat16, device=dev)) for n in sizes]
    ref = [torch.nn.Parameter(torch.zeros(n, dtype=torch.bfloat16, device=dev)) for n in sizes]
    for acc in (False, True):
        zo_utils.seed_expansion_on_stream_([{"params": got}], SEEDS40[:33], coefs, accumulate=acc, stream_mode="torch_rocm")
        zo_utils.seed_expansion_([{"params": ref}], SEEDS40[:33], coefs, accumulate=acc, stream_mode="torch_rocm")
        torch.cuda.synchronize()
        for a, b in zip(got, ref):
            assert a.grad.dtype == torch.bfloat16 and _same(a.grad, b.grad)
    assert bool(got[0].grad.any())
    # without a stream_mode the call takes the stream the process-wide setting resolves to
    from fate_llm.algo.fedkseed import codec
    mode = codec.resolve_stream_mode(dev, None)
    for ps in (got, ref):
        for p in ps:
            p.grad = None
    zo_utils.seed_expansion_on_stream_([{"params": got}], SEEDS40[:33], coefs)
    zo_utils.seed_expansion_on_stream_([{"params": ref}], SEEDS40[:33], coefs, stream_mode=mode)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert _same(a.grad, b.grad)
