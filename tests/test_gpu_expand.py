"""Seed-basis expansion written in place on the torch_rocm stream (fks_expand_multi,
codec.expand_multi, zo_utils.seed_expansion_ / seed_expansions_): out = cast(beta out + sum_s
f32(c_s) z_s), an f32 fma chain in seed order rounded once to the output's dtype.

References: torch's own draws on the same GPU (K = 1), and codec.delta_accumulate on a zeroed f32
buffer -- the same chain through 32-seed read-modify-write passes, exact in between because the
buffer is f32 -- whose ranges an f32 output must equal bit for bit and a 2-byte output rounded
once.  Comparisons are bitwise on integer views; where non-finite values are meant, a NaN matches
any NaN.  The tensor list, the frozen tensor and SEEDS are tests/test_gpu_project.py's (about 2.9 M
elements: ragged groups, a capped row, j = 1 items); K = 70 and 4096 extend SEEDS with drawn ones."""
import ctypes
import fractions
import functools
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import _dev
from test_gpu_project import DT, DTYPES, FROZEN, SEEDS, _dense_vec, _offsets, _sizes, _specs

pytestmark = pytest.mark.gpu

MODE = "torch_rocm"
SUB = (4096, 65536)  # the sub-list of the K = 4096 case
_gx = torch.Generator().manual_seed(20261021)
_MORE = torch.randint(0, 2**32, (4096,), generator=_gx).tolist()


def _seeds(k):
    return (SEEDS + _MORE)[:k]


def _coefs(k, row=0, scale=1.0):
    g = torch.Generator().manual_seed(1000 + row)
    return (torch.randn(k, generator=g, dtype=torch.float64) * scale).tolist()


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b, nan_ok=False):
    """bitwise equality of two tensors of one dtype; nan_ok: a NaN matches any NaN"""
    assert a.dtype == b.dtype and a.shape == b.shape
    eq = _bits(a) == _bits(b)
    if nan_ok:
        eq = eq | (torch.isnan(a) & torch.isnan(b))
    return bool(eq.all())


def _alloc(sizes, dtypes, fill=None, dev=None):
    """one output list: a tensor per spec (the frozen one too: it must keep its fill)"""
    dev = _dev() if dev is None else dev
    if not isinstance(dtypes, (list, tuple)):
        dtypes = [dtypes] * len(sizes)
    out = []
    for n, d in zip(sizes, dtypes):
        t = torch.empty(n, dtype=DT[d], device=dev)
        if fill is not None:
            t.fill_(fill)
        out.append(t)
    return out


def _live(sizes):
    return [i for i in range(len(sizes)) if i != FROZEN]


@functools.lru_cache(maxsize=None)
def _delta(dtype, k, row=0, scale=1.0, sizes=None, special=None):
    """codec.delta_accumulate on a zeroed f32 buffer: the per-tensor ranges, computed once per case
    and shared (never written to again)."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    sizes = _sizes() if sizes is None else list(sizes)
    specs = _specs(dtype, sizes, dev)
    coefs = _coefs(k, row, scale)
    if special:  # "inf": an infinite coefficient; "nan+inf": a NaN as well
        coefs[5] = float("inf")
        if special == "nan+inf":
            coefs[1] = float("nan")
    buf = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
    codec.delta_accumulate(specs, _seeds(k), coefs, buf, stream_mode=MODE)
    off = _offsets(sizes)
    return [buf[off[i]:off[i + 1]] for i in range(len(sizes))], coefs


def _expand(dtype, k, coef_rows, outs, betas=None, sizes=None, **kw):
    from fate_llm.algo.fedkseed import codec
    sizes = _sizes() if sizes is None else list(sizes)
    codec.expand_multi(_specs(dtype, sizes), _seeds(k), coef_rows, outs, betas=betas, stream_mode=MODE, **kw)
    torch.cuda.synchronize()


# ---- 1. against torch's own draws
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_seed_equals_torch_draws(dtype):
    dev, sizes = _dev(), _sizes()
    c = 0.37
    outs = _alloc(sizes, "float32", fill=-7.0)
    _expand(dtype, 1, [[c]], [outs])
    torch.manual_seed(SEEDS[0])
    z = [torch.normal(mean=0, std=1, size=(n,), device=dev, dtype=DT[dtype]) for n in sizes]
    c32 = torch.tensor(np.float32(c), device=dev)
    for i, n in enumerate(sizes):
        if i == FROZEN:
            assert bool((outs[i] == -7.0).all())  # the frozen tensor's output keeps its sentinel
            continue
        want = z[i].float() * c32 + 0.0  # fmaf(c, z, +0): one rounding both ways (a -0 product becomes +0)
        assert bool((outs[i] == z[i].float() * c32).all()), i
        assert _same(outs[i], want), i


# ---- 2. against codec.delta_accumulate on a zeroed f32 buffer
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 33, 70])
def test_f32_output_equals_delta_accumulate(dtype, k):
    dev, sizes = _dev(), _sizes()
    ref, coefs = _delta(dtype, k)
    outs = _alloc(sizes, "float32", fill=-7.0)
    _expand(dtype, k, [coefs], [outs])
    for i in range(len(sizes)):
        if i == FROZEN:
            assert bool((outs[i] == -7.0).all())
        else:
            assert _same(outs[i], ref[i]), (i, sizes[i])


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_4096_seeds_read_the_seed_table_far_past_its_first_entries(dtype):
    _dev()
    ref, coefs = _delta(dtype, 4096, sizes=SUB)
    outs = _alloc(SUB, "float32", fill=-7.0)
    _expand(dtype, 4096, [coefs], [outs], sizes=SUB)
    for i in range(len(SUB)):
        assert _same(outs[i], ref[i]), i
    # ... and the result depends on the late seeds: another coefficient for the last one moves it
    other = list(coefs)
    other[-1] += 1.0
    outs2 = _alloc(SUB, "float32")
    _expand(dtype, 4096, [other], [outs2], sizes=SUB)
    assert not _same(outs2[1], outs[1])


# ---- 3. output dtypes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("out_dtypes", ["bfloat16", "float16", "mixed"])
def test_two_byte_outputs_are_the_delta_rounded_once(dtype, out_dtypes):
    """Two coefficient rows in one call, so that the f16 reference holds overflow to inf (row 0,
    sums of spread 1.7e5) and subnormals (row 1, spread 5.7e-6), both asserted.  (One row cannot
    hold both: its sums are spread like one normal variable, and with a spread that reaches 65504
    the chance of a sum below 6.1e-5 is about 1e-9 per element.)"""
    dev, sizes = _dev(), _sizes()
    od = ["bfloat16", "float16", "float32", "float16", "bfloat16", "float16", "float16"] if out_dtypes == "mixed" \
        else [out_dtypes] * len(sizes)
    rows = [_delta(dtype, 33, 1, 3e4), _delta(dtype, 33, 2, 1e-6)]
    outs = [_alloc(sizes, od, fill=-7.0) for _ in rows]
    _expand(dtype, 33, [r[1] for r in rows], outs)
    h_big = torch.cat([rows[0][0][i] for i in _live(sizes)]).to(torch.float16)
    h_tiny = torch.cat([rows[1][0][i] for i in _live(sizes)]).to(torch.float16)
    assert bool(torch.isinf(h_big).any())
    assert bool(((h_tiny != 0) & (h_tiny.abs() < 2.0 ** -14)).any())
    for (ref, _), out in zip(rows, outs):
        for i in _live(sizes):
            assert out[i].dtype == DT[od[i]]
            assert _same(out[i], ref[i].to(DT[od[i]])), (i, od[i])
        assert bool((out[FROZEN] == -7.0).all())


# ---- 4. beta
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
def test_beta_zero_never_reads_the_output(dtype, out_dtype):
    dev, sizes = _dev(), _sizes()
    ref, coefs = _delta(dtype, 33)
    outs = _alloc(sizes, out_dtype, fill=float("nan"))
    _expand(dtype, 33, [coefs], [outs], betas=[0.0])
    for i in _live(sizes):
        assert _same(outs[i], ref[i].to(DT[out_dtype])), i
    assert bool(torch.isnan(outs[FROZEN]).all())


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_beta_scales_the_old_output(dtype, out_dtype, beta):
    """(beta old + delta) in torch f32 is a single rounding (the product by a power of two is
    exact), then the cast: the kernel's fmaf and cast."""
    dev, sizes = _dev(), _sizes()
    ref, coefs = _delta(dtype, 33)
    g = torch.Generator().manual_seed(77)
    old = [(torch.randn(n, generator=g) * 3).to(DT[out_dtype]).to(dev) for n in sizes]
    outs = [o.clone() for o in old]
    _expand(dtype, 33, [coefs], [outs], betas=[beta])
    for i in _live(sizes):
        want = (beta * old[i].float() + ref[i]).to(DT[out_dtype])
        assert _same(outs[i], want), i
    assert _same(outs[FROZEN], old[FROZEN])


# ---- 5. batching invariance
ROW_DTYPES = ["float32", "bfloat16", "float16", "bfloat16", "float32"]


@functools.lru_cache(maxsize=None)
def _single(dtype, m):
    dev, sizes = _dev(), _sizes()
    outs = _alloc(sizes, ROW_DTYPES[m], fill=-7.0)
    _expand(dtype, 33, [_coefs(33, 10 + m)], [outs])
    return outs


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("M", [2, 3, 4, 5])
def test_row_m_equals_the_one_output_call(dtype, M):
    dev, sizes = _dev(), _sizes()
    singles = [_single(dtype, m) for m in range(5)]
    big = len(sizes) - 1
    for a in range(5):  # the five single results differ from each other
        for b in range(a + 1, 5):
            assert not torch.equal(singles[a][big].float(), singles[b][big].float()), (a, b)
    outs = [_alloc(sizes, ROW_DTYPES[m], fill=-7.0) for m in range(M)]
    _expand(dtype, 33, [_coefs(33, 10 + m) for m in range(M)], outs)
    for m in range(M):
        for i in range(len(sizes)):
            assert _same(outs[m][i], singles[m][i]), (m, i)


# ---- 6. shards
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
def test_shards_write_their_own_runs_only(dtype, out_dtype):
    from fate_llm.algo.fedkseed import codec
    dev, sizes = _dev(), _sizes()
    off = _offsets(sizes)
    ref, coefs = _delta(dtype, 33)
    whole = torch.cat([r.to(DT[out_dtype]) for r in ref])
    live = torch.ones(off[-1], dtype=torch.bool, device=dev)
    live[off[FROZEN]:off[FROZEN + 1]] = False
    buf = torch.full((off[-1],), -7.0, dtype=DT[out_dtype], device=dev)
    views = [buf[off[i]:off[i + 1]] for i in range(len(sizes))]
    specs = _specs(dtype, sizes)
    at = 0
    for sh in range(3):
        before = buf.clone()
        lo, hi = codec.shard_range(specs, sh, 3, stream_mode=MODE)
        assert lo == at and hi > lo
        at = hi
        _expand(dtype, 33, [coefs], [views], shard=sh, nshards=3)
        mine = torch.zeros_like(live)
        mine[lo:hi] = True
        assert _same(buf[~(mine & live)], before[~(mine & live)])  # nothing outside its own run
        assert _same(buf[mine & live], whole[mine & live])
    assert at == off[-1]
    assert _same(buf[live], whole[live]) and bool((buf[~live] == -7.0).all())


# ---- 7. launch cuts
def _launch_cuts(specs, k, work):
    from fate_llm.algo.fedkseed import _native as N, codec
    b = codec._Batch(specs, MODE, stage=False)
    n = ctypes.c_int32(0)
    buf = (ctypes.c_int64 * 256)()
    with torch.cuda.device(b.device):
        N.check(N.load().fks_expand_launch_cuts(ctypes.addressof(b.arr), b.n, k, 0, 1, work, 0, buf, 256,
                                                ctypes.byref(n)))
    return list(buf[:n.value])


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_forced_launch_cuts_change_nothing(dtype):
    from fate_llm.algo.fedkseed import codec
    dev, sizes = _dev(), _sizes()
    S = 256 * codec.rocm_grid_cap()  # the big tensor's stride: it has two rows of S items
    work = 4 * S * 33                # one such row at K = 33
    cuts = _launch_cuts(_specs(dtype, sizes), 33, work)
    assert len(cuts) - 1 >= 3 and cuts[-1] - S in cuts and cuts[-1] - 2 * S in cuts  # a cut inside the big tensor
    ref, coefs = _delta(dtype, 33)
    for od in ("float32", "bfloat16"):
        outs = _alloc(sizes, od, fill=-7.0)
        os.environ["FKS_EXPAND_WORK"] = str(work)
        try:
            _expand(dtype, 33, [coefs], [outs])
        finally:
            del os.environ["FKS_EXPAND_WORK"]
        uncut = _alloc(sizes, od, fill=-7.0)
        _expand(dtype, 33, [coefs], [uncut])
        for i in range(len(sizes)):
            assert _same(outs[i], uncut[i]), (od, i)
        for i in _live(sizes):
            assert _same(outs[i], ref[i].to(DT[od])), (od, i)


# ---- 8. alignment
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_outputs_at_element_offset_one(dtype, out_dtype, beta):
    dev, sizes = _dev(), _sizes()
    ref, coefs = _delta(dtype, 33)
    g = torch.Generator().manual_seed(78)
    old = [torch.randn(n, generator=g).to(DT[out_dtype]).to(dev) for n in sizes]
    aligned = [o.clone() for o in old]
    _expand(dtype, 33, [coefs], [aligned], betas=[beta])
    for i in _live(sizes):
        assert aligned[i].data_ptr() % 16 == 0
        assert _same(aligned[i], (beta * old[i].float() + ref[i]).to(DT[out_dtype]) if beta else
                     ref[i].to(DT[out_dtype])), i
    allocs = [torch.full((n + 2,), -7.0, dtype=DT[out_dtype], device=dev) for n in sizes]
    views = [a[1:n + 1] for a, n in zip(allocs, sizes)]
    for v, o in zip(views, old):
        v.copy_(o)
    _expand(dtype, 33, [coefs], [views], betas=[beta])
    for i in range(len(sizes)):
        assert views[i].data_ptr() % 16 != 0
        assert _same(views[i], aligned[i]), i
        assert float(allocs[i][0]) == -7.0 and float(allocs[i][-1]) == -7.0  # the guards on both sides


# ---- 9. non-finite coefficients
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("special", ["nan+inf", "inf"])
def test_nan_and_inf_coefficients(dtype, special):
    """A NaN coefficient turns every sum into NaN, so the infinite one is also run alone: sums of
    either sign of inf (and NaN where inf meets a zero z or the other sign)."""
    dev, sizes = _dev(), _sizes()
    ref, coefs = _delta(dtype, 33, special=special)
    assert np.isinf(coefs[5]) and np.isnan(coefs[1]) == (special == "nan+inf")
    outs = _alloc(sizes, "float32", fill=-7.0)
    _expand(dtype, 33, [coefs], [outs])
    for i in _live(sizes):
        assert bool((torch.isnan(ref[i]) if special == "nan+inf" else torch.isinf(ref[i])).any())
        assert _same(outs[i], ref[i], nan_ok=True), i


# ---- 10. zo_utils
def _params(dtype, sizes, dev):
    return [torch.nn.Parameter(torch.zeros(n, dtype=DT[dtype], device=dev), requires_grad=(i != FROZEN))
            for i, n in enumerate(sizes)]


def test_seed_expansion_fills_grad():
    from fate_llm.algo.fedkseed import zo_utils
    dev, sizes = _dev(), _sizes()
    params = _params("bfloat16", sizes, dev)
    groups = [{"params": params[:3]}, {"params": params[3:]}]
    scalars = _coefs(33, 20)
    got = zo_utils.seed_expansion_(groups, _seeds(33), scalars, stream_mode=MODE)
    want = _alloc(sizes, "bfloat16", fill=-7.0)
    _expand("bfloat16", 33, [scalars], [want])
    assert params[FROZEN].grad is None and got[FROZEN] is None
    for i in _live(sizes):
        assert got[i] is params[i].grad and params[i].grad.dtype == torch.bfloat16
        assert _same(params[i].grad, want[i]), i
    # accumulate=True adds to what is there
    first = [None if p.grad is None else p.grad.clone() for p in params]
    more = _coefs(33, 21)
    zo_utils.seed_expansion_(groups, _seeds(33), more, accumulate=True, stream_mode=MODE)
    added = [torch.full_like(w, -7.0) if f is None else f.clone() for f, w in zip(first, want)]
    _expand("bfloat16", 33, [more], [added], betas=[1.0])
    for i in _live(sizes):
        assert _same(params[i].grad, added[i]), i
        assert not _same(params[i].grad, first[i])


def test_seed_expansions_rows_equal_the_single_calls():
    from fate_llm.algo.fedkseed import zo_utils
    dev, sizes = _dev(), _sizes()
    params = _params("bfloat16", sizes, dev)
    groups = [{"params": params}]
    rows = [_coefs(33, 30 + m) for m in range(3)]
    names = ("float32", "bfloat16", "float16")
    lists = [_alloc(sizes, d, fill=-7.0) for d in names]
    got = zo_utils.seed_expansions_(groups, _seeds(33), rows, lists, stream_mode=MODE)
    for m in range(3):
        single = _alloc(sizes, names[m], fill=-7.0)
        zo_utils.seed_expansion_(groups, _seeds(33), rows[m], outputs=single, stream_mode=MODE)
        for i in _live(sizes):
            assert got[m][i] is lists[m][i]
            assert _same(lists[m][i], single[i]), (m, i)
        assert bool((lists[m][FROZEN] == -7.0).all())


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_adjoint_identity(dtype):
    """<v, expand(c)> = sum_s c_s project(v)_s up to the roundings of either side: the expansion's f32
    chain, (k + 1) 2^-24 sum_e |v_e| sum_s |c_s z_s,e| (k fmas and nothing else: k roundings; one more
    for slack as the issue states it), the projection's documented n 2^-52 sum |v z| |c|, and the f64
    dot's n 2^-52 sum_e |v_e| |expand(c)_e|.  The first is evaluated from torch's draws.  The
    difference itself is formed exactly (fractions), so nothing else enters."""
    from fate_llm.algo.fedkseed import codec
    dev, sizes = _dev(), _sizes()
    k = 8
    off = _offsets(sizes)
    live = torch.ones(off[-1], dtype=torch.bool, device=dev)
    live[off[FROZEN]:off[FROZEN + 1]] = False
    n = int(live.sum())
    c = [float(np.float32(x)) for x in _coefs(k, 40)]  # f32-exact: both sides see the same numbers
    v = _dense_vec(off[-1]).to(dev)
    vs = [None if i == FROZEN else v[off[i]:off[i + 1]] for i in range(len(sizes))]
    specs = _specs(dtype, sizes)
    outs = [None if i == FROZEN else torch.empty(m, dtype=torch.float32, device=dev) for i, m in enumerate(sizes)]
    codec.expand_multi(specs, _seeds(k), [c], [outs], stream_mode=MODE)
    proj = codec.project_multi(specs, _seeds(k), [vs], stream_mode=MODE)[0].cpu().tolist()
    e64 = torch.cat([torch.zeros(m, device=dev) if o is None else o for o, m in zip(outs, sizes)]).double()
    v64 = v.double()
    lhs = float(torch.dot(v64[live], e64[live]))
    rhs = sum(fractions.Fraction(cs) * fractions.Fraction(g) for cs, g in zip(c, proj))
    err = float(abs(fractions.Fraction(lhs) - rhs))
    chain = torch.zeros(off[-1], dtype=torch.float64, device=dev)
    b_proj = 0.0
    for s, cs in zip(_seeds(k), c):
        torch.manual_seed(s)
        z = torch.cat([torch.normal(mean=0, std=1, size=(m,), device=dev, dtype=DT[dtype]).double() for m in sizes])
        chain += abs(cs) * z.abs()
        b_proj += abs(cs) * float((v64.abs() * z.abs())[live].sum())
    b_chain = (k + 1) * 2.0 ** -24 * float((v64.abs() * chain)[live].sum())
    b_proj *= n * 2.0 ** -52
    b_dot = n * 2.0 ** -52 * float((v64.abs() * e64.abs())[live].sum())
    print(f"{dtype}: |lhs - rhs| = {err:.3e}, bounds: chain {b_chain:.3e} + projection {b_proj:.3e} + dot {b_dot:.3e}")
    assert err <= b_chain + b_proj + b_dot
