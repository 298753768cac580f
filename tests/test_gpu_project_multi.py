"""Seed-basis projection of several vectors, each read where it lies (fks_project_multi,
codec.project_multi, zo_utils.seed_projections_multi / fit_seed_scalars_multi).

The reference is codec.project itself (tests/test_gpu_project.py checks it against torch's
draws): fks_project_multi adds the same exact products in the same order, so every comparison
here is BITWISE on the int64 view of the float64 results unless a test says otherwise --
against codec.project on the f32 widening of the vectors laid end to end, or against the
one-vector call.  The one-hot test goes back to torch.normal on the device.

Tensor list, seeds and helpers are those of tests/test_gpu_project.py: its seven tensors
(the third frozen, a ragged and a capped row, j = 1 items; about 2.9 M elements), k = 1 and
33 (33 crosses the 32-seed pass); vector counts 1 .. 5 (5 crosses the four-vector pass)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import _dev
from test_gpu_project import (DT, DTYPES, FROZEN, SEEDS, U, _case, _dense_vec, _i64, _mixed_specs, _offsets, _sizes,
                              _specs, _stride)

pytestmark = pytest.mark.gpu

MIXED = ["bfloat16", "float16", "float32"]  # vector dtypes taken in turn, tensor by tensor


def _project(specs, k, buf, **kw):
    from fate_llm.algo.fedkseed import codec
    return _i64(codec.project(specs, SEEDS[:k], buf, stream_mode="torch_rocm", **kw))


def _multi(specs, k, vectors, **kw):
    from fate_llm.algo.fedkseed import codec
    got = codec.project_multi(specs, SEEDS[:k], vectors, stream_mode="torch_rocm", **kw)
    assert got.dtype == torch.float64 and got.shape == (len(vectors), k) and got.device.type == "cuda"
    return _i64(got)


def _views(buf, sizes):
    off = _offsets(sizes)
    return [buf[off[i]:off[i + 1]] for i in range(len(sizes))]


def _pieces(buf, sizes, dts, frozen=None):
    """The vector `buf` (f32, the concatenation) as one tensor per spec, each an allocation of
    its own in dtype dts[i % len(dts)]; None for the frozen spec."""
    return [None if i == frozen else v.to(DT[dts[i % len(dts)]]).clone() for i, v in enumerate(_views(buf, sizes))]


def _widen(pieces, sizes, dev):
    """The f32 concatenation codec.project reads (a None entry: zeros)"""
    return torch.cat([torch.zeros(n, device=dev) if p is None else p.float() for p, n in zip(pieces, sizes)])


@functools.lru_cache(maxsize=None)
def _small_vec():
    """A dense vector every element of which is finite in f16 too (|x| < 30); a few are f16
    subnormals after the rounding."""
    dev = _dev()
    g = torch.Generator().manual_seed(77)
    total = sum(_sizes())
    v = torch.randn(total, generator=g) * 4.0
    v[::1000] *= 1e-5
    return v.to(dev)


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 33])
def test_one_f32_vector_as_views_of_one_buffer_equals_project(dtype, k):
    c = _case(dtype)
    buf = c["vec"].to(_dev())
    specs = _specs(dtype)
    got = _multi(specs, k, [_views(buf, c["sizes"])])
    assert np.array_equal(got[0], _project(specs, k, buf))


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)  # the tensors' dtype selects z; the vector's is its own
@pytest.mark.parametrize("vdt", [["bfloat16"], ["float16"], MIXED], ids=["bf16", "f16", "mixed"])
def test_two_byte_vectors_equal_project_on_their_widening(dtype, vdt):
    dev = _dev()
    sizes = _sizes()
    specs = _specs(dtype)
    pieces = _pieces(_small_vec(), sizes, vdt, frozen=FROZEN)
    if vdt == ["float16"]:
        assert any((p.float().abs() < 2.0 ** -14).logical_and(p != 0).any() for p in pieces if p is not None)
    got = _multi(specs, 33, [pieces])
    assert np.array_equal(got[0], _project(specs, 33, _widen(pieces, sizes, dev)))


# 3 ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _five_vectors():
    sizes = _sizes()
    base = _small_vec()
    out = []
    for m, dts in enumerate([["float32"], ["bfloat16"], MIXED, ["float16"], MIXED[1:] + MIXED[:1]]):
        out.append(_pieces(torch.roll(base, 1000 * m) * (1.0 + m), sizes, dts, frozen=FROZEN))
    return out


@functools.lru_cache(maxsize=None)
def _five_singles(dtype, k):
    return [_multi(_specs(dtype), k, [v])[0] for v in _five_vectors()]


@pytest.mark.parametrize("M", [2, 3, 4, 5])
@pytest.mark.parametrize("k", [1, 33])
def test_batching_invariance(M, k):
    _dev()
    got = _multi(_specs("bfloat16"), k, _five_vectors()[:M])
    want = _five_singles("bfloat16", k)
    assert len({w.tobytes() for w in want}) == 5, "five different vectors"
    for m in range(M):
        assert np.array_equal(got[m], want[m]), m


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdt", DTYPES)
@pytest.mark.parametrize("which", ["seven_tensors", "whole_16_byte_runs"])
def test_alignment_does_not_change_the_bits(vdt, which):
    """Every tensor's vector in an allocation of its own, one element in (4-byte or 2-byte
    aligned only: per-element loads), against 16-byte aligned copies (whole 16-byte runs
    wherever four runs lie inside the tensor -- all of the second list's first two rows)."""
    dev = _dev()
    if which == "seven_tensors":
        sizes, specs, k, frozen = _sizes(), _specs("bfloat16"), 33, FROZEN
        base = _small_vec()
    else:
        S = _stride(10**9)
        sizes, k, frozen = [8 * S + 1025, 1000], 2, None
        specs = _mixed_specs(["bfloat16", "float32"], sizes, dev)
        base = _dense_vec(sum(sizes), seed=41).clamp(-6e4, 6e4).to(dev)
    aligned = _pieces(base, sizes, [vdt], frozen=frozen)
    shifted = []
    for p in aligned:
        if p is None:
            shifted.append(None)
            continue
        q = torch.empty(p.numel() + 1, dtype=p.dtype, device=dev)[1:]
        q.copy_(p)
        assert q.is_contiguous() and q.data_ptr() % 16 == p.element_size() and p.data_ptr() % 16 == 0
        shifted.append(q)
    a = _multi(specs, k, [aligned])
    assert np.array_equal(a, _multi(specs, k, [shifted]))
    assert np.array_equal(a[0], _multi(specs, k, [aligned, shifted])[1])
    assert np.array_equal(a[0], _project(specs, k, _widen(aligned, sizes, dev)))


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_bf16_vector_is_exact(dtype):
    """float64(v) float64(z) at the probed element and nothing else: z as torch.normal draws
    it on the device (test_gpu_project._case), v = 2.71875 (exact in bf16)."""
    dev = _dev()
    c = _case(dtype)
    specs = _specs(dtype)
    pieces = [torch.zeros(n, dtype=torch.bfloat16, device=dev) for n in c["sizes"]]
    v = 2.71875
    assert float(torch.tensor(v).to(torch.bfloat16)) == v
    bad = []
    for pi in range(0, len(c["probes"]), 6):
        e = int(c["probes"][pi])
        ti = int(np.searchsorted(c["off"], e, side="right")) - 1
        pieces[ti][e - c["off"][ti]] = v
        got = _multi(specs, 33, [pieces])[0]
        pieces[ti][e - c["off"][ti]] = 0.0
        z = c["zp"][:33, pi]
        want = (np.float64(v) * z).view(np.int64) if c["live"][e] else np.zeros(33, np.int64)
        if c["live"][e]:
            assert (z != 0.0).all()
        if not np.array_equal(got, want):
            bad.append(e)
    assert not bad, f"elements that differ: {bad}"


# 6 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards(dtype, nshards):
    """Every shard's rows are codec.project's for that shard; the shards add up to the whole
    call within total 2^-52 sum|v z| (any f64 order of the exact products errs by less; the
    bf16 row's sum|v z| is at most (1 + 2^-8) times the f32 vector's, a rounding each)."""
    dev = _dev()
    c = _case(dtype)
    specs = _specs(dtype)
    k = 33
    buf = c["vec"].to(dev)
    rows = [_views(buf, c["sizes"]), _pieces(buf, c["sizes"], ["bfloat16"], frozen=FROZEN)]
    wide = [buf, _widen(rows[1], c["sizes"], dev)]
    whole = _multi(specs, k, rows).view(np.float64)
    parts = []
    for r in range(nshards):
        got = _multi(specs, k, rows, shard=r, nshards=nshards)
        for m in range(2):
            assert np.array_equal(got[m], _project(specs, k, wide[m], shard=r, nshards=nshards)), (r, m)
        parts.append(got.view(np.float64))
    for m, slack in ((0, 1.0), (1, 1.0 + 2.0 ** -8)):
        total = np.array([math.fsum(p[m, s] for p in parts) for s in range(k)])
        # U = 2^-52 is twice the unit roundoff: it covers the error of the whole call and the parts'
        err, bound = np.abs(total - whole[m]), c["n"] * U * c["sabs"][:k] * slack
        print(f"{dtype} nshards={nshards} row {m}: max err / bound = {float((err / bound).max()):.3e}")
        assert (err <= bound).all(), (err, bound)


# 7 ---------------------------------------------------------------------------------------------
def test_frozen_empty_and_no_vectors_or_seeds():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    sizes = _sizes()
    specs = _specs("bfloat16")
    pieces = _pieces(_small_vec(), sizes, MIXED, frozen=FROZEN)
    want = _multi(specs, 33, [pieces])
    # the frozen spec's entry is ignored: None, or any tensor
    other = list(pieces)
    other[FROZEN] = torch.full((11,), 7, dtype=torch.int32, device=dev)
    assert np.array_equal(_multi(specs, 33, [other]), want)
    # an empty tensor in the list draws nothing: the same bits
    sp = list(specs)
    sp.insert(4, codec.ParamSpec(torch.empty(0, dtype=torch.bfloat16, device=dev)))
    pe = list(pieces)
    pe.insert(4, torch.empty(0, dtype=torch.float16, device=dev))
    assert np.array_equal(_multi(sp, 33, [pe, pe])[1], want[0])
    # no vectors, no seeds
    none = codec.project_multi(specs, SEEDS, [], stream_mode="torch_rocm")
    assert none.dtype == torch.float64 and none.shape == (0, len(SEEDS))
    none = codec.project_multi(specs, [], [pieces, pieces], stream_mode="torch_rocm")
    assert none.dtype == torch.float64 and none.shape == (2, 0)
    # a list with no live element: +0 everywhere
    sp0 = [codec.ParamSpec(torch.empty(0, dtype=torch.float32, device=dev)),
           codec.ParamSpec(torch.empty(5, dtype=torch.float32, device=dev), frozen=True)]
    z = _multi(sp0, 33, [[torch.empty(0, device=dev), None]] * 3)
    assert np.array_equal(z, np.zeros((3, 33), np.int64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinity_poisons_its_own_row_only(dtype):
    c = _case(dtype)
    specs = _specs(dtype)
    k = 33
    sizes = c["sizes"]
    pi = next(i for i, e in enumerate(c["probes"].tolist())
              if e > c["off"][-2] + 4 * _stride(sizes[-1]) and (c["zp"][:k, i] != 0.0).all())
    e = int(c["probes"][pi]) - c["off"][-2]
    clean = [_pieces(_small_vec() * s, sizes, MIXED, frozen=FROZEN) for s in (1.0, -2.0, 0.5)]
    want = _multi(specs, k, clean)
    for inf in (float("inf"), float("-inf")):
        rows = [list(r) for r in clean]
        rows[1][-1] = rows[1][-1].clone()
        rows[1][-1][e] = inf
        got = _multi(specs, k, rows)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[1].view(np.float64), np.float64(inf) * np.sign(c["zp"][:k, pi]))


# 8 ---------------------------------------------------------------------------------------------
def test_overwrites_and_repeats():
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    sizes = _sizes()
    specs = _specs("float16")
    rows = _five_vectors()
    a = _multi(specs, 33, rows)
    assert np.array_equal(a, _multi(specs, 33, rows))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        d = codec.project_multi(specs, SEEDS, rows, stream_mode="torch_rocm")
    side.synchronize()
    assert np.array_equal(a, _i64(d))
    # the C call overwrites its output (here pre-filled with NaN), it does not accumulate
    L = N.load()
    batch = codec._Batch(specs, "torch_rocm", stage=False)
    M, nt, K = len(rows), len(sizes), len(SEEDS)
    varr = (N.FksVec * (M * nt))()
    for m, r in enumerate(rows):
        for i, p in enumerate(r):
            if p is not None:
                varr[m * nt + i].data = p.data_ptr()
                varr[m * nt + i].dtype = codec._DTYPES[p.dtype]
    seeds = np.array(SEEDS, dtype=np.uint64)
    out = torch.full((M, K), float("nan"), dtype=torch.float64, device=dev)
    nbytes = ctypes.c_size_t(0)
    N.check(L.fks_project_multi_workspace_size(ctypes.addressof(batch.arr), batch.n, K, M, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(L.fks_project_multi(ctypes.addressof(batch.arr), batch.n, seeds.ctypes.data, K, ctypes.addressof(varr), M, 0,
                                1, out.data_ptr(), ws.data_ptr(), nbytes.value, stream))
    assert np.array_equal(_i64(out), a)
    # ... also when the shard holds nothing (a list of empty and frozen tensors): zeroed
    out.fill_(float("nan"))
    sp0 = [codec.ParamSpec(torch.empty(0, dtype=torch.float16, device=dev)),
           codec.ParamSpec(torch.empty(5, dtype=torch.float16, device=dev), frozen=True)]
    b0 = codec._Batch(sp0, "torch_rocm", stage=False)
    v0 = (N.FksVec * (M * 2))()
    N.check(L.fks_project_multi(ctypes.addressof(b0.arr), b0.n, seeds.ctypes.data, K, ctypes.addressof(v0), M, 0, 1,
                                out.data_ptr(), None, 0, stream))
    assert np.array_equal(_i64(out), np.zeros((M, K), np.int64))


# 9 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["several_dtypes_in_one_wave", "table_longer_than_the_lds_copy"])
def test_other_table_shapes(which):
    dev = _dev()
    if which == "several_dtypes_in_one_wave":
        dts = ["bfloat16", "float32", "float16", "bfloat16", "float32", "float16", "float32"]
        sizes = [256, 1000, 100, 8, 200, 256, 4096]
    else:
        n = 600
        dts = [DTYPES[i % 3] for i in range(n)]
        sizes = [(7 * i) % 41 + 1 for i in range(n)]
    specs = _mixed_specs(dts, sizes, dev)
    base = (_dense_vec(sum(sizes), seed=31).clamp(-6e4, 6e4)).to(dev)
    rows = [_pieces(torch.roll(base, 7 * m), sizes, v) for m, v in enumerate([["float32"], MIXED, ["float16", "bfloat16"]])]
    got = _multi(specs, 33, rows)
    for m, r in enumerate(rows):
        assert np.array_equal(got[m], _project(specs, 33, _widen(r, sizes, dev))), m


# 10 --------------------------------------------------------------------------------------------
def test_seed_projections_multi_against_the_staged_path():
    from fate_llm.algo.fedkseed import zo_utils
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    shapes, dts, rg = [(5000,), (1000, 3), (300,)], ["bfloat16", "float32", "bfloat16"], [True, True, False]
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(DT[d]).to(dev), requires_grad=r)
              for s, d, r in zip(shapes, dts, rg)]
    for p in params[:2]:
        p.grad = torch.randn(p.shape, generator=g).to(p.dtype).to(dev)
    assert params[0].grad.dtype == torch.bfloat16
    groups = [{"params": params[:1], "lr": 1e-3, "weight_decay": 0.0}, {"params": params[1:], "lr": 1e-3, "weight_decay": 0.0}]
    seeds = SEEDS[:7]
    staged = zo_utils.seed_projections(groups, seeds, stream_mode="torch_rocm")
    torch.manual_seed(123)
    torch.rand(3)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    got = zo_utils.seed_projections_multi(groups, seeds, stream_mode="torch_rocm")
    other = [(params[0].grad * 3).float(), params[1].grad.double().t().contiguous().t(), None]  # staged copies of these only
    two = zo_utils.seed_projections_multi(groups, seeds, [[p.grad for p in params[:2]] + [None], other],
                                          stream_mode="torch_rocm")
    fit = zo_utils.fit_seed_scalars_multi(groups, seeds, [[p.grad for p in params[:2]] + [None]], stream_mode="torch_rocm")
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    assert got.dtype == torch.float64 and got.shape == (1, 7) and got.device.type == "cuda"
    assert np.array_equal(_i64(got)[0], _i64(staged))
    assert np.array_equal(_i64(two)[0], _i64(staged))
    assert np.array_equal(_i64(two)[1], _i64(zo_utils.seed_projections(groups, seeds, vectors=other, stream_mode="torch_rocm")))
    assert np.array_equal(_i64(two)[1], _i64(zo_utils.seed_projections_multi(groups, seeds, [other], stream_mode="torch_rocm"))[0])
    assert torch.equal(fit, got / float(sum(p.numel() for p in params[:2])))
    assert torch.equal(fit[0], zo_utils.fit_seed_scalars(groups, seeds, [p.grad for p in params[:2]] + [None],
                                                         stream_mode="torch_rocm"))


# 11 --------------------------------------------------------------------------------------------
def test_no_model_size_staging_buffer():
    """A condition, not a measurement: the staged path's f32 buffer alone is 4 x total bytes
    (11.6 MB here); the in-place call allocates its workspace, about 1 MiB per vector of the
    pass, and the 33 results."""
    dev = _dev()
    sizes = _sizes()
    total = sum(sizes)
    specs = _specs("bfloat16")
    pieces = _pieces(_small_vec(), sizes, ["bfloat16"], frozen=FROZEN)
    _multi(specs, 33, [pieces])  # the spec list's plan is built
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    from fate_llm.algo.fedkseed import codec
    out = codec.project_multi(specs, SEEDS, [pieces], stream_mode="torch_rocm")
    torch.cuda.synchronize(dev)
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f"peak rise {rise} bytes, staging buffer {4 * total} bytes")
    assert out.shape == (1, 33) and rise < 4 * total
