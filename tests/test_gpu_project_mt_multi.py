"""Seed-basis projection of several vectors read in place on the torch_cpu stream
(fks_project_mt_multi, codec.project_mt_multi, zo_utils.seed_projections_in_place /
fit_seed_scalars_in_place).

The centre is the bit-for-bit rule of include/fks.h: row m of any call equals the one-vector call
on vector m, and a one-vector call on f32 entries lying end to end in one buffer equals
fks_project_mt on that buffer -- for every k, shard and dtype, whatever the vectors' dtype (widened
to f32 exactly) and alignment.  So almost every test compares int64 views (NaN payloads included)
with codec.project_mt, whose own values test_gpu_project_mt.py pins to the reference stream and to
a recorded commit's bits; one test goes to the reference stream on its own: torch's CPU draws,
math.fsum of the exact products, and the derived bound n 2^-52 sum|v z| of that file.

The tensor list, the seeds and the pass shapes are test_gpu_project_mt.py's (the smallest list
that reaches every branch of the two kernels); k = 19 and 20 also cross the two-vector pass's
10 seeds, and codec.PROJECT_MT_PASS_VECTORS + 1 vectors reach the host-side batching."""
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import _dev
from test_gpu_project_mt import (DT, DTYPES, FROZEN, KS, SEEDS, SIZES, U, _case, _dense_vec, _draw, _i64, _offsets,
                                 _probes, _specs)

pytestmark = pytest.mark.gpu

VDT = [torch.float32, torch.bfloat16, torch.float16]


def _max_vec():
    from fate_llm.algo.fedkseed import codec
    return codec.PROJECT_MT_PASS_VECTORS


def _buffers(M, dev, scale=1.0):
    """M different dense f32 concatenation buffers on the device"""
    dense = _dense_vec(_offsets(SIZES)[-1])  # test_gpu_project_mt.py's dense vector
    return [(torch.roll(dense, 1000 * m) * (scale * (1 + m))).to(dev) for m in range(M)]


def _views(buf, off=None):
    """the per-spec f32 views of one concatenation buffer (None for the frozen spec)"""
    off = off or _offsets(SIZES)
    return [None if i == FROZEN else buf[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _off_boundary(values, dtype, dev):
    """`values` as a contiguous tensor of `dtype` that starts one element past a 16-byte boundary"""
    store = torch.empty(values.numel() + 9, dtype=dtype, device=dev)
    view = store[1:1 + values.numel()]
    view.copy_(values)
    if values.numel():  # (an empty view has no address)
        assert store.data_ptr() % 16 == 0 and view.data_ptr() % 16 == view.element_size() and view.is_contiguous()
    return view


# ---------------------------------------------------------------- 1. bitwise against project_mt
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", KS)
def test_rows_equal_project_mt_bit_for_bit(dtype, k):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs(dtype)
    cap = _max_vec()
    bufs = _buffers(cap + 1, dev)
    want = [_i64(codec.project_mt(specs, SEEDS[:k], b)) for b in bufs]
    for M in sorted({1, 2, cap, cap + 1}):  # cap + 1 reaches the host-side batching
        got = codec.project_mt_multi(specs, SEEDS[:k], [_views(b) for b in bufs[:M]])
        assert got.dtype == torch.float64 and got.shape == (M, k) and got.device.type == "cuda"
        got = _i64(got)
        for m in range(M):
            assert np.array_equal(got[m], want[m]), (M, m, np.nonzero(got[m] != want[m])[0].tolist())


# ---------------------------------------------------------------- 2. vector dtype and alignment
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("vdt", ["bfloat16", "float16", "mixed"])
def test_vector_dtype_and_alignment(dtype, vdt):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs(dtype)
    off = _offsets(SIZES)
    k = 20
    lists, want = [], []
    for m, buf in enumerate(_buffers(2, dev, scale=1e-2)):  # |v| < 65504: finite as f16 too
        buf = buf.clamp(-6e4, 6e4)
        vs, wide = [], torch.zeros_like(buf)
        for i, v in enumerate(_views(buf)):
            if v is None:
                vs.append(None)
                continue
            t = DT[vdt] if vdt != "mixed" else VDT[(i + m) % 3]
            x = _off_boundary(v, t, dev)
            wide[off[i]:off[i + 1]] = x.float()  # the same values, widened exactly
            vs.append(x)
        lists.append(vs)
        want.append(_i64(codec.project_mt(specs, SEEDS[:k], wide)))
    if vdt == "mixed":
        assert {v.dtype for v in lists[0] if v is not None} == set(VDT)
    got = _i64(codec.project_mt_multi(specs, SEEDS[:k], lists))
    for m in range(2):
        assert np.array_equal(got[m], want[m]), (m, np.nonzero(got[m] != want[m])[0].tolist())


def test_non_contiguous_and_float64_vectors_equal_their_f32_copies():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs("bfloat16")
    buf = _buffers(1, dev)[0]
    plain = _views(buf)
    strided, f64 = [], []
    for v in plain:
        if v is None:
            strided.append(None)
            f64.append(None)
            continue
        wide = torch.empty(2 * v.numel(), dtype=torch.float32, device=dev)
        wide[::2] = v
        strided.append(wide[::2])
        f64.append(v.double())
    assert not strided[0].is_contiguous()
    got = _i64(codec.project_mt_multi(specs, SEEDS, [strided, f64, plain]))
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[2])
    assert np.array_equal(got[2], _i64(codec.project_mt(specs, SEEDS, buf)))


# ---------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_independent(dtype):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs(dtype)
    off = _offsets(SIZES)
    M = _max_vec()
    bufs = _buffers(M, dev)
    lists = [_views(b) for b in bufs]
    whole = _i64(codec.project_mt_multi(specs, SEEDS, lists))
    for m in range(M):  # row m of the M-vector call is the one-vector call on vector m
        assert np.array_equal(whole[m], _i64(codec.project_mt_multi(specs, SEEDS, [lists[m]]))[0]), m
    # NaN / inf in one vector (a fast element, an irregular one, a serial one) reach no other row
    bad = bufs[1].clone()
    probes = _probes(SIZES, dev)
    fast = next(e for e in probes if e > 624)
    irr = next(e for e in probes if e > off[5])
    tiny = off[4] + 2
    bad[fast], bad[irr], bad[tiny] = float("nan"), float("inf"), float("-inf")
    got = _i64(codec.project_mt_multi(specs, SEEDS, [lists[0], _views(bad)] + lists[2:]))
    for m in range(M):
        if m != 1:
            assert np.array_equal(got[m], whole[m]), m
    assert np.array_equal(got[1], _i64(codec.project_mt(specs, SEEDS, bad)))  # NaN payloads as bits
    assert np.isnan(got[1].view(np.float64)).all()


# ---------------------------------------------------------------- 4. shards
@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_equal_project_mt(dtype):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs(dtype)
    bufs = _buffers(2, dev)
    k, nshards = 20, 3
    for r in range(nshards):
        got = _i64(codec.project_mt_multi(specs, SEEDS[:k], [_views(b) for b in bufs], shard=r, nshards=nshards))
        for m, b in enumerate(bufs):
            want = _i64(codec.project_mt(specs, SEEDS[:k], b, shard=r, nshards=nshards))
            assert np.array_equal(got[m], want), (r, m)


def test_mixed_dtype_spec_list():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    dts = ["bfloat16", "float32", "float16", "bfloat16", "float32"]
    sizes = [1 << 18, 4096, 4096, 1000, 5]
    off = _offsets(sizes)
    specs = [codec.ParamSpec(torch.empty(n, dtype=DT[d], device=dev)) for d, n in zip(dts, sizes)]
    k = 20
    bufs = [(_dense_vec(off[-1], seed=31 + m)).to(dev) for m in range(3)]
    lists = [[b[off[i]:off[i + 1]] for i in range(len(sizes))] for b in bufs]
    got = _i64(codec.project_mt_multi(specs, SEEDS[:k], lists))
    for m, b in enumerate(bufs):
        assert np.array_equal(got[m], _i64(codec.project_mt(specs, SEEDS[:k], b))), m
    for r in range(3):
        got = _i64(codec.project_mt_multi(specs, SEEDS[:k], lists, shard=r, nshards=3))
        for m, b in enumerate(bufs):
            assert np.array_equal(got[m], _i64(codec.project_mt(specs, SEEDS[:k], b, shard=r, nshards=3))), (r, m)


# ---------------------------------------------------------------- 5. against the reference stream
def test_bf16_in_place_against_the_reference_stream():
    """bf16 specs, bf16 vectors read in place: torch's CPU draws, math.fsum of the exact products
    (each vector element is a bf16 value, each z a bf16 value: exact in f64), the derived bound
    n 2^-52 sum|v z| -- no other projection call enters."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs("bfloat16")
    c = _case("bfloat16")
    off, live = c["off"], c["live"]
    k = 13  # two vectors: a full 10-seed pass and a partial one
    vals = [(torch.roll(c["vec"], 777 * m) * (1 + m)).bfloat16() for m in range(2)]  # CPU, bf16 values
    lists = [[None if i == FROZEN else v[off[i]:off[i + 1]].to(dev) for i in range(len(SIZES))] for v in vals]
    assert all(t.dtype == torch.bfloat16 for t in lists[0] if t is not None)
    got = codec.project_mt_multi(specs, SEEDS[:k], lists).cpu().numpy()
    v64 = [v.float().numpy().astype(np.float64) for v in vals]
    n = int(live.sum())
    for s in range(k):
        z = _draw(["bfloat16"] * len(SIZES), SIZES, SEEDS[s])  # once per seed for both vectors
        for m in range(2):
            p = (v64[m] * z)[live]
            ref, bound = math.fsum(p.tolist()), n * U * float(np.abs(p).sum())
            assert abs(got[m, s] - ref) <= bound, (m, s, got[m, s], ref, bound)


def test_bf16_one_hot_is_exact():
    """every third probe of test_gpu_project_mt.py, one probe per vector of a call: the result is
    float64(v) float64(z) exactly -- the element-to-word mapping of the in-place tables"""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs("bfloat16")
    c = _case("bfloat16")
    off, live = c["off"], c["live"]
    assert np.array_equal(c["probes"], np.array(_probes(SIZES, dev)))
    probes, zp = c["probes"][::3].tolist(), c["zp"][:, ::3]
    v = float(torch.tensor(-3.1415927).bfloat16())
    M = _max_vec()
    tensors = [[None if i == FROZEN else torch.zeros(n, dtype=torch.bfloat16, device=dev)
                for i, n in enumerate(SIZES)] for _ in range(M)]
    bad = []
    for p0 in range(0, len(probes), M):
        batch = probes[p0:p0 + M]
        where = []
        for m, e in enumerate(batch):
            i = max(j for j in range(len(SIZES)) if off[j] <= e and SIZES[j])
            where.append((m, i, e - off[i]))
            if i != FROZEN:
                tensors[m][i][e - off[i]] = v
        got = codec.project_mt_multi(specs, SEEDS, tensors[:len(batch)]).cpu().numpy()
        for m, i, j in where:
            if i != FROZEN:
                tensors[m][i][j] = 0.0
            e = batch[m]
            want = np.float64(v) * zp[:, p0 + m] if live[e] else np.zeros(len(SEEDS))
            if not np.array_equal(got[m], want):  # bit for bit but for the sign of a zero
                bad.append((e, int((got[m] != want).sum())))
    assert not bad, f"(element, seeds that differ): {bad}"


# ---------------------------------------------------------------- 6. libm flavour
def test_libm_flavour_equals_project_mt():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs("float32")
    bufs = _buffers(2, dev)
    default = _i64(codec.project_mt_multi(specs, SEEDS, [_views(b) for b in bufs]))
    codec.set_cpu_fp32_flavour("libm")
    try:
        assert codec.cpu_fp32_flavour() == "libm"
        got = _i64(codec.project_mt_multi(specs, SEEDS, [_views(b) for b in bufs]))
        want = [_i64(codec.project_mt(specs, SEEDS, b)) for b in bufs]
    finally:
        codec.set_cpu_fp32_flavour(None)
    for m in range(2):
        assert np.array_equal(got[m], want[m]), m
    if codec.cpu_fp32_flavour() != "libm":  # the two flavours' z differ: so do their projections
        assert (got != default).any()


# ---------------------------------------------------------------- 7. zo_utils
def test_zo_utils_in_place_forms():
    from fate_llm.algo.fedkseed import zo_utils
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    shapes, dts, rg = [(5000,), (1000, 3), (300,)], ["bfloat16", "float32", "bfloat16"], [True, True, False]
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(DT[d]).to(dev), requires_grad=r)
              for s, d, r in zip(shapes, dts, rg)]
    for p in params[:2]:
        p.grad = torch.randn(p.shape, generator=g).to(p.dtype).to(dev)
    groups = [{"params": params[:1], "lr": 1e-3, "weight_decay": 0.0},
              {"params": params[1:], "lr": 1e-3, "weight_decay": 0.0}]
    seeds = SEEDS[:7]
    n = sum(p.numel() for p in params[:2])
    torch.manual_seed(123)
    torch.rand(3)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    got = zo_utils.seed_projections_in_place(groups, seeds, stream_mode="torch_cpu")
    lists = [[p.grad for p in params[:2]] + [None], [2 * p.grad for p in params[:2]] + [None]]
    fit = zo_utils.fit_seed_scalars_in_place(groups, seeds, lists, stream_mode="torch_cpu")
    rocm = zo_utils.seed_projections_in_place(groups, seeds, stream_mode="torch_rocm")
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    assert got.dtype == torch.float64 and got.shape == (1, len(seeds)) and got.device.type == "cuda"
    # torch_cpu: the staged form's bits; torch_rocm: the torch_rocm in-place form's bits
    assert np.array_equal(_i64(got[0]), _i64(zo_utils.seed_projections(groups, seeds, stream_mode="torch_cpu")))
    assert np.array_equal(_i64(rocm), _i64(zo_utils.seed_projections_multi(groups, seeds, stream_mode="torch_rocm")))
    assert not torch.equal(rocm, got)  # another stream
    # the fit is the projection / N
    proj = zo_utils.seed_projections_in_place(groups, seeds, lists, stream_mode="torch_cpu")
    assert fit.shape == (2, len(seeds)) and torch.equal(fit, proj / float(n))
    assert np.array_equal(_i64(proj[0]), _i64(got[0]))
    # the default-.grad path raises on a missing grad
    params[1].grad = None
    with pytest.raises(ValueError, match="grad"):
        zo_utils.seed_projections_in_place(groups, seeds, stream_mode="torch_cpu")
