"""Seed-basis projection on the torch_rocm stream (fks_project, codec.project,
zo_utils.seed_projections / fit_seed_scalars): out[s] = <vec, z_s>.

The reference is torch itself on the same GPU, as for the rest of this stream: after
torch.manual_seed(s), torch.normal(0, 1, (n,), device, dtype) per tensor in order (frozen
ones drawn and dropped), converted to float64 on the host, and dotted with vec by math.fsum
of the products -- each exact in f64 (24 x 24 significand bits), so fsum returns the
correctly rounded exact value.

Bound of the dense tests: the kernel adds exact products in f64 in some fixed order; ANY
order of n terms errs by at most (n - 1) u sum|v z| (1 + O(n u)), u = 2^-53, so
|got - ref| <= n 2^-52 sum|v z| holds for every correct implementation (derived, not
tuned; sum|v z| is a numpy float64 sum, relative error ~1e-15).

The one-hot tests need no bound: with one non-zero element every other product is an exact
zero and the result must equal float64(v) float64(z_s[e]) bit for bit (the reference draws
checked non-zero at the probed elements, so no sign of a zero is in play).

Tensor list (cap = codec.rocm_grid_cap(), 2,048 on an MI355X): 4096 | 1000 | 3 (frozen) |
700,001 (capped stride 256 cap, a ragged last row) | 7 | 65536 | 4 256 cap + 1025 (one past
a full-grid loop iteration: j = 1 items); k = 1 and 33 (33 crosses the 32-seed pass)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
DTYPES = ["float32", "bfloat16", "float16"]
FROZEN = 2
_g = torch.Generator().manual_seed(20261020)
SEEDS = [0, 2**32 - 1, 2**40 + 3] + torch.randint(0, 2**32, (30,), generator=_g).tolist()  # 33
U = 2.0 ** -52


def _sizes():
    from fate_llm.algo.fedkseed import codec
    cap = codec.rocm_grid_cap()
    return [4096, 1000, 3, 700_001, 7, 65536, 4 * 256 * cap + 1025]


def _offsets(sizes):
    return [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]


def _stride(n):
    from fate_llm.algo.fedkseed import codec
    return 256 * min((n + 255) // 256, codec.rocm_grid_cap())


def _probes(sizes):
    """Concatenation indices to probe: per tensor its first and last element, both sides of
    every boundary between runs of one stride (the element index i of an item changes there)
    and of the row boundary 4 stride (j changes), elements of the last, ragged item group, and
    for the big tensor its j = 1 elements."""
    off = _offsets(sizes)
    out = []
    for i, n in enumerate(sizes):
        S = _stride(n)
        local = {0, n - 1, n - 2, n - 8, n - 9}
        for b in (S, 2 * S, 3 * S, 4 * S):
            local |= {b - 1, b, b + 5}
        if n > 4 * S:
            local |= {4 * S + 255, 4 * S + 256, 4 * S + 1024, n - 1}
        out += [off[i] + e for e in sorted(local) if 0 <= e < n]
    return out


def _specs(dtype, sizes=None, dev=None):
    from fate_llm.algo.fedkseed import codec
    sizes = _sizes() if sizes is None else sizes
    dev = _dev() if dev is None else dev
    return [codec.ParamSpec(torch.empty(n, dtype=DT[dtype], device=dev), frozen=(i == FROZEN))
            for i, n in enumerate(sizes)]


def _draw(dtype, sizes, seed, dev):
    """float64 z of one seed over the concatenation, as the reference draws it"""
    torch.manual_seed(seed)
    z = [torch.normal(mean=0, std=1, size=(n,), device=dev, dtype=DT[dtype]) for n in sizes]
    return torch.cat([t.float() for t in z]).cpu().numpy().astype(np.float64)


def _dense_vec(total, seed=5):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(total, generator=g)
    big = torch.rand(total, generator=g) < 0.01
    return torch.where(big, v * 1e6, v)


@functools.lru_cache(maxsize=None)
def _case(dtype):
    """Computed once per dtype and shared: the dense vector, and per seed the reference
    projection, sum|v z| and the reference z at the probed elements."""
    dev = _dev()
    sizes = _sizes()
    off = _offsets(sizes)
    live = np.ones(off[-1], bool)
    live[off[FROZEN]:off[FROZEN + 1]] = False
    vec = _dense_vec(off[-1])
    v64 = vec.numpy().astype(np.float64)
    probes = np.array(_probes(sizes))
    ref, sabs, zp = [], [], []
    for s in SEEDS:
        z = _draw(dtype, sizes, s, dev)
        p = (v64 * z)[live]  # exact products
        ref.append(math.fsum(p.tolist()))
        sabs.append(float(np.abs(p).sum()))
        zp.append(z[probes].copy())
    return {"sizes": sizes, "off": off, "vec": vec, "ref": np.array(ref), "sabs": np.array(sabs),
            "n": int(live.sum()), "probes": probes, "zp": np.array(zp), "live": live}


def _i64(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 33])
def test_dense_projection_within_f64_sum_bound(dtype, k):
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    got = codec.project(_specs(dtype), SEEDS[:k], c["vec"].to(dev), stream_mode="torch_rocm")
    assert got.dtype == torch.float64 and got.shape == (k,) and got.device.type == "cuda"
    got = got.cpu().numpy()
    err, bound = np.abs(got - c["ref"][:k]), c["n"] * U * c["sabs"][:k]
    print(f"{dtype} k={k}: max |got - ref| / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 33])
def test_one_hot_is_exact(dtype, k):
    """Pins the element-to-counter mapping and the dtype rounding of z: a dropped, doubled or
    misplaced element shows here."""
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    specs = _specs(dtype)
    vec = torch.zeros(c["off"][-1], dtype=torch.float32, device=dev)
    v = float(np.float32(-3.1415927))
    bad = []
    for pi, e in enumerate(c["probes"].tolist()):
        vec[e] = v
        got = _i64(codec.project(specs, SEEDS[:k], vec, stream_mode="torch_rocm"))
        vec[e] = 0.0
        z = c["zp"][:k, pi]
        if c["live"][e]:
            assert (z != 0.0).all(), "probe an element whose reference z is non-zero"
            want = (np.float64(v) * z).view(np.int64)
        else:
            want = np.zeros(k, np.int64)  # the frozen tensor: exactly +0
        if not np.array_equal(got, want):
            bad.append((e, int((got != want).sum())))
    assert not bad, f"(element, seeds that differ): {bad}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_and_empty_tensors(dtype):
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    off, sizes = c["off"], c["sizes"]
    # non-zero only over the frozen tensor's range: nothing
    vec = torch.zeros(off[-1], dtype=torch.float32, device=dev)
    vec[off[FROZEN]:off[FROZEN + 1]] = 7.5
    got = _i64(codec.project(_specs(dtype), SEEDS, vec, stream_mode="torch_rocm"))
    assert np.array_equal(got, np.zeros(len(SEEDS), np.int64))
    # an empty tensor in the list draws nothing and has no range in vec: the same bits
    dense = c["vec"].to(dev)
    whole = _i64(codec.project(_specs(dtype), SEEDS, dense, stream_mode="torch_rocm"))
    sp = _specs(dtype)
    sp.insert(4, codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)))
    assert np.array_equal(_i64(codec.project(sp, SEEDS, dense, stream_mode="torch_rocm")), whole)
    # no seeds: an empty float64 tensor
    none = codec.project(_specs(dtype), [], dense, stream_mode="torch_rocm")
    assert none.dtype == torch.float64 and none.numel() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards(dtype, nshards):
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    specs = _specs(dtype)
    k = 33
    dense = c["vec"].to(dev)
    parts = [codec.project(specs, SEEDS[:k], dense, stream_mode="torch_rocm", shard=r, nshards=nshards).cpu().numpy()
             for r in range(nshards)]
    total = np.array([math.fsum(p[s] for p in parts) for s in range(k)])
    err, bound = np.abs(total - c["ref"][:k]), c["n"] * U * c["sabs"][:k]
    assert (err <= bound).all(), (err, bound)
    # one-hot: the shard that owns the element returns the whole call's value, the others +0
    ranges = [codec.shard_range(specs, r, nshards, stream_mode="torch_rocm") for r in range(nshards)]
    assert ranges[0][0] == 0 and ranges[-1][1] == c["off"][-1]
    vec = torch.zeros(c["off"][-1], dtype=torch.float32, device=dev)
    edges = [e for lo, hi in ranges for e in (lo, hi - 1)]
    for e in sorted(set(edges + c["probes"][::7].tolist())):
        if not c["live"][e]:
            continue
        vec[e] = 1.75
        whole = _i64(codec.project(specs, SEEDS[:k], vec, stream_mode="torch_rocm"))
        assert whole.any()
        for r, (lo, hi) in enumerate(ranges):
            got = _i64(codec.project(specs, SEEDS[:k], vec, stream_mode="torch_rocm", shard=r, nshards=nshards))
            want = whole if lo <= e < hi else np.zeros(k, np.int64)
            assert np.array_equal(got, want), (e, r, lo, hi)
        vec[e] = 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_and_overwrites(dtype):
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    specs = _specs(dtype)
    dense = c["vec"].to(dev)
    a = _i64(codec.project(specs, SEEDS, dense, stream_mode="torch_rocm"))
    b = _i64(codec.project(specs, SEEDS, dense, stream_mode="torch_rocm"))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        d = codec.project(specs, SEEDS, dense, stream_mode="torch_rocm")
    side.synchronize()
    assert np.array_equal(a, b) and np.array_equal(a, _i64(d))
    # the C call overwrites its output (here pre-filled with NaN), it does not accumulate
    L = N.load()
    batch = codec._Batch(specs, "torch_rocm")
    seeds = np.array(SEEDS, dtype=np.uint64)
    out = torch.full((len(SEEDS),), float("nan"), dtype=torch.float64, device=dev)
    nbytes = ctypes.c_size_t(0)
    N.check(L.fks_project_workspace_size(ctypes.addressof(batch.arr), batch.n, len(SEEDS), ctypes.byref(nbytes)))
    assert nbytes.value > 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    N.check(L.fks_project(ctypes.addressof(batch.arr), batch.n, seeds.ctypes.data, len(SEEDS), dense.data_ptr(), 0, 1,
                          out.data_ptr(), ws.data_ptr(), nbytes.value, torch.cuda.current_stream(dev).cuda_stream))
    assert np.array_equal(_i64(out), a)
    # ... also when the shard holds nothing (a list of empty and frozen tensors): zeroed
    out.fill_(float("nan"))
    sp0 = [codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)),
           codec.ParamSpec(torch.empty(5, dtype=DT[dtype], device=dev), frozen=True)]
    b0 = codec._Batch(sp0, "torch_rocm")
    v0 = torch.ones(5, dtype=torch.float32, device=dev)
    N.check(L.fks_project(ctypes.addressof(b0.arr), b0.n, seeds.ctypes.data, len(SEEDS), v0.data_ptr(), 0, 1,
                          out.data_ptr(), None, 0, torch.cuda.current_stream(dev).cuda_stream))
    assert np.array_equal(_i64(out), np.zeros(len(SEEDS), np.int64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_adjoint_of_delta_accumulate(dtype):
    """<Z c, v> = <c, Z^T v>.  delta_accumulate rounds every element's K fmas to f32 -- the
    only inexact step: |delta_e - sum_s f32(c_s) z_s(e)| <= K 2^-24 sum_s |f32(c_s) z_s(e)|
    (K roundings, each at most 2^-24 of a partial sum that the absolute sum bounds) -- and
    the projection errs by the dense bound per seed."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    sizes = sorted(_sizes())[:3]  # 3, 7, 1000
    K = 5
    seeds = SEEDS[3:3 + K]
    g = torch.Generator().manual_seed(9)
    coefs = (torch.randn(K, generator=g, dtype=torch.float64) * 3).tolist()
    c32 = np.array(coefs, dtype=np.float32).astype(np.float64)
    specs = [codec.ParamSpec(torch.empty(n, dtype=DT[dtype], device=dev)) for n in sizes]
    total = sum(sizes)
    v = _dense_vec(total, seed=13)
    v64 = v.numpy().astype(np.float64)
    delta = torch.zeros(total, dtype=torch.float32, device=dev)
    codec.delta_accumulate(specs, seeds, coefs, delta, stream_mode="torch_rocm")
    proj = codec.project(specs, seeds, v.to(dev), stream_mode="torch_rocm").cpu().numpy()
    lhs = math.fsum((delta.cpu().numpy().astype(np.float64) * v64).tolist())  # exact products
    rhs = math.fsum((c32 * proj).tolist())
    z = np.stack([_draw(dtype, sizes, s, dev) for s in seeds])  # [K, total]
    bound = K * 2.0 ** -24 * float((np.abs(v64) * (np.abs(c32)[:, None] * np.abs(z)).sum(0)).sum())
    bound += float((np.abs(c32) * total * U * np.abs(v64 * z).sum(1)).sum())
    print(f"{dtype}: |lhs - rhs| / bound = {abs(lhs - rhs) / bound:.3e}")
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_vector(dtype):
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    specs = _specs(dtype)
    k = 33
    # an element of the big tensor's second row whose reference z is non-zero for every seed
    pi = next(i for i, e in enumerate(c["probes"].tolist())
              if e > c["off"][-2] + 4 * _stride(c["sizes"][-1]) and (c["zp"][:k, i] != 0.0).all())
    e = int(c["probes"][pi])
    dense = c["vec"].to(dev)
    dense[e] = float("nan")
    got = codec.project(specs, SEEDS[:k], dense, stream_mode="torch_rocm").cpu().numpy()
    assert np.isnan(got).all()
    for inf in (float("inf"), float("-inf")):
        vec = torch.zeros(c["off"][-1], dtype=torch.float32, device=dev)
        vec[e] = inf
        got = codec.project(specs, SEEDS[:k], vec, stream_mode="torch_rocm").cpu().numpy()
        assert np.array_equal(got, np.float64(inf) * np.sign(c["zp"][:k, pi]))


def test_zo_utils_seed_projections_and_fit():
    from fate_llm.algo.fedkseed import zo_utils
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    shapes, dts, rg = [(5000,), (1000, 3), (300,)], ["bfloat16", "float32", "bfloat16"], [True, True, False]
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(DT[d]).to(dev), requires_grad=r)
              for s, d, r in zip(shapes, dts, rg)]
    for p in params[:2]:
        p.grad = torch.randn(p.shape, generator=g).to(p.dtype).to(dev)
    groups = [{"params": params[:1], "lr": 1e-3, "weight_decay": 0.0}, {"params": params[1:], "lr": 1e-3, "weight_decay": 0.0}]
    seeds = SEEDS[:7]
    # explicit reference: every parameter draws in its own dtype, the frozen one is dropped
    ref, sabs = [], []
    for s in seeds:
        torch.manual_seed(s)
        z = [torch.normal(mean=0, std=1, size=p.shape, device=dev, dtype=p.dtype) for p in params]
        prod = np.concatenate([(p.grad.float().cpu().numpy().astype(np.float64) *
                                t.float().cpu().numpy().astype(np.float64)).reshape(-1)
                               for p, t in zip(params[:2], z[:2])])
        ref.append(math.fsum(prod.tolist()))
        sabs.append(float(np.abs(prod).sum()))
    n = sum(p.numel() for p in params[:2])
    bound = n * U * np.array(sabs)
    torch.manual_seed(123)
    torch.rand(3)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    got = zo_utils.seed_projections(groups, seeds, stream_mode="torch_rocm")
    fit = zo_utils.fit_seed_scalars(groups, seeds, [p.grad for p in params[:2]] + [None], stream_mode="torch_rocm")
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    assert got.dtype == torch.float64 and got.device.type == "cuda"
    assert (np.abs(got.cpu().numpy() - np.array(ref)) <= bound).all()
    assert torch.equal(fit, got / float(n))
    assert (np.abs(fit.cpu().numpy() - np.array(ref) / n) <= bound / n * (1 + 2.0 ** -50)).all()
    # explicit vectors of another float dtype are read as f32
    same = zo_utils.seed_projections(groups, seeds, vectors=[params[0].grad.float(), params[1].grad.double(), None],
                                     stream_mode="torch_rocm")
    assert torch.equal(same, got)
    params[1].grad = None
    with pytest.raises(ValueError, match="grad"):
        zo_utils.seed_projections(groups, seeds, stream_mode="torch_rocm")


# ---------------------------------------------------------------- paths the list above never takes
# The issue's list leaves three branches of the kernel unvisited: with cap = 2048 its only
# tensor long enough for whole 16-byte runs (four strides plus eight elements) starts at
# element 770,643 of the vector, 12 bytes past a 16-byte boundary, so every group there loads
# element by element; every list has one dtype; and no table has more than 512 entries.  The
# lists below reach them, against the same reference and the same bound.
def _reference(dts, sizes, vec, seeds, probes, dev):
    """Per seed: z at the probes and, with a vec, the fsum projection and sum|v z|; tensor i
    draws dtype dts[i]."""
    v64 = None if vec is None else vec.numpy().astype(np.float64)
    idx = torch.as_tensor(probes, device=dev)
    ref, sabs, zp = [], [], []
    for s in seeds:
        torch.manual_seed(s)
        z = [torch.normal(mean=0, std=1, size=(n,), device=dev, dtype=DT[d]) for d, n in zip(dts, sizes)]
        z = torch.cat([t.float() for t in z])
        zp.append(z[idx].cpu().numpy().astype(np.float64))
        if v64 is not None:
            p = v64 * z.cpu().numpy().astype(np.float64)  # exact products
            ref.append(math.fsum(p.tolist()))
            sabs.append(float(np.abs(p).sum()))
    return np.array(ref), np.array(sabs), np.array(zp)


def _mixed_specs(dts, sizes, dev):
    from fate_llm.algo.fedkseed import codec
    return [codec.ParamSpec(torch.empty(n, dtype=DT[d], device=dev)) for d, n in zip(dts, sizes)]


def _check_dense_and_one_hot(dts, sizes, probes, k_dense, dev):
    """Dense within the f64-sum bound for SEEDS[:k_dense]; one-hot bit-exact at every probe for
    all 33 seeds."""
    from fate_llm.algo.fedkseed import codec
    total = sum(sizes)
    probes = np.array(sorted(set(probes)))
    assert probes.min() >= 0 and probes.max() < total
    vec = _dense_vec(total, seed=31)
    ref, sabs, _ = _reference(dts, sizes, vec, SEEDS[:k_dense], probes, dev)
    specs = _mixed_specs(dts, sizes, dev)
    dvec = vec.to(dev)
    assert dvec.data_ptr() % 16 == 0
    got = codec.project(specs, SEEDS[:k_dense], dvec, stream_mode="torch_rocm").cpu().numpy()
    err, bound = np.abs(got - ref), total * U * sabs
    print(f"dense: max |got - ref| / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all(), (err, bound)
    _, _, zp = _reference(dts, sizes, None, SEEDS, probes, dev)
    assert (zp != 0.0).all(), "probe elements whose reference z is non-zero"
    dvec.zero_()
    v = float(np.float32(2.7182817))
    bad = []
    for pi, e in enumerate(probes.tolist()):
        dvec[e] = v
        g = _i64(codec.project(specs, SEEDS, dvec, stream_mode="torch_rocm"))
        dvec[e] = 0.0
        if not np.array_equal(g, (np.float64(v) * zp[:, pi]).view(np.int64)):
            bad.append(e)
    assert not bad, f"elements that differ: {bad}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_16_byte_runs(dtype):
    """The path every model tensor takes: a tensor of eight strides and a ragged third row
    at a 16-byte aligned vector offset (first in the list), so rows j = 0 and j = 1 load
    whole 16-byte runs and row 2 element by element.  Probes in both whole rows, in each of
    the four runs, at the run's first group, both sides of a group and a lane boundary, and
    its last element; the ragged row; the unaligned tensor behind."""
    dev = _dev()
    S = _stride(10**9)  # the capped stride, 256 cap
    sizes = [8 * S + 1025, 1000]
    probes = [8 * S, 8 * S + 1024, sizes[0], sizes[0] + 999]
    for j in (0, 1):
        for i in range(4):
            base = S * (4 * j + i)
            probes += [base + x for x in (0, 3, 7, 8, 15, 511, 512, 4093, S // 2 + 5, S - 9, S - 1)]
    _check_dense_and_one_hot([dtype, dtype], sizes, probes, 2, dev)


def test_several_dtypes_in_one_wave():
    """Tensors of at most 256 elements have 256 items, half a wave's 64 groups of eight: a
    wave that spans two or three of them of different dtypes runs one pass per dtype."""
    dev = _dev()
    dts = ["bfloat16", "float32", "float16", "bfloat16", "float32", "float16", "float32"]
    sizes = [256, 1000, 100, 8, 200, 256, 4096]
    off = _offsets(sizes)
    probes = [o + x for o, n in zip(off, sizes) for x in (0, 1, n // 2, n - 1) if 0 <= x < n]
    _check_dense_and_one_hot(dts, sizes, probes, 33, dev)


def test_table_longer_than_the_lds_copy():
    """600 entries: the kernel reads the tensor table from device memory (more than 512)."""
    dev = _dev()
    n = 600
    dts = [DTYPES[i % 3] for i in range(n)]
    sizes = [(7 * i) % 41 + 1 for i in range(n)]
    off = _offsets(sizes)
    probes = [0, off[1] - 1, off[300], off[511], off[512], off[513] + 1, off[599], off[600] - 1]
    _check_dense_and_one_hot(dts, sizes, probes, 33, dev)


def test_non_contiguous_specs_are_not_staged():
    """project never reads the parameters: a non-contiguous spec gets no staging copy (its
    own address keys the plan) and the result is that of a contiguous spec of its size."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    base = torch.empty(64, 100, dtype=torch.bfloat16, device=dev)
    view = base[:, :50]
    assert not view.is_contiguous()
    vec = _dense_vec(view.numel(), seed=3).to(dev)
    b = codec._Batch([codec.ParamSpec(view)], "torch_rocm", stage=False)
    assert not b.copies and b.arr[0].data == view.data_ptr()
    got = codec.project([codec.ParamSpec(view)], SEEDS[:3], vec, stream_mode="torch_rocm")
    want = codec.project([codec.ParamSpec(torch.empty(view.numel(), dtype=torch.bfloat16, device=dev))], SEEDS[:3], vec,
                         stream_mode="torch_rocm")
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
