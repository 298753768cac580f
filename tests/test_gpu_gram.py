"""Seed-basis Gram matrix on the torch_rocm stream (fks_gram, codec.gram, zo_utils.seed_gram /
fit_seed_scalars_exact): G[r][c] = <z_r, z_c>.

Two references, both torch itself on the same GPU (torch.manual_seed(s), then torch.normal per
tensor in order, frozen ones drawn and dropped):

* bit for bit, the contract of include/fks.h: row r of the matrix equals
  codec.project_multi(specs, column seeds, [torch's draw of row seed r, in the spec dtype])[0],
  compared as int64.  This pins the order of the additions, the +0 of the elements past a
  tensor's end and of the lanes without a group, and the frozen tensor.
* independent of the projection code: math.fsum of the exact f64 products z_r z_c (24 x 24
  significand bits at most), with test_gpu_project.py's bound for any f64 summation order of n
  terms, |got - ref| <= n 2^-52 sum|z_r z_c|.

Tensor list: test_gpu_project.py's (4096 | 1000 | 3 frozen | 700,001 | 7 | 65,536 |
4 256 cap + 1025), in each of the three dtypes."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import _dev
from test_gpu_project import DT, DTYPES, FROZEN, U, _i64, _offsets, _sizes, _specs

pytestmark = pytest.mark.gpu

_g = torch.Generator().manual_seed(20261021)
SEEDS = [0, 2**32 - 1, 2**40 + 3] + torch.randint(0, 2**32, (34,), generator=_g).tolist()  # 37: 32 + 5, 9 x 4 + 1
ROWS = [0, 1, 3, 4, 31, 32, 36]


def _draw_list(dts, sizes, seed, dev):
    """torch's draw of one seed: one tensor per spec, in the spec's dtype (tensor i draws dts[i])"""
    torch.manual_seed(seed)
    return [torch.normal(mean=0, std=1, size=(n,), device=dev, dtype=DT[d]) for d, n in zip(dts, sizes)]


def _gram(specs, seeds, cols=None, **kw):
    from fate_llm.algo.fedkseed import codec
    return codec.gram(specs, seeds, cols, stream_mode="torch_rocm", **kw)


def _rows_by_projection(specs, dts, sizes, rows, cols, dev, **kw):
    """what the contract says rows `rows` (seeds) of the matrix against the column seeds are"""
    from fate_llm.algo.fedkseed import codec
    out = []
    for s in rows:
        z = _draw_list(dts, sizes, s, dev)
        out.append(_i64(codec.project_multi(specs, cols, [z], stream_mode="torch_rocm", **kw)[0]))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _dense(dtype):
    """Computed once per dtype and shared: for the first three seeds, fsum(z_r z_c) and
    sum|z_r z_c| over the live elements, all pairs."""
    dev = _dev()
    sizes = _sizes()
    off = _offsets(sizes)
    live = np.ones(off[-1], bool)
    live[off[FROZEN]:off[FROZEN + 1]] = False
    z = [torch.cat([t.float() for t in _draw_list([dtype] * len(sizes), sizes, s, dev)]).cpu().numpy()
         .astype(np.float64)[live] for s in SEEDS[:3]]
    ref, sabs = np.zeros((3, 3)), np.zeros((3, 3))
    for r in range(3):
        for c in range(r, 3):
            p = z[r] * z[c]  # exact products
            ref[r, c] = ref[c, r] = math.fsum(p.tolist())
            sabs[r, c] = sabs[c, r] = float(np.abs(p).sum())
    return {"ref": ref, "sabs": sabs, "n": int(live.sum())}


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_equal_the_projection_of_torchs_draws(dtype):
    dev = _dev()
    sizes = _sizes()
    specs = _specs(dtype)
    G = _gram(specs, SEEDS)
    assert G.dtype == torch.float64 and G.shape == (37, 37) and G.device.type == "cuda"
    got = _i64(G)
    want = _rows_by_projection(specs, [dtype] * len(sizes), sizes, [SEEDS[r] for r in ROWS], SEEDS, dev)
    bad = [(r, int((got[r] != w).sum())) for r, w in zip(ROWS, want) if not np.array_equal(got[r], w)]
    assert not bad, f"(row, columns that differ): {bad}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_within_f64_sum_bound(dtype):
    c = _dense(dtype)
    got = _gram(_specs(dtype), SEEDS[:3]).cpu().numpy()
    err, bound = np.abs(got - c["ref"]), c["n"] * U * c["sabs"]
    print(f"{dtype}: max |got - fsum| / bound = {float((err / bound).max()):.3e}; diagonal / n = "
          f"{(np.diag(got) / c['n']).tolist()}")
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_symmetry_and_batching_independence(dtype):
    specs = _specs(dtype)
    G = _i64(_gram(specs, SEEDS))
    assert np.array_equal(G, G.T)
    perm = np.random.default_rng(3).permutation(len(SEEDS))
    P = _i64(_gram(specs, [SEEDS[i] for i in perm]))
    assert np.array_equal(P, G[np.ix_(perm, perm)])
    # a rectangular call on (rows A, columns B) is the [A, B] block of the symmetric call on A + B
    A, B = list(range(0, 9)), list(range(9, 37))  # 9 rows: a last row tile of one; 28 columns
    R = _gram(specs, [SEEDS[i] for i in A], [SEEDS[i] for i in B])
    assert R.shape == (9, 28) and np.array_equal(_i64(R), G[np.ix_(A, B)])
    R = _gram(specs, [SEEDS[i] for i in B], [SEEDS[i] for i in A + B])  # 28 x 37: two column batches
    assert np.array_equal(_i64(R), G[np.ix_(B, A + B)])
    # duplicated seeds give duplicated rows and columns
    idx = [0, 5, 0, 7, 5, 36, 0]
    D = _i64(_gram(specs, [SEEDS[i] for i in idx]))
    assert np.array_equal(D, G[np.ix_(idx, idx)])
    one = _gram(specs, [SEEDS[4]])
    assert one.shape == (1, 1) and _i64(one)[0, 0] == G[4, 4] and float(one) > 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards(dtype, nshards):
    dev = _dev()
    c = _dense(dtype)
    sizes = _sizes()
    specs = _specs(dtype)
    seeds = SEEDS[:3]
    parts = []
    for r in range(nshards):
        S = _gram(specs, seeds, shard=r, nshards=nshards)
        want = _rows_by_projection(specs, [dtype] * len(sizes), sizes, seeds[1:], seeds, dev, shard=r, nshards=nshards)
        assert np.array_equal(_i64(S)[1:], want), r
        assert np.array_equal(_i64(S), _i64(S).T)
        parts.append(S.cpu().numpy())
    total = np.array([[math.fsum(p[i, j] for p in parts) for j in range(3)] for i in range(3)])
    err, bound = np.abs(total - c["ref"]), c["n"] * U * c["sabs"]
    assert (err <= bound).all(), (err, bound)


def test_a_shard_with_no_element_gives_zeros():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = [codec.ParamSpec(torch.empty(7, dtype=torch.bfloat16, device=dev))]  # one row of items: one shard owns it
    ranges = [codec.shard_range(specs, r, 3, stream_mode="torch_rocm") for r in range(3)]
    empty = [r for r, (lo, hi) in enumerate(ranges) if lo == hi]
    assert len(empty) == 2
    whole = _i64(_gram(specs, SEEDS[:5]))
    for r in range(3):
        S = _i64(_gram(specs, SEEDS[:5], shard=r, nshards=3))
        assert np.array_equal(S, np.zeros((5, 5), np.int64) if r in empty else whole)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_cases(dtype):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    frozen = [codec.ParamSpec(torch.empty(n, dtype=DT[dtype], device=dev), frozen=True) for n in (4096, 7)]
    assert np.array_equal(_i64(_gram(frozen, SEEDS[:5])), np.zeros((5, 5), np.int64))
    assert np.array_equal(_i64(_gram(frozen, SEEDS[:5], SEEDS[:2])), np.zeros((5, 2), np.int64))
    specs = _specs(dtype)
    none = _gram(specs, [])
    assert none.shape == (0, 0) and none.dtype == torch.float64
    assert _gram(specs, SEEDS[:3], []).shape == (3, 0) and _gram(specs, [], SEEDS[:3]).shape == (0, 3)
    # empty tensors in the list draw nothing: the same bits
    sp = _specs(dtype)
    sp.insert(4, codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)))
    sp.append(codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)))
    assert np.array_equal(_i64(_gram(sp, SEEDS[:5])), _i64(_gram(specs, SEEDS[:5])))


def _check_list_against_projection(dts, sizes, frozen=()):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = [codec.ParamSpec(torch.empty(n, dtype=DT[d], device=dev), frozen=(i in frozen))
             for i, (d, n) in enumerate(zip(dts, sizes))]
    G = _i64(_gram(specs, SEEDS))
    assert np.array_equal(G, G.T)
    rows = [0, 4, 33, 36]
    want = _rows_by_projection(specs, dts, sizes, [SEEDS[r] for r in rows], SEEDS, dev)
    assert np.array_equal(G[rows], want)
    assert (np.diag(G.view(np.float64)) > 0.0).all()


def test_several_dtypes_in_one_wave():
    """Tensors of 300 to 2,000 elements have 512 to 2,048 items, one to four waves of 64 groups of
    eight; the items past a tensor's end belong to no element, so a wave spans neighbours of
    different dtypes, runs one pass per dtype, and every lane's rows are drawn in its own dtype."""
    dts = [DTYPES[(i * 7) % 3] for i in range(12)]
    sizes = [300, 2000, 777, 1025, 301, 1999, 512, 1300, 300, 640, 1111, 2000]
    _check_list_against_projection(dts, sizes, frozen=(5,))


def test_table_longer_than_the_lds_copy():
    """600 entries: the kernel reads the tensor table from device memory (more than 512)."""
    n = 600
    _check_list_against_projection([DTYPES[i % 3] for i in range(n)], [(7 * i) % 41 + 1 for i in range(n)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_ordering_and_state(dtype):
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs(dtype)
    seeds = SEEDS[:9]
    torch.manual_seed(123)
    torch.rand(3)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    a = _i64(_gram(specs, seeds))
    b = _i64(_gram(specs, seeds))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        d = _gram(specs, seeds)
    side.synchronize()
    assert np.array_equal(a, b) and np.array_equal(a, _i64(d))
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    # the C call overwrites every element of its output (pre-filled with NaN): the symmetric form, whose
    # lower triangle only the mirror writes, and the rectangular one
    L = N.load()
    batch = codec._Batch(specs, "torch_rocm", stage=False)
    s = np.array(seeds, dtype=np.uint64)
    nbytes = ctypes.c_size_t(0)
    N.check(L.fks_gram_workspace_size(ctypes.addressof(batch.arr), batch.n, 9, 9, ctypes.byref(nbytes)))
    assert 0 < nbytes.value <= 16 << 20  # nothing of the model's size
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.full((9, 9), float("nan"), dtype=torch.float64, device=dev)
    N.check(L.fks_gram(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, 9, None, 0, 0, 1, out.data_ptr(),
                       ws.data_ptr(), nbytes.value, stream))
    assert np.array_equal(_i64(out), a)
    out = torch.full((9, 5), float("nan"), dtype=torch.float64, device=dev)
    N.check(L.fks_gram(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, 9, s[2:7].ctypes.data, 5, 0, 1,
                       out.data_ptr(), ws.data_ptr(), nbytes.value, stream))
    assert np.array_equal(_i64(out), a[:, 2:7])
    # ... also when the shard holds nothing (a list of empty and frozen tensors): zeroed, no workspace
    out.fill_(float("nan"))
    sp0 = [codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)),
           codec.ParamSpec(torch.empty(5, dtype=DT[dtype], device=dev), frozen=True)]
    b0 = codec._Batch(sp0, "torch_rocm", stage=False)
    N.check(L.fks_gram(ctypes.addressof(b0.arr), b0.n, s.ctypes.data, 9, s[2:7].ctypes.data, 5, 0, 1, out.data_ptr(),
                       None, 0, stream))
    assert np.array_equal(_i64(out), np.zeros((9, 5), np.int64))


@functools.lru_cache(maxsize=None)
def _model():
    """Two groups, N = 3,000 live elements (2,000 f32 + 1,000 bf16) and a frozen parameter between
    them; K = 40 seeds; Z[N, K] as torch draws it, in float64."""
    dev = _dev()
    g = torch.Generator().manual_seed(77)
    shapes, dts, rg = [(50, 40), (300,), (1000,)], ["float32", "float32", "bfloat16"], [True, False, True]
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(DT[d]).to(dev), requires_grad=r)
              for s, d, r in zip(shapes, dts, rg)]
    groups = [{"params": params[:2], "lr": 1e-3, "weight_decay": 0.0}, {"params": params[2:], "lr": 1e-3, "weight_decay": 0.0}]
    seeds = torch.randint(0, 2**32, (40,), generator=g).tolist()
    assert len(set(seeds)) == 40
    cols = []
    for s in seeds:
        torch.manual_seed(s)
        z = [torch.normal(mean=0, std=1, size=p.shape, device=dev, dtype=p.dtype) for p in params]
        cols.append(torch.cat([t.float().reshape(-1) for t, r in zip(z, rg) if r]).cpu().numpy().astype(np.float64))
    return params, groups, seeds, np.stack(cols, axis=1)


def _as_vectors(params, flat):
    """a float64[N] vector over the live elements as one f32 tensor per parameter (None: frozen)"""
    out, at = [], 0
    for p in params:
        if not p.requires_grad:
            out.append(None)
            continue
        out.append(torch.from_numpy(flat[at:at + p.numel()].astype(np.float32)).reshape(p.shape).to(p.device))
        at += p.numel()
    return out


def test_seed_gram_and_exact_fit():
    from fate_llm.algo.fedkseed import zo_utils
    params, groups, seeds, Z = _model()
    n, K = Z.shape
    assert (n, K) == (3000, 40)
    G = zo_utils.seed_gram(groups, seeds, stream_mode="torch_rocm")
    assert G.shape == (K, K) and G.dtype == torch.float64 and G.device.type == "cuda"
    ref = Z.T @ Z
    assert np.abs(G.cpu().numpy() - ref).max() <= n * U * (np.abs(Z).T @ np.abs(Z)).max() * 2
    assert np.linalg.cond(ref) < 2.0
    R = zo_utils.seed_gram(groups, seeds[:3], seeds[5:9], stream_mode="torch_rocm")
    assert torch.equal(R.view(torch.int64), G[:3, 5:9].contiguous().view(torch.int64))
    rng = np.random.default_rng(5)
    # (a) generic deltas against numpy's least squares on torch's draws
    deltas = rng.standard_normal((2, n)).astype(np.float32).astype(np.float64)
    want = np.stack([np.linalg.lstsq(Z, d, rcond=None)[0] for d in deltas])
    got = zo_utils.fit_seed_scalars_exact(groups, seeds, [_as_vectors(params, d) for d in deltas],
                                          stream_mode="torch_rocm")
    assert got.shape == (2, K) and got.dtype == torch.float64 and got.device.type == "cuda"
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"(a) exact fit against lstsq: {err:.3e}, max|c| {np.abs(want).max():.3e}")
    assert err <= 1e-9 * np.abs(want).max()
    # (b) a delta inside the span, delta = Z c formed in float64 and stored as f32, is recovered
    c = rng.standard_normal(K)
    vec = _as_vectors(params, Z @ c)
    c_hat = zo_utils.fit_seed_scalars_exact(groups, seeds, [vec], stream_mode="torch_rocm").cpu().numpy()[0]
    rel = np.linalg.norm(c_hat - c) / np.linalg.norm(c)
    print(f"(b) |c_hat - c| / |c| = {rel:.3e}")
    assert rel <= 1e-6
    # (c) the approximate fit, Z^T delta / N, misses by more than 1e-2 on the same input
    c_fit = zo_utils.fit_seed_scalars_in_place(groups, seeds, [vec], stream_mode="torch_rocm").cpu().numpy()[0]
    rel_fit = np.linalg.norm(c_fit - c) / np.linalg.norm(c)
    print(f"(c) fit_seed_scalars_in_place: |c_fit - c| / |c| = {rel_fit:.3e}")
    assert rel_fit > 1e-2
    staged = zo_utils.fit_seed_scalars(groups, seeds, vec, stream_mode="torch_rocm").cpu().numpy()
    assert np.linalg.norm(staged - c) / np.linalg.norm(c) > 1e-2
    # more seeds than live elements: the Gram matrix is singular and the fit says so
    small = torch.nn.Parameter(torch.zeros(8, dtype=torch.float32, device=params[0].device))
    with pytest.raises(ValueError, match="positive definite"):
        zo_utils.fit_seed_scalars_exact([{"params": [small]}], seeds[:12], [[torch.ones(8, device=small.device)]],
                                        stream_mode="torch_rocm")


def test_refuses_the_torch_cpu_stream():
    from fate_llm.algo.fedkseed import zo_utils
    params, groups, seeds, _ = _model()
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        _ = __import__("fate_llm.algo.fedkseed.codec", fromlist=["gram"]).gram(
            _specs("bfloat16"), SEEDS[:3], stream_mode="torch_cpu")
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        zo_utils.seed_gram(groups, seeds[:3], stream_mode="torch_cpu")
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        zo_utils.fit_seed_scalars_exact(groups, seeds[:3], [_as_vectors(params, np.zeros(3000))],
                                        stream_mode="torch_cpu")
