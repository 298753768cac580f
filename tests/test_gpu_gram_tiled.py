"""Tiled seed-basis Gram matrix on the f64 matrix unit (fks_gram_tiled, codec.gram_tiled,
zo_utils.seed_gram_tiled / fit_seed_scalars_exact_tiled): G[r][c] = <z_r, z_c> in passes of 64 x 64
seeds.

The call's products are exact and its additions f64, in an order of its own, so it is held to two
references that are not the code under test, each with the bound any f64 summation order of n
terms meets, |sum - true| <= n 2^-52 sum|terms| (U = 2^-52, test_gpu_project.py's):

* codec.gram, the 4 x 32 kernel this change leaves alone: both are within n U sum|z_r z_c| of the
  true sum, so they differ by at most 2 n U sum|z_r z_c| <= 2 n U sqrt(G_rr G_cc) (Cauchy-Schwarz),
  with the diagonal taken from codec.gram.  Derived, not measured; a wrong lane or row map, a
  missed tail zero or a frozen tensor counted misses it by orders of magnitude.
* math.fsum of torch's own draws for three seeds (test_gpu_gram.py's _dense): n U sum|z_r z_c|.

What the contract promises bit for bit -- reproducibility, exact symmetry, independence of the
other seeds, their order and number, the place in a tile and the passes -- is compared as int64.

Tensor list: test_gpu_project.py's (4096 | 1000 | 3 frozen | 700,001 | 7 | 65,536 |
4 256 cap + 1025), in each of the three dtypes; T + 16 + 5 seeds for a tile of T seeds (85 at 64),
so that a call crosses a tile boundary both ways and ends in a partial 16-block."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import _dev
from test_gpu_project import DT, DTYPES, FROZEN, U, _i64, _offsets, _sizes, _specs
from test_gpu_gram import SEEDS as GRAM_SEEDS
from test_gpu_gram import _as_vectors, _dense, _model

pytestmark = pytest.mark.gpu

_g = torch.Generator().manual_seed(20261022)
_MORE = torch.randint(0, 2**32, (400,), generator=_g).tolist()


@functools.lru_cache(maxsize=None)
def _tile():
    from fate_llm.algo.fedkseed import codec
    return max(codec._gram_tiled_tile())


@functools.lru_cache(maxsize=None)
def _seeds():
    """T + 16 + 5 distinct seeds; the first three are test_gpu_gram.py's (the dense reference's)"""
    k = _tile() + 16 + 5
    out = list(GRAM_SEEDS[:3])
    for s in _MORE:
        if len(out) == k:
            break
        if s not in out:
            out.append(s)
    assert len(out) == k
    return out


def _tiled(specs, seeds, cols=None, **kw):
    from fate_llm.algo.fedkseed import codec
    return codec.gram_tiled(specs, seeds, cols, stream_mode="torch_rocm", **kw)


def _gram(specs, seeds, cols=None, **kw):
    from fate_llm.algo.fedkseed import codec
    return codec.gram(specs, seeds, cols, stream_mode="torch_rocm", **kw)


def _live(sizes, frozen=(FROZEN,)):
    return int(sum(n for i, n in enumerate(sizes) if i not in frozen))


@functools.lru_cache(maxsize=None)
def _big(dtype):
    """Computed once per dtype and shared, never changed: the tiled matrix of all the seeds (bits)."""
    return _i64(_tiled(_specs(dtype), _seeds()))


def _rows_of_interest(k):
    t = _tile()
    return sorted({0, 15, 16, t - 1, t, k - 1})


def _check_against_gram(specs, seeds, n, G, rows):
    """rows `rows` of the tiled matrix G (float64, all columns) against codec.gram's, a rectangular call"""
    ref = _gram(specs, [seeds[r] for r in rows], seeds).cpu().numpy()
    diag = np.array([float(_gram(specs, [s])) for s in seeds]) if len(seeds) <= 4 else \
        np.diag(_gram(specs, seeds).cpu().numpy())
    assert (diag > 0).all()
    bound = 2 * n * U * np.sqrt(np.outer(diag[rows], diag))
    err = np.abs(G[rows] - ref)
    print(f"max |tiled - gram| / bound = {float((err / bound).max()):.3e} over rows {rows}")
    assert (err <= bound).all(), (float(err.max()), float(bound.min()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_untiled_kernel(dtype):
    specs, seeds = _specs(dtype), _seeds()
    G = _tiled(specs, seeds)
    k = len(seeds)
    assert G.dtype == torch.float64 and G.shape == (k, k) and G.device.type == "cuda"
    assert np.array_equal(_i64(G), _big(dtype))
    _check_against_gram(specs, seeds, _live(_sizes()), G.cpu().numpy(), _rows_of_interest(k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 15, 16, 17])
def test_small_seed_counts(dtype, k):
    specs, seeds = _specs(dtype), _seeds()[:k]
    G = _tiled(specs, seeds)
    assert G.shape == (k, k)
    _check_against_gram(specs, seeds, _live(_sizes()), G.cpu().numpy(), sorted({0, k - 1}))
    # ... and the same bits as inside the large call
    assert np.array_equal(_i64(G), _big(dtype)[:k, :k])


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_within_f64_sum_bound(dtype):
    c = _dense(dtype)
    got = _big(dtype)[:3, :3].copy().view(np.float64)
    err, bound = np.abs(got - c["ref"]), c["n"] * U * c["sabs"]
    print(f"{dtype}: max |got - fsum| / bound = {float((err / bound).max()):.3e}; diagonal / n = "
          f"{(np.diag(got) / c['n']).tolist()}")
    assert (err <= bound).all(), (err, bound)
    rect = _tiled(_specs(dtype), _seeds()[:2], _seeds()[:3]).cpu().numpy()
    assert (np.abs(rect - c["ref"][:2]) <= bound[:2]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_for_bit_properties(dtype):
    dev = _dev()
    specs, seeds = _specs(dtype), _seeds()
    k = len(seeds)
    G = _big(dtype)
    # the same call twice, and on a side stream
    again = _i64(_tiled(specs, seeds))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        d = _tiled(specs, seeds)
    side.synchronize()
    assert np.array_equal(G, again) and np.array_equal(G, _i64(d))
    assert np.array_equal(G, G.T)
    # a permutation of the seeds permutes the matrix: nothing depends on the place in a tile
    perm = np.random.default_rng(3).permutation(k)
    P = _i64(_tiled(specs, [seeds[i] for i in perm]))
    assert np.array_equal(P, G[np.ix_(perm, perm)])
    # a rectangular call on (rows A, columns B) is the [A, B] block of the symmetric call on A + B
    A, B = list(range(0, 9)), list(range(9, k))
    R = _tiled(specs, [seeds[i] for i in A], [seeds[i] for i in B])
    assert R.shape == (9, k - 9) and np.array_equal(_i64(R), G[np.ix_(A, B)])
    R = _tiled(specs, [seeds[i] for i in B], [seeds[i] for i in A + B])
    assert np.array_equal(_i64(R), G[np.ix_(B, A + B)])
    # duplicated seeds give duplicated rows and columns
    idx = [0, 5, 0, 7, 5, k - 1, 0, 16, 64 % k]
    D = _i64(_tiled(specs, [seeds[i] for i in idx]))
    assert np.array_equal(D, G[np.ix_(idx, idx)])
    # K = 1 is the diagonal element of the large call
    one = _tiled(specs, [seeds[k - 2]])
    assert one.shape == (1, 1) and _i64(one)[0, 0] == G[k - 2, k - 2] and float(one) > 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards(dtype, nshards):
    c = _dense(dtype)
    specs = _specs(dtype)
    seeds = _seeds()[:3]
    parts = []
    for r in range(nshards):
        S = _tiled(specs, seeds, shard=r, nshards=nshards)
        assert np.array_equal(_i64(S), _i64(S).T), r
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
    seeds = _seeds()[:5]
    whole = _i64(_tiled(specs, seeds))
    assert (whole.view(np.float64).diagonal() > 0).all()
    for r in range(3):
        S = _i64(_tiled(specs, seeds, shard=r, nshards=3))
        assert np.array_equal(S, np.zeros((5, 5), np.int64) if r in empty else whole)


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_lists(dtype):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    seeds = _seeds()
    frozen = [codec.ParamSpec(torch.empty(n, dtype=DT[dtype], device=dev), frozen=True) for n in (4096, 7)]
    assert np.array_equal(_i64(_tiled(frozen, seeds[:5])), np.zeros((5, 5), np.int64))
    assert np.array_equal(_i64(_tiled(frozen, seeds[:5], seeds[:2])), np.zeros((5, 2), np.int64))
    specs = _specs(dtype)
    none = _tiled(specs, [])
    assert none.shape == (0, 0) and none.dtype == torch.float64
    assert _tiled(specs, seeds[:3], []).shape == (3, 0) and _tiled(specs, [], seeds[:3]).shape == (0, 3)
    # empty tensors in the list draw nothing: the same bits
    sp = _specs(dtype)
    sp.insert(4, codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)))
    sp.append(codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)))
    assert np.array_equal(_i64(_tiled(sp, seeds[:18])), _big(dtype)[:18, :18])


def _check_list_against_gram(dts, sizes, frozen=()):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = [codec.ParamSpec(torch.empty(n, dtype=DT[d], device=dev), frozen=(i in frozen))
             for i, (d, n) in enumerate(zip(dts, sizes))]
    seeds = _seeds()
    G = _tiled(specs, seeds)
    assert np.array_equal(_i64(G), _i64(G).T)
    _check_against_gram(specs, seeds, _live(sizes, frozen), G.cpu().numpy(), _rows_of_interest(len(seeds)))


def test_several_dtypes_side_by_side():
    """test_gpu_gram.py's 12-tensor list (300 to 2,000 elements each, the three dtypes mixed, one
    frozen): every tensor is a few 256-item chunks, most of them past the tensor's end in part,
    and neighbouring chunks of a wave draw different dtypes."""
    dts = [DTYPES[(i * 7) % 3] for i in range(12)]
    sizes = [300, 2000, 777, 1025, 301, 1999, 512, 1300, 300, 640, 1111, 2000]
    _check_list_against_gram(dts, sizes, frozen=(5,))


def test_table_longer_than_the_lds_copy():
    """600 entries: the kernel reads the tensor table from device memory (more than 512)."""
    n = 600
    _check_list_against_gram([DTYPES[i % 3] for i in range(n)], [(7 * i) % 41 + 1 for i in range(n)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_c_call_overwrites_and_leaves_the_generators(dtype):
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs(dtype)
    seeds = _seeds()[:20]
    torch.manual_seed(123)
    torch.rand(3)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    a = _i64(_tiled(specs, seeds))
    assert np.array_equal(a, _big(dtype)[:20, :20])
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    # the C call overwrites every element of its output (pre-filled with NaN): the symmetric form, whose
    # lower triangle only the mirror writes, and the rectangular one
    L = N.load()
    batch = codec._Batch(specs, "torch_rocm", stage=False)
    s = np.array(seeds, dtype=np.uint64)
    nbytes = ctypes.c_size_t(0)
    N.check(L.fks_gram_tiled_workspace_size(ctypes.addressof(batch.arr), batch.n, 20, 20, ctypes.byref(nbytes)))
    assert 0 < nbytes.value <= 64 << 20  # nothing of the model's size
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.full((20, 20), float("nan"), dtype=torch.float64, device=dev)
    N.check(L.fks_gram_tiled(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, 20, None, 0, 0, 1, out.data_ptr(),
                             ws.data_ptr(), nbytes.value, stream))
    assert np.array_equal(_i64(out), a)
    out = torch.full((20, 5), float("nan"), dtype=torch.float64, device=dev)
    N.check(L.fks_gram_tiled(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, 20, s[2:7].ctypes.data, 5, 0, 1,
                             out.data_ptr(), ws.data_ptr(), nbytes.value, stream))
    assert np.array_equal(_i64(out), a[:, 2:7])
    # ... also when the shard holds nothing (a list of empty and frozen tensors): zeroed, no workspace
    out.fill_(float("nan"))
    sp0 = [codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)),
           codec.ParamSpec(torch.empty(5, dtype=DT[dtype], device=dev), frozen=True)]
    b0 = codec._Batch(sp0, "torch_rocm", stage=False)
    N.check(L.fks_gram_tiled(ctypes.addressof(b0.arr), b0.n, s.ctypes.data, 20, s[2:7].ctypes.data, 5, 0, 1,
                             out.data_ptr(), None, 0, stream))
    assert np.array_equal(_i64(out), np.zeros((20, 5), np.int64))
    out = torch.full((20, 20), float("nan"), dtype=torch.float64, device=dev)
    N.check(L.fks_gram_tiled(ctypes.addressof(b0.arr), b0.n, s.ctypes.data, 20, None, 0, 0, 1, out.data_ptr(),
                             None, 0, stream))
    assert np.array_equal(_i64(out), np.zeros((20, 20), np.int64))
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)


def test_seed_gram_tiled_and_exact_fit():
    from fate_llm.algo.fedkseed import zo_utils
    params, groups, seeds, Z = _model()
    n, K = Z.shape
    assert (n, K) == (3000, 40)
    G = zo_utils.seed_gram_tiled(groups, seeds, stream_mode="torch_rocm")
    assert G.shape == (K, K) and G.dtype == torch.float64 and G.device.type == "cuda"
    ref = Z.T @ Z
    assert np.abs(G.cpu().numpy() - ref).max() <= 2 * n * U * (np.abs(Z).T @ np.abs(Z)).max()
    assert torch.equal(G.view(torch.int64), G.t().contiguous().view(torch.int64))
    assert np.linalg.cond(ref) < 2.0
    R = zo_utils.seed_gram_tiled(groups, seeds[:3], seeds[5:9], stream_mode="torch_rocm")
    assert torch.equal(R.view(torch.int64), G[:3, 5:9].contiguous().view(torch.int64))
    rng = np.random.default_rng(5)
    # (a) generic deltas against numpy's least squares on torch's draws
    deltas = rng.standard_normal((2, n)).astype(np.float32).astype(np.float64)
    want = np.stack([np.linalg.lstsq(Z, d, rcond=None)[0] for d in deltas])
    got = zo_utils.fit_seed_scalars_exact_tiled(groups, seeds, [_as_vectors(params, d) for d in deltas],
                                                stream_mode="torch_rocm")
    assert got.shape == (2, K) and got.dtype == torch.float64 and got.device.type == "cuda"
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"(a) exact tiled fit against lstsq: {err:.3e}, max|c| {np.abs(want).max():.3e}")
    assert err <= 1e-9 * np.abs(want).max()
    # (b) a delta inside the span, delta = Z c formed in float64 and stored as f32, is recovered
    c = rng.standard_normal(K)
    vec = _as_vectors(params, Z @ c)
    c_hat = zo_utils.fit_seed_scalars_exact_tiled(groups, seeds, [vec], stream_mode="torch_rocm").cpu().numpy()[0]
    rel = np.linalg.norm(c_hat - c) / np.linalg.norm(c)
    print(f"(b) |c_hat - c| / |c| = {rel:.3e}")
    assert rel <= 1e-6
    # more seeds than live elements: the Gram matrix is singular and the fit says so
    small = torch.nn.Parameter(torch.zeros(8, dtype=torch.float32, device=params[0].device))
    with pytest.raises(ValueError, match="positive definite"):
        zo_utils.fit_seed_scalars_exact_tiled([{"params": [small]}], seeds[:12],
                                              [[torch.ones(8, device=small.device)]], stream_mode="torch_rocm")


def test_refuses_the_torch_cpu_stream():
    from fate_llm.algo.fedkseed import codec, zo_utils
    params, groups, seeds, _ = _model()
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        codec.gram_tiled(_specs("bfloat16"), _seeds()[:3], stream_mode="torch_cpu")
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        zo_utils.seed_gram_tiled(groups, seeds[:3], stream_mode="torch_cpu")
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        zo_utils.fit_seed_scalars_exact_tiled(groups, seeds[:3], [_as_vectors(params, np.zeros(3000))],
                                              stream_mode="torch_cpu")
