"""Seed-basis Gram matrix on the torch_cpu stream (fks_gram_mt, codec.gram_mt, and
zo_utils.seed_gram_on_stream / fit_seed_scalars_exact_on_stream routed there): G[r][c] = <z_r, z_c>,
z_s the CPU generator's MT19937 draw.

Two references, both torch's CPU generator (torch.manual_seed(s), then torch.normal per tensor in
order on the CPU, frozen ones drawn and dropped), as in tests/test_gpu_project_mt.py:

* bit for bit, the contract of include/fks.h: row r of the matrix equals
  codec.project_mt_multi(specs, column seeds, [that draw of row seed r, moved to the device in the
  spec dtypes])[0], compared as int64.  This pins the order of the additions, the +0 of the lanes
  off every segment and of the elements past a run's limit, the ragged tail, the serial draws with
  the value the frozen tensor cached, and the frozen tensor.
* independent of the projection code: math.fsum of the exact f64 products z_r z_c (24 x 24
  significand bits at most) with that file's bound for any f64 summation order of n terms,
  |got - ref| <= n 2^-52 sum|z_r z_c| (derived there, not tuned).

Tensor lists: test_gpu_project_mt.py's 1.1M-element list in each of the three dtypes, and
mt_layouts' G:mixed and R.  The seed counts follow the library's tile (NR rows by NC columns)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import mt_layouts as ML
from test_gpu_expand_mt import SEEDS57
from test_gpu_parity import _dev
from test_gpu_project_mt import DT, DTYPES, FROZEN, SEEDS, SIZES, U, _i64, _offsets, _specs

pytestmark = pytest.mark.gpu

_g = torch.Generator().manual_seed(20261022)
SEEDS_G = SEEDS + torch.randint(0, 2**32, (64,), generator=_g).tolist()  # the 20 of that file, then 64 more


def _tile():
    from fate_llm.algo.fedkseed import codec
    return codec.GRAM_MT_PASS_ROWS, codec.GRAM_MT_PASS_COLS


def _seeds():
    """2 NC + NR + 1 seeds: a last row tile of one, a partial column tile, several diagonal tiles"""
    NR, NC = _tile()
    k = 2 * NC + NR + 1
    assert k <= len(SEEDS_G) and len(set(SEEDS_G[:k])) == k
    return SEEDS_G[:k]


@functools.lru_cache(maxsize=None)
def _cpu_draw(dtype, seed):
    """torch's CPU draw of one seed over test_gpu_project_mt.py's list: one tensor per spec, in the
    spec's dtype; drawn once per (dtype, seed), shared, never written to"""
    torch.manual_seed(seed)
    return tuple(torch.normal(mean=0, std=1, size=(n,), dtype=DT[dtype]) for n in SIZES)


def _vector(dtype, seed, dev):
    return [None if i == FROZEN else z.to(dev) for i, z in enumerate(_cpu_draw(dtype, seed))]


def _rows_by_projection(specs, dtype, rows, cols, dev, **kw):
    """what the contract says rows `rows` (seeds) of the matrix against the column seeds are"""
    from fate_llm.algo.fedkseed import codec
    return np.stack([_i64(codec.project_mt_multi(specs, cols, [_vector(dtype, s, dev)], **kw)[0]) for s in rows])


@functools.lru_cache(maxsize=None)
def _dense(dtype):
    """Computed once per dtype and shared: for the first three seeds, fsum(z_r z_c) and
    sum|z_r z_c| over the live elements, all pairs."""
    off = _offsets(SIZES)
    live = np.ones(off[-1], bool)
    live[off[FROZEN]:off[FROZEN + 1]] = False
    z = [torch.cat([t.float() for t in _cpu_draw(dtype, s)]).numpy().astype(np.float64)[live] for s in SEEDS_G[:3]]
    ref, sabs = np.zeros((3, 3)), np.zeros((3, 3))
    for r in range(3):
        for c in range(r, 3):
            p = z[r] * z[c]  # exact products
            ref[r, c] = ref[c, r] = math.fsum(p.tolist())
            sabs[r, c] = sabs[c, r] = float(np.abs(p).sum())
    return {"ref": ref, "sabs": sabs, "n": int(live.sum())}


# ---- 1. rows equal the projection
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_equal_the_projection_of_torchs_cpu_draws(dtype):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    NR, NC = _tile()
    S = _seeds()
    K = len(S)
    specs = _specs(dtype)
    G = codec.gram_mt(specs, S)
    assert G.dtype == torch.float64 and G.shape == (K, K) and G.device.type == "cuda"
    got = _i64(G)
    rows = sorted({0, 1, NR - 1, NR, K - 1})
    want = _rows_by_projection(specs, dtype, [S[r] for r in rows], S, dev)
    bad = [(r, int((got[r] != w).sum())) for r, w in zip(rows, want) if not np.array_equal(got[r], w)]
    assert not bad, f"(row, columns that differ): {bad}"


# ---- 2. dense reference, independent of the projection
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_within_f64_sum_bound(dtype):
    from fate_llm.algo.fedkseed import codec
    c = _dense(dtype)
    got = codec.gram_mt(_specs(dtype), SEEDS_G[:3]).cpu().numpy()
    err, bound = np.abs(got - c["ref"]), c["n"] * U * c["sabs"]
    print(f"{dtype}: max |got - fsum| / bound = {float((err / bound).max()):.3e}; diagonal / n = "
          f"{(np.diag(got) / c['n']).tolist()}")
    assert (err <= bound).all(), (err, bound)


# ---- 3. symmetry and batching
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_symmetry_and_batching_independence(dtype):
    from fate_llm.algo.fedkseed import codec
    NR, NC = _tile()
    S = _seeds()
    K = len(S)
    specs = _specs(dtype)
    G = _i64(codec.gram_mt(specs, S))
    assert np.array_equal(G, G.T)
    perm = np.random.default_rng(3).permutation(K)
    P = _i64(codec.gram_mt(specs, [S[i] for i in perm]))
    assert np.array_equal(P, G[np.ix_(perm, perm)])
    # a rectangular call on (rows A, columns B) is the [A, B] block of the symmetric call on A + B
    A, B = list(range(0, NR + 1)), list(range(NR + 1, K))  # a last row tile of one; 2 NC columns
    R = codec.gram_mt(specs, [S[i] for i in A], [S[i] for i in B])
    assert R.shape == (len(A), len(B)) and np.array_equal(_i64(R), G[np.ix_(A, B)])
    R = codec.gram_mt(specs, [S[i] for i in B], [S[i] for i in A + B])  # more than two column tiles
    assert np.array_equal(_i64(R), G[np.ix_(B, A + B)])
    # duplicated seeds give duplicated rows and columns
    idx = [0, 5, 0, 7, 5, K - 1, 0]
    D = _i64(codec.gram_mt(specs, [S[i] for i in idx]))
    assert np.array_equal(D, G[np.ix_(idx, idx)])
    one = codec.gram_mt(specs, [S[4]])
    assert one.shape == (1, 1) and _i64(one)[0, 0] == G[4, 4] and float(one) > 0.0


# ---- 4. shards
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards(dtype, nshards):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    c = _dense(dtype)
    specs = _specs(dtype)
    seeds = SEEDS_G[:3]
    parts = []
    for r in range(nshards):
        S = codec.gram_mt(specs, seeds, shard=r, nshards=nshards)
        want = _rows_by_projection(specs, dtype, seeds[1:], seeds, dev, shard=r, nshards=nshards)
        assert np.array_equal(_i64(S)[1:], want), r
        assert np.array_equal(_i64(S), _i64(S).T)
        parts.append(S.cpu().numpy())
    total = np.array([[math.fsum(p[i, j] for p in parts) for j in range(3)] for i in range(3)])
    err, bound = np.abs(total - c["ref"]), c["n"] * U * c["sabs"]
    assert (err <= bound).all(), (err, bound)


def test_a_shard_with_no_element_gives_zeros():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = [codec.ParamSpec(torch.empty(48, dtype=torch.bfloat16, device=dev))]  # one MT block: one shard owns it
    ranges = [codec.shard_range(specs, r, 3, stream_mode="torch_cpu") for r in range(3)]
    empty = [r for r, (lo, hi) in enumerate(ranges) if lo == hi]
    assert len(empty) == 2
    whole = _i64(codec.gram_mt(specs, SEEDS_G[:5]))
    assert whole.any()
    for r in range(3):
        S = _i64(codec.gram_mt(specs, SEEDS_G[:5], shard=r, nshards=3))
        assert np.array_equal(S, np.zeros((5, 5), np.int64) if r in empty else whole)


# ---- 5. other layouts
@functools.lru_cache(maxsize=None)
def _layout_specs(name):
    from fate_llm.algo.fedkseed import codec
    lst, dev = ML.get(name), _dev()
    return tuple(codec.ParamSpec(torch.empty(n, dtype=ML.DT[d], device=dev), frozen=(i in lst.frozen))
                 for i, (n, d) in enumerate(zip(lst.sizes, lst.dts)))


@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_layouts_against_the_projection(name):
    """Several dtypes in one launch, gaps, a chunk that starts inside a frozen stretch (G:mixed); a
    workgroup that walks several blocks and a table of 1,200 entries (R)."""
    from fate_llm.algo.fedkseed import codec
    dev, lst = _dev(), ML.get(name)
    NR, NC = _tile()
    K = NR + NC + 1
    S = SEEDS57[:K]
    specs = _layout_specs(name)
    off = ML.offsets(lst.sizes)
    G = _i64(codec.gram_mt(specs, S))
    assert np.array_equal(G, G.T) and (np.diag(G.view(np.float64)) > 0.0).all()
    zs = ML.zs(name, S)
    for r in (1, K - 1):
        vec = [None if i in lst.frozen else zs[r][off[i]:off[i + 1]].to(ML.DT[d]).to(dev)  # exact: drawn in d
               for i, d in enumerate(lst.dts)]
        want = _i64(codec.project_mt_multi(specs, S, [vec])[0])
        assert np.array_equal(G[r], want), (name, r, np.nonzero(G[r] != want)[0].tolist())


# ---- 6. the FKS_LIBM flavour
def test_libm_flavour():
    """fp32 under codec.set_cpu_fp32_flavour("libm"): the row vector is what codec.normal_ writes
    under that flavour (the existing suite pins that draw to the reference's)."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    specs = _specs("float32")
    S = SEEDS_G[:6]
    default = _i64(codec.gram_mt(specs, S))
    tensors = [torch.empty(n, dtype=torch.float32, device=dev) for n in SIZES]
    codec.set_cpu_fp32_flavour("libm")
    try:
        assert codec.cpu_fp32_flavour() == "libm"
        got = _i64(codec.gram_mt(specs, S))
        codec.normal_(tensors, S[2], stream_mode="torch_cpu", leave_generator=False)
        vec = [None if i == FROZEN else t for i, t in enumerate(tensors)]
        want = _i64(codec.project_mt_multi(specs, S, [vec])[0])
    finally:
        codec.set_cpu_fp32_flavour(None)
    assert np.array_equal(got[2], want), np.nonzero(got[2] != want)[0].tolist()
    assert np.array_equal(got, got.T)
    if codec.cpu_fp32_flavour() != "libm":  # the two flavours' z differ: so do their Gram matrices
        assert (got != default).any()


# ---- 7. empty cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_cases(dtype):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    S = SEEDS_G[:5]
    specs = _specs(dtype)
    none = codec.gram_mt(specs, [])
    assert none.shape == (0, 0) and none.dtype == torch.float64
    assert codec.gram_mt(specs, S[:3], []).shape == (3, 0) and codec.gram_mt(specs, [], S[:3]).shape == (0, 3)
    frozen = [codec.ParamSpec(torch.empty(n, dtype=DT[dtype], device=dev), frozen=True) for n in (4096, 7)]
    assert np.array_equal(_i64(codec.gram_mt(frozen, S)), np.zeros((5, 5), np.int64))
    assert np.array_equal(_i64(codec.gram_mt(frozen, S, S[:2])), np.zeros((5, 2), np.int64))
    empty = [codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)) for _ in range(2)]
    assert np.array_equal(_i64(codec.gram_mt(empty, S)), np.zeros((5, 5), np.int64))


# ---- 8. stream order and state
def test_stream_ordering_and_state():
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    NR, NC = _tile()
    dtype = "bfloat16"
    specs = _specs(dtype)
    seeds = SEEDS_G[:NR + 2]
    K = len(seeds)
    # a torch_cpu reconstruct through the window cache, before the calls
    g = torch.Generator().manual_seed(9)
    init = [(torch.randn(n, generator=g) * 0.02).to(DT[dtype]).to(dev) for n in SIZES]
    rec_seeds, rec_vals = SEEDS_G[:24], [1e-3 * (i + 1) for i in range(24)]

    def reconstruct():
        ps = [t.clone() for t in init]
        sp = [codec.ParamSpec(t, lr=1e-2, weight_decay=0.0, frozen=(i == FROZEN)) for i, t in enumerate(ps)]
        codec.directional_step(sp, rec_seeds, rec_vals, stream_mode="torch_cpu", cache_windows=True,
                               leave_generator=False)
        return [_i64(t.view(torch.int16).to(torch.int64)) for t in ps]

    before = reconstruct()
    torch.manual_seed(123)
    torch.rand(3)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    a = _i64(codec.gram_mt(specs, seeds))
    b = _i64(codec.gram_mt(specs, seeds))
    assert np.array_equal(a, b)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    after = reconstruct()  # the same bits with the windows the first reconstruct left: the cache is untouched
    codec.jwin_release(dev)
    fresh = reconstruct()
    codec.jwin_release(dev)
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(before, after, fresh))
    # queued behind a kernel that fills dev_out on a side stream, the result is the call's own: the
    # symmetric form, whose lower triangle only the mirror writes, and the rectangular one
    L = N.load()
    batch = codec._Batch(specs, "torch_cpu", stage=False)
    s = np.array(seeds, dtype=np.uint64)
    nbytes = ctypes.c_size_t(0)
    N.check(L.fks_gram_mt_workspace_size(ctypes.addressof(batch.arr), batch.n, K, K, ctypes.byref(nbytes)))
    assert 0 < nbytes.value <= 64 << 20  # nothing of the model's size
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        out = torch.empty((K, K), dtype=torch.float64, device=dev)
        out.fill_(float("nan"))
        N.check(L.fks_gram_mt(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, K, None, 0, 0, 1, out.data_ptr(),
                              ws.data_ptr(), nbytes.value, side.cuda_stream))
        rect = torch.empty((K, 3), dtype=torch.float64, device=dev)
        rect.fill_(float("nan"))
        N.check(L.fks_gram_mt(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, K, s[1:4].ctypes.data, 3, 0, 1,
                              rect.data_ptr(), ws.data_ptr(), nbytes.value, side.cuda_stream))
    side.synchronize()
    assert np.array_equal(_i64(out), a) and np.array_equal(_i64(rect), a[:, 1:4])


# ---- 9. end to end
@functools.lru_cache(maxsize=None)
def _model():
    """test_gpu_gram.py's model -- two groups, N = 3,000 live elements (2,000 f32 + 1,000 bf16) and a
    frozen parameter between them, K = 40 seeds -- with Z[N, K] as torch draws it on the CPU."""
    from test_gpu_gram import _model as rocm_model
    params, groups, seeds, _ = rocm_model()
    cols = []
    for s in seeds:
        torch.manual_seed(s)
        z = [torch.normal(mean=0, std=1, size=p.shape, dtype=p.dtype) for p in params]
        cols.append(torch.cat([t.float().reshape(-1) for t, p in zip(z, params) if p.requires_grad]).numpy()
                    .astype(np.float64))
    return params, groups, seeds, np.stack(cols, axis=1)


def test_seed_gram_and_exact_fit_on_the_torch_cpu_stream():
    from test_gpu_gram import _as_vectors
    from fate_llm.algo.fedkseed import zo_utils
    params, groups, seeds, Z = _model()
    n, K = Z.shape
    assert (n, K) == (3000, 40)
    G = zo_utils.seed_gram_on_stream(groups, seeds, stream_mode="torch_cpu")
    assert G.shape == (K, K) and G.dtype == torch.float64 and G.device.type == "cuda"
    ref = Z.T @ Z
    assert np.abs(G.cpu().numpy() - ref).max() <= n * U * (np.abs(Z).T @ np.abs(Z)).max() * 2
    assert np.linalg.cond(ref) < 2.0
    R = zo_utils.seed_gram_on_stream(groups, seeds[:3], seeds[5:9], stream_mode="torch_cpu")
    assert torch.equal(R.view(torch.int64), G[:3, 5:9].contiguous().view(torch.int64))
    rng = np.random.default_rng(5)
    # (a) generic deltas against numpy's least squares on torch's draws
    deltas = rng.standard_normal((2, n)).astype(np.float32).astype(np.float64)
    want = np.stack([np.linalg.lstsq(Z, d, rcond=None)[0] for d in deltas])
    got = zo_utils.fit_seed_scalars_exact_on_stream(groups, seeds, [_as_vectors(params, d) for d in deltas],
                                                    stream_mode="torch_cpu")
    assert got.shape == (2, K) and got.dtype == torch.float64 and got.device.type == "cuda"
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"(a) exact fit against lstsq: {err:.3e}, max|c| {np.abs(want).max():.3e}")
    assert err <= 1e-9 * np.abs(want).max()
    # (b) a delta inside the span, delta = Z c formed in float64 and stored as f32, is recovered
    c = rng.standard_normal(K)
    vec = _as_vectors(params, Z @ c)
    c_hat = zo_utils.fit_seed_scalars_exact_on_stream(groups, seeds, [vec], stream_mode="torch_cpu").cpu().numpy()[0]
    rel = np.linalg.norm(c_hat - c) / np.linalg.norm(c)
    print(f"(b) |c_hat - c| / |c| = {rel:.3e}")
    assert rel <= 1e-6
    # (c) the approximate fit, Z^T delta / N, misses by more than 1e-2 on the same input
    c_fit = zo_utils.fit_seed_scalars_in_place(groups, seeds, [vec], stream_mode="torch_cpu").cpu().numpy()[0]
    rel_fit = np.linalg.norm(c_fit - c) / np.linalg.norm(c)
    print(f"(c) fit_seed_scalars_in_place: |c_fit - c| / |c| = {rel_fit:.3e}")
    assert rel_fit > 1e-2
    # more seeds than live elements: the Gram matrix is singular and the fit says so
    small = torch.nn.Parameter(torch.zeros(8, dtype=torch.float32, device=params[0].device))
    with pytest.raises(ValueError, match="positive definite"):
        zo_utils.fit_seed_scalars_exact_on_stream([{"params": [small]}], seeds[:12],
                                                  [[torch.ones(8, device=small.device)]], stream_mode="torch_cpu")


def test_the_torch_rocm_route_returns_the_torch_rocm_bits():
    from test_gpu_gram import _as_vectors
    from fate_llm.algo.fedkseed import zo_utils
    params, groups, seeds, _ = _model()
    G = zo_utils.seed_gram_on_stream(groups, seeds[:9], stream_mode="torch_rocm")
    assert torch.equal(G.view(torch.int64), zo_utils.seed_gram(groups, seeds[:9], stream_mode="torch_rocm").view(torch.int64))
    R = zo_utils.seed_gram_on_stream(groups, seeds[:3], seeds[5:9], stream_mode="torch_rocm")
    assert torch.equal(R.view(torch.int64),
                       zo_utils.seed_gram(groups, seeds[:3], seeds[5:9], stream_mode="torch_rocm").view(torch.int64))
    vec = [_as_vectors(params, np.random.default_rng(6).standard_normal(3000))]
    a = zo_utils.fit_seed_scalars_exact_on_stream(groups, seeds, vec, stream_mode="torch_rocm")
    b = zo_utils.fit_seed_scalars_exact(groups, seeds, vec, stream_mode="torch_rocm")
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
