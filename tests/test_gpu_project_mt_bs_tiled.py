"""Bit-sliced seed-basis projection of many vectors per draw on the torch_cpu stream
(fks_project_mt_bs_tiled, codec.project_mt_bs_tiled, zo_utils.seed_projections_bitsliced_tiled):
out[m][s] = <vec_m, z_s> over the CPU generator's MT19937 draws, 32 seeds x 16 vectors per pass.

References: test_gpu_project_mt_bs's -- (a) torch's own CPU draws, exact f64 products summed with
math.fsum; (b) codec.project_mt_multi.  Bounds, derived: any order of n exact products errs by at
most one f64 rounding per term, n 2^-52 sum|v z| against (a), and two such sums differ by at most
twice that against (b).  Everything else the contract states is bit for bit, compared as int64.
Lists: that file's G in bf16, mixed and f16 (no bit-sliced launch at all), R, one bf16 tensor of 16
elements (one task, one wave), and one of 128 * 8 * 3 + 48 (every wave has tasks, the last is partial).
(K, nvec): every K of {1, 16, 17, 32, 33, 65} -- one block, a block plus one seed, a full state, a
second pass -- and every nvec of {1, 2, 16, 17} -- a full tile, a second tile of one column."""
import functools

import numpy as np
import pytest
import torch

import mt_layouts as ML
import test_gpu_project_mt_bs as B
from test_gpu_parity import _dev
from test_gpu_project_mt import U, _i64
from test_gpu_project_mt_bs import S97

pytestmark = pytest.mark.gpu

B.OWN.setdefault("waves8", ML.MtList("waves8", (128 * 8 * 3 + 48,), ("bfloat16",), ()))
LISTS = ["G:bfloat16", "G:mixed", "G:float16", "R", "one16", "waves8"]
VDTS = ["float32", "bfloat16", "float16"]  # vector m is stored as VDTS[m % 3]
K_NVEC = [(1, 17), (16, 2), (17, 16), (32, 1), (33, 17), (65, 2)]


def _tiled(name, seeds, vecs, **kw):
    from fate_llm.algo.fedkseed import codec
    return B._call(codec.project_mt_bs_tiled, name, False, seeds, vecs, **kw)


@functools.lru_cache(maxsize=None)
def _three(name):
    return tuple(B._vector(name, B._values(name, d)) for d in VDTS)


def _cycle(name, nvec):
    """nvec vectors over the three dtypes' values, mixed in one call"""
    return [_three(name)[m % 3] for m in range(nvec)]


def _distinct(name, nvec):
    """nvec vectors of their own values, dtypes mixed"""
    n = sum(B._list(name).sizes)
    return [B._vector(name, torch.randn(n, generator=torch.Generator().manual_seed(100 + m)).to(B.VDT[VDTS[m % 3]]))
            for m in range(nvec)]


@pytest.mark.parametrize("k,nvec", K_NVEC)
@pytest.mark.parametrize("name", LISTS)
def test_against_the_exact_sum_and_project_mt_multi(name, k, nvec):
    out = _tiled(name, S97[:k], _cycle(name, nvec))
    assert out.shape == (nvec, k) and out.dtype == torch.float64 and out.device.type == "cuda"
    got, a, b = out.cpu().numpy(), 0.0, 0.0
    for m in range(nvec):
        (ref, n), multi = B._fsum(name, False, VDTS[m % 3]), B._multi(name, False, VDTS[m % 3])
        have = [i for i in ref if i < k]
        assert have
        a = max([a] + [abs(got[m, i] - ref[i][0]) / (n * U * ref[i][1]) for i in have])
        b = max([b] + [abs(got[m, i] - multi[i]) / (2 * n * U * ref[i][1]) for i in have])
    print(f"{name} K={k} nvec={nvec}: share of the bound: {a:.3e} against fsum, {b:.3e} against project_mt_multi")
    assert a <= 1.0 and b <= 1.0
    assert np.array_equal(_i64(out)[3:], _i64(out)[:-3])  # the same values in another column, another tile


@pytest.mark.parametrize("name", LISTS)
def test_bit_for_bit_properties(name):
    vecs, seeds = _distinct(name, 17), S97[:33]
    full = _i64(_tiled(name, seeds, vecs))
    assert np.array_equal(_i64(_tiled(name, seeds, vecs)), full)  # two calls
    for m in range(17):  # the one-vector calls
        assert np.array_equal(_i64(_tiled(name, seeds, [vecs[m]])), full[m:m + 1]), m
    for s in (0, 15, 16, 32):  # the one-seed calls, and the one-seed, one-vector calls
        assert np.array_equal(_i64(_tiled(name, [seeds[s]], vecs)), full[:, s:s + 1]), s
        assert np.array_equal(_i64(_tiled(name, [seeds[s]], [vecs[s % 17]])), full[s % 17:s % 17 + 1, s:s + 1]), s
    sp = [int(i) for i in np.random.default_rng(3).permutation(33)] + [0, 32, 7, 0]  # permuted and duplicated seeds
    vp = [int(i) for i in np.random.default_rng(4).permutation(17)]
    assert np.array_equal(_i64(_tiled(name, [seeds[i] for i in sp], [vecs[m] for m in vp])), full[vp][:, sp])
    vbf, v16 = B._values(name, "bfloat16"), B._values(name, "float16")
    same = _i64(_tiled(name, seeds, [B._vector(name, vbf), B._vector(name, vbf.float()),  # the same values stored as f32
                                     B._vector(name, vbf, shift=1), B._vector(name, vbf.float(), shift=1),  # at an odd offset
                                     B._vector(name, v16), B._vector(name, v16, shift=1)]))
    assert all(np.array_equal(same[0], same[m]) for m in (1, 2, 3)) and np.array_equal(same[4], same[5])


@pytest.mark.parametrize("name", ["G:mixed", "R"])
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards_add_up(name, nshards):
    (ref, n), vecs = B._fsum(name, False, "float32"), _cycle(name, 2)[:1]
    idx = [i for i in ref][:33]
    parts = [_tiled(name, [S97[i] for i in idx], vecs, shard=r, nshards=nshards).cpu().numpy()[0] for r in range(nshards)]
    share = max(abs(sum(p[j] for p in parts) - ref[i][0]) / ((nshards + 1) * n * U * ref[i][1]) for j, i in enumerate(idx))
    print(f"{name} {nshards} shards: share of the bound {share:.3e}")
    assert share <= 1.0


def test_a_shard_with_no_element_gives_zeros():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.empty(48, dtype=torch.bfloat16, device=_dev()))]  # one MT block: one shard owns it
    vec = [[torch.randn(48, generator=torch.Generator().manual_seed(2)).to(_dev())]] * 2
    whole = _i64(codec.project_mt_bs_tiled(specs, S97[:33], vec))
    got = [_i64(codec.project_mt_bs_tiled(specs, S97[:33], vec, shard=r, nshards=3)) for r in range(3)]
    assert whole.any() and sorted(g.any() for g in got) == [False, False, True]
    assert all(np.array_equal(g, whole) for g in got if g.any())


def test_zo_utils_routes_by_stream():
    from test_gpu_gram import _as_vectors
    from test_gpu_gram_mt import _model
    from fate_llm.algo.fedkseed import codec, zo_utils
    params, groups, seeds, Z = _model()  # N = 3,000 live elements (f32 and bf16), K = 40
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    vecs = [_as_vectors(params, Z @ np.random.default_rng(5 + m).standard_normal(len(seeds))) for m in range(2)]
    for mode, want in (("torch_cpu", codec.project_mt_bs_tiled(specs, seeds, vecs)),
                       ("torch_rocm", codec.project_multi(specs, seeds, vecs, stream_mode="torch_rocm"))):
        got = zo_utils.seed_projections_bitsliced_tiled(groups, seeds, vecs, stream_mode=mode)
        assert got.shape == (2, len(seeds)) and torch.equal(got.view(torch.int64), want.view(torch.int64)), mode
    grads = [[None if v is None else v.to(p.dtype) for p, v in zip(params, vecs[0])]]
    for p, v in zip(params, grads[0]):
        p.grad = v  # the default: the .grad tensors
    got = zo_utils.seed_projections_bitsliced_tiled(groups, seeds, stream_mode="torch_cpu")
    assert torch.equal(got.view(torch.int64), codec.project_mt_bs_tiled(specs, seeds, grads).view(torch.int64))
