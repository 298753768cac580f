"""Tiled seed-basis Gram matrix on the torch_cpu stream (fks_gram_mt_tiled, codec.gram_mt_tiled,
the zo_utils *_tiled_on_stream forms): G[r][c] = <z_r, z_c> over the CPU generator's MT19937 draws.

References: (a) torch's own CPU draws (under FKS_LIBM what codec.normal_ writes, which the suite
pins), exact products summed with math.fsum; (b) codec.gram_mt.  Bounds, the header's with
sum|z_r z_c| <= sqrt(G_rr G_cc): n 2^-52 sqrt(G_rr G_cc) against (a), twice that against (b).
Everything else the contract states is bit for bit, compared as int64.  Lists: mt_layouts' G per
dtype (G:float16 has no fast segment: no regular launch) and mixed, G in f32 under FKS_LIBM, R (a
workgroup walks several blocks), tensors below 16 elements only.  K = 33: three blocks, one of one."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import mt_layouts as ML
from test_gpu_expand_mt import SEEDS57
from test_gpu_parity import _dev
from test_gpu_project_mt import U, _i64

pytestmark = pytest.mark.gpu

S33 = SEEDS57[:33]
TINY = ML.MtList("tiny", (5, 3, 7, 1, 15, 2, 4, 9), tuple(ML.CYC[i % 3] for i in range(8)), (2,))
CASES = [("G:bfloat16", False), ("G:float32", False), ("G:float32", True), ("G:float16", False), ("G:mixed", False),
         ("tiny", False), ("R", False)]
_list = lambda name: TINY if name == "tiny" else ML.get(name)  # noqa: E731


@functools.lru_cache(maxsize=None)
def _specs(name):
    from fate_llm.algo.fedkseed import codec
    lst, dev = _list(name), _dev()
    return tuple(codec.ParamSpec(torch.empty(n, dtype=ML.DT[d], device=dev), frozen=(i in lst.frozen))
                 for i, (n, d) in enumerate(zip(lst.sizes, lst.dts)))


def _call(fn, name, libm, *a, **kw):
    from fate_llm.algo.fedkseed import codec
    codec.set_cpu_fp32_flavour("libm" if libm else None)
    try:
        return fn(_specs(name), *a, **kw)
    finally:
        codec.set_cpu_fp32_flavour(None)


@functools.lru_cache(maxsize=None)
def _tiled(name, libm, k):
    from fate_llm.algo.fedkseed import codec
    return _call(codec.gram_mt_tiled, name, libm, S33[:k])


@functools.lru_cache(maxsize=None)
def _gram_mt(name, libm):
    from fate_llm.algo.fedkseed import codec
    return _call(codec.gram_mt, name, libm, S33).cpu().numpy()


def _draws(name, libm, seeds):
    from fate_llm.algo.fedkseed import codec
    lst = _list(name)
    if libm:
        out = []
        for s in seeds:
            ts = [torch.empty(n, dtype=ML.DT[d], device=_dev()) for n, d in zip(lst.sizes, lst.dts)]
            _call(lambda _, t, seed: codec.normal_(t, seed, stream_mode="torch_cpu", leave_generator=False), name, True,
                  ts, s)
            out.append(torch.cat([t.float().cpu() for t in ts]))
    else:
        out = [ML.draw(lst, s) for s in seeds] if name == "tiny" else ML.zs(name, list(seeds))
    live = ML.live_mask(lst)
    return [z.numpy().astype(np.float64)[live] for z in out]


@functools.lru_cache(maxsize=None)
def _fsum(name, libm):
    z = _draws(name, libm, S33[:3] if name == "R" else S33)  # all pairs of 33 seeds on the small lists, of 3 on R
    ref = np.zeros((len(z), len(z)))
    for r in range(len(z)):
        for c in range(r, len(z)):
            ref[r, c] = ref[c, r] = math.fsum((z[r] * z[c]).tolist())  # exact products
    return ref, len(z[0])


def _share(got, ref, n, terms=1):
    d = np.sqrt(np.diag(ref))
    return float((np.abs(got - ref) / (terms * n * U * np.outer(d, d)[:got.shape[0], :got.shape[1]])).max())


@pytest.mark.parametrize("k", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("name,libm", CASES)
def test_against_fsum_and_gram_mt(name, libm, k):
    G = _tiled(name, libm, k)
    assert G.shape == (k, k) and G.dtype == torch.float64 and G.device.type == "cuda"
    got = G.cpu().numpy()
    ref, n = _fsum(name, libm)
    m = min(k, len(ref))
    a, b = _share(got[:m, :m], ref[:m, :m], n), _share(got, _gram_mt(name, libm)[:k, :k], n, terms=2)
    print(f"{name} libm={libm} K={k}: share of the bound: {a:.3e} against fsum, {b:.3e} against gram_mt")
    assert a <= 1.0 and b <= 1.0 and (np.diag(got) > 0.0).all()
    assert np.array_equal(_i64(G), _i64(G).T)
    assert np.array_equal(_i64(G), _i64(_tiled(name, libm, 33))[:k, :k])  # the corner of the K = 33 call


@pytest.mark.parametrize("name,libm", CASES)
def test_bit_for_bit_properties(name, libm):
    from fate_llm.algo.fedkseed import codec
    G = _i64(_tiled(name, libm, 33))
    assert np.array_equal(_i64(_call(codec.gram_mt_tiled, name, libm, S33)), G)  # two calls
    assert np.array_equal(_i64(_call(codec.gram_mt_tiled, name, libm, S33, S33)), G)  # the rectangular form
    perm = np.random.default_rng(3).permutation(33)
    assert np.array_equal(_i64(_call(codec.gram_mt_tiled, name, libm, [S33[i] for i in perm])), G[np.ix_(perm, perm)])
    idx = [0, 5, 0, 20, 5, 32, 0] + list(range(16, 30))  # duplicated seeds, 21: two blocks
    assert np.array_equal(_i64(_call(codec.gram_mt_tiled, name, libm, [S33[i] for i in idx])), G[np.ix_(idx, idx)])
    R = _call(codec.gram_mt_tiled, name, libm, S33[:17], S33[20:25])  # 17 x 5: a block of one row
    assert R.shape == (17, 5) and np.array_equal(_i64(R), G[:17, 20:25])


@pytest.mark.parametrize("name", ["G:mixed", "R"])
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards_add_up(name, nshards):
    from fate_llm.algo.fedkseed import codec
    parts = [codec.gram_mt_tiled(_specs(name), S33[:17], shard=r, nshards=nshards) for r in range(nshards)]
    assert all(np.array_equal(_i64(p), _i64(p).T) for p in parts)
    total = sum(p.cpu().numpy() for p in parts)
    ref, n = _fsum(name, False)
    m = len(ref) if name == "R" else 17
    assert _share(total[:m, :m], ref[:m, :m], n, terms=2) <= 1.0  # the shards' own sums, then their addition
    assert _share(total, _gram_mt(name, False)[:17, :17], n, terms=3) <= 1.0


def test_a_shard_with_no_element_gives_zeros():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.empty(48, dtype=torch.bfloat16, device=_dev()))]  # one MT block: one shard owns it
    whole = _i64(codec.gram_mt_tiled(specs, S33[:17]))
    got = [_i64(codec.gram_mt_tiled(specs, S33[:17], shard=r, nshards=3)) for r in range(3)]
    assert whole.any() and sorted(g.any() for g in got) == [False, False, True]
    assert all(np.array_equal(g, whole) for g in got if g.any())


def test_c_call_overwrites_and_leaves_generators_and_caches_alone():
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev, name = _dev(), "G:bfloat16"
    lst, specs = _list(name), _specs(name)
    g = torch.Generator().manual_seed(9)
    init = [(torch.randn(n, generator=g) * 0.02).to(torch.bfloat16).to(dev) for n in lst.sizes]

    def reconstruct():  # through the attached window caches
        ps = [t.clone() for t in init]
        sp = [codec.ParamSpec(t, lr=1e-2, weight_decay=0.0, frozen=(i in lst.frozen)) for i, t in enumerate(ps)]
        codec.directional_step(sp, S33[:24], [1e-3 * (i + 1) for i in range(24)], stream_mode="torch_cpu",
                               cache_windows=True, leave_generator=False)
        return [_i64(t.view(torch.int16).to(torch.int64)) for t in ps]

    before = reconstruct()
    torch.manual_seed(123)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    batch = codec._Batch(list(specs), "torch_cpu", stage=False)
    s = np.array(S33[:17], dtype=np.uint64)
    nbytes = ctypes.c_size_t(0)
    N.check(N.load().fks_gram_mt_tiled_workspace_size(ctypes.addressof(batch.arr), batch.n, 17, 17, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    out = torch.full((17, 17), float("nan"), dtype=torch.float64, device=dev)
    N.check(N.load().fks_gram_mt_tiled(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, 17, None, 0, 0, 1, out.data_ptr(),
                                ws.data_ptr(), nbytes.value, torch.cuda.current_stream(dev).cuda_stream))
    assert np.array_equal(_i64(out), _i64(_tiled(name, False, 17)))  # the mirror writes the lower triangle too
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    after = reconstruct()  # the same bits with the windows the first reconstruct left
    codec.jwin_release(dev)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_zo_utils_route_by_stream_and_the_fit_recovers_a_delta_in_the_span():
    from test_gpu_gram import _as_vectors
    from test_gpu_gram_mt import _model
    from fate_llm.algo.fedkseed import codec, zo_utils
    params, groups, seeds, Z = _model()  # N = 3,000 live elements, K = 40, Z as torch draws it on the CPU
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    for mode, want in (("torch_cpu", codec.gram_mt_tiled(specs, seeds)),
                       ("torch_rocm", codec.gram_tiled(specs, seeds, stream_mode="torch_rocm"))):
        G = zo_utils.seed_gram_tiled_on_stream(groups, seeds, stream_mode=mode)
        assert torch.equal(G.view(torch.int64), want.view(torch.int64)), mode
    c = np.random.default_rng(5).standard_normal(len(seeds))
    vec = [_as_vectors(params, Z @ c)]  # delta = Z c formed in float64 and stored as f32
    c_hat = zo_utils.fit_seed_scalars_exact_tiled_on_stream(groups, seeds, vec, stream_mode="torch_cpu").cpu().numpy()[0]
    assert np.linalg.norm(c_hat - c) / np.linalg.norm(c) <= 1e-6
    a = zo_utils.fit_seed_scalars_exact_tiled_on_stream(groups, seeds, vec, stream_mode="torch_rocm")
    b = zo_utils.fit_seed_scalars_exact_tiled(groups, seeds, vec, stream_mode="torch_rocm")
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
