"""Bit-sliced seed-basis projection on the torch_cpu stream (fks_project_mt_bs, codec.project_mt_bs,
zo_utils.seed_projections_bitsliced): out[m][s] = <vec_m, z_s> over the CPU generator's MT19937 draws.

References: (a) torch's own CPU draws (under FKS_LIBM what codec.normal_ writes, which the suite
pins), exact f64 products summed with math.fsum; (b) codec.project_mt_multi.  Bounds, derived: any
order of n exact products errs by at most one f64 rounding per term, n 2^-52 sum|v z| against (a),
and two such sums differ by at most twice that against (b).  Everything else the contract states is
bit for bit, compared as int64.  Lists: mt_layouts' G in bf16 and mixed, G in f32 under FKS_LIBM and
in f16 (no bf16 fast segment: no bit-sliced launch), R (a workgroup walks several blocks and its
tasks wrap the 624-row state; its fsum reference covers three of the seeds), one bf16 tensor of 16
elements (one task) and one of 128 W 3 + 48 (every wave of a half has tasks, the last is partial).
K: below the slice kernel's old threshold, one full half, a half plus one seed, a full pass, a pass
plus one seed (a split pass behind a two-half one) and 97."""
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

W = 4  # waves per half (csrc/fks_project_mt_bs.h FKS_PMBS_WAVES)
S97 = SEEDS57 + torch.randint(0, 2**32, (40,), generator=torch.Generator().manual_seed(97)).tolist()
KS = [1, 19, 20, 32, 33, 64, 65, 97]
OWN = {"one16": ML.MtList("one16", (16,), ("bfloat16",), ()),
       "waves": ML.MtList("waves", (128 * W * 3 + 48,), ("bfloat16",), ())}
CASES = [("G:bfloat16", False), ("G:mixed", False), ("G:float32", True), ("G:float16", False), ("R", False),
         ("one16", False), ("waves", False)]
VDT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
_list = lambda name: OWN.get(name) or ML.get(name)  # noqa: E731
_ref_idx = lambda name: (0, 33, 96) if name == "R" else tuple(range(97))  # noqa: E731  (seeds with an fsum reference)


@functools.lru_cache(maxsize=None)
def _specs(name):
    from fate_llm.algo.fedkseed import codec
    lst, dev = _list(name), _dev()
    return tuple(codec.ParamSpec(torch.empty(n, dtype=ML.DT[d], device=dev), frozen=(i in lst.frozen))
                 for i, (n, d) in enumerate(zip(lst.sizes, lst.dts)))


@functools.lru_cache(maxsize=None)
def _values(name, vdt):
    """N(0, 1) over the concatenation, rounded to the vector's dtype; a CPU tensor of that dtype"""
    return torch.randn(sum(_list(name).sizes), generator=torch.Generator().manual_seed(11)).to(VDT[vdt])


def _vector(name, values, shift=0):
    """one device tensor per spec (None: frozen), each `shift` elements into a buffer of its own"""
    lst, off, out = _list(name), ML.offsets(_list(name).sizes), []
    for i, n in enumerate(lst.sizes):
        buf = torch.empty(n + shift, dtype=values.dtype, device=_dev())
        buf[shift:] = values[off[i]:off[i + 1]].to(_dev())
        out.append(None if i in lst.frozen else buf[shift:])
    return out


def _call(fn, name, libm, *a, **kw):
    from fate_llm.algo.fedkseed import codec
    codec.set_cpu_fp32_flavour("libm" if libm else None)
    try:
        return fn(_specs(name), *a, **kw)
    finally:
        codec.set_cpu_fp32_flavour(None)


@functools.lru_cache(maxsize=None)
def _bs(name, libm, k, vdt):
    from fate_llm.algo.fedkseed import codec
    return _call(codec.project_mt_bs, name, libm, S97[:k], [_vector(name, _values(name, vdt))])


@functools.lru_cache(maxsize=None)
def _multi(name, libm, vdt):
    from fate_llm.algo.fedkseed import codec
    return _call(codec.project_mt_multi, name, libm, S97, [_vector(name, _values(name, vdt))]).cpu().numpy()[0]


@functools.lru_cache(maxsize=None)
def _draws(name, libm):
    """float64 z over the live elements for the seeds _ref_idx names, drawn once per list"""
    from fate_llm.algo.fedkseed import codec
    lst, seeds = _list(name), [S97[i] for i in _ref_idx(name)]
    if libm:
        out = []
        for s in seeds:
            ts = [torch.empty(n, dtype=ML.DT[d], device=_dev()) for n, d in zip(lst.sizes, lst.dts)]
            _call(lambda _, t, seed: codec.normal_(t, seed, stream_mode="torch_cpu", leave_generator=False), name, True,
                  ts, s)
            out.append(torch.cat([t.float().cpu() for t in ts]))
    else:
        out = ML.zs(name, seeds) if name.startswith("G:") else [ML.draw(lst, s) for s in seeds]
    live = ML.live_mask(lst)
    return [z.numpy().astype(np.float64)[live] for z in out]


@functools.lru_cache(maxsize=None)
def _fsum(name, libm, vdt):
    """{seed index: (the exact sum, sum|v z|)} and n"""
    v = _values(name, vdt).float().numpy().astype(np.float64)[ML.live_mask(_list(name))]
    ref = {i: (math.fsum((v * z).tolist()), float(np.abs(v * z).sum())) for i, z in zip(_ref_idx(name), _draws(name, libm))}
    return ref, len(v)


@pytest.mark.parametrize("k,vdt", [(k, "float32") for k in KS] + [(97, "bfloat16"), (97, "float16")])
@pytest.mark.parametrize("name,libm", CASES)
def test_against_the_exact_sum_and_project_mt_multi(name, libm, k, vdt):
    out = _bs(name, libm, k, vdt)
    assert out.shape == (1, k) and out.dtype == torch.float64 and out.device.type == "cuda"
    got, (ref, n), multi = out.cpu().numpy()[0], _fsum(name, libm, vdt), _multi(name, libm, vdt)
    have = [i for i in ref if i < k]
    a = max([abs(got[i] - ref[i][0]) / (n * U * ref[i][1]) for i in have], default=0.0)
    b = max([abs(got[i] - multi[i]) / (2 * n * U * ref[i][1]) for i in have], default=0.0)
    print(f"{name} libm={libm} K={k} {vdt}: share of the bound: {a:.3e} against fsum, {b:.3e} against project_mt_multi")
    assert have and a <= 1.0 and b <= 1.0
    assert np.array_equal(_i64(out), _i64(_bs(name, libm, 97, vdt))[:, :k])  # the entries of the K = 97 call


@pytest.mark.parametrize("name,libm", CASES)
def test_bit_for_bit_properties(name, libm):
    from fate_llm.algo.fedkseed import codec
    run = lambda seeds, vecs: _i64(_call(codec.project_mt_bs, name, libm, seeds, vecs))  # noqa: E731
    v32, v16, vbf = (_values(name, d) for d in ("float32", "float16", "bfloat16"))
    full = _i64(_bs(name, libm, 97, "float32"))
    assert np.array_equal(run(S97, [_vector(name, v32)]), full)  # two calls
    perm = np.random.default_rng(3).permutation(97)
    assert np.array_equal(run([S97[i] for i in perm], [_vector(name, v32)]), full[:, perm])
    idx = [0, 40, 0, 96, 40, 5, 0] + list(range(30, 70))  # duplicated seeds, 47: a half and a part of one
    assert np.array_equal(run([S97[i] for i in idx], [_vector(name, v32)]), full[:, idx])
    three = run(S97[:33], [_vector(name, v32), _vector(name, vbf), _vector(name, v16)])  # mixed dtypes, one call
    assert three.shape == (3, 33) and np.array_equal(three[0], full[0, :33])
    assert np.array_equal(three[1], _i64(_bs(name, libm, 97, "bfloat16"))[0, :33])
    assert np.array_equal(three[2], _i64(_bs(name, libm, 97, "float16"))[0, :33])
    assert np.array_equal(run(S97[:33], [_vector(name, vbf.float())]), three[1:2])  # the same values stored as f32
    assert np.array_equal(run(S97[:33], [_vector(name, v16, shift=1)]), three[2:3])  # at an odd element offset
    assert np.array_equal(run(S97[:33], [_vector(name, v32, shift=1)]), full[:, :33])


@pytest.mark.parametrize("name", ["G:mixed", "R"])
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards_add_up(name, nshards):
    from fate_llm.algo.fedkseed import codec
    (ref, n), vec = _fsum(name, False, "float32"), [_vector(name, _values(name, "float32"))]
    idx = [i for i in ref][:33]
    parts = [codec.project_mt_bs(_specs(name), [S97[i] for i in idx], vec, shard=r, nshards=nshards).cpu().numpy()[0]
             for r in range(nshards)]
    share = max(abs(sum(p[j] for p in parts) - ref[i][0]) / ((nshards + 1) * n * U * ref[i][1]) for j, i in enumerate(idx))
    print(f"{name} {nshards} shards: share of the bound {share:.3e}")
    assert share <= 1.0


def test_a_shard_with_no_element_gives_zeros():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.empty(48, dtype=torch.bfloat16, device=_dev()))]  # one MT block: one shard owns it
    vec = [[torch.randn(48, generator=torch.Generator().manual_seed(2)).to(_dev())]]
    whole = _i64(codec.project_mt_bs(specs, S97[:33], vec))
    got = [_i64(codec.project_mt_bs(specs, S97[:33], vec, shard=r, nshards=3)) for r in range(3)]
    assert whole.any() and sorted(g.any() for g in got) == [False, False, True]
    assert all(np.array_equal(g, whole) for g in got if g.any())


def test_c_call_overwrites_and_leaves_generators_and_caches_alone():
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev, name, k = _dev(), "G:bfloat16", 33
    lst, specs = _list(name), _specs(name)
    g = torch.Generator().manual_seed(9)
    init = [(torch.randn(n, generator=g) * 0.02).to(torch.bfloat16).to(dev) for n in lst.sizes]

    def reconstruct():  # through the attached window caches
        ps = [t.clone() for t in init]
        sp = [codec.ParamSpec(t, lr=1e-2, weight_decay=0.0, frozen=(i in lst.frozen)) for i, t in enumerate(ps)]
        codec.directional_step(sp, S97[:24], [1e-3 * (i + 1) for i in range(24)], stream_mode="torch_cpu",
                               cache_windows=True, leave_generator=False)
        return [_i64(t.view(torch.int16).to(torch.int64)) for t in ps]

    before = reconstruct()
    torch.manual_seed(123)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    batch = codec._Batch(list(specs), "torch_cpu", stage=False)
    vec = _vector(name, _values(name, "float32"))
    varr = (N.FksVec * len(specs))()
    for i, v in enumerate(vec):
        if v is not None and v.numel():
            varr[i].data, varr[i].dtype = v.data_ptr(), N.F32
    s = np.array(S97[:k], dtype=np.uint64)
    nbytes = ctypes.c_size_t(0)
    N.check(N.load().fks_project_mt_bs_workspace_size(ctypes.addressof(batch.arr), batch.n, k, 1, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    out = torch.full((1, k), float("nan"), dtype=torch.float64, device=dev)
    N.check(N.load().fks_project_mt_bs(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, k, ctypes.addressof(varr), 1, 0,
                                       1, out.data_ptr(), ws.data_ptr(), nbytes.value,
                                       torch.cuda.current_stream(dev).cuda_stream))
    assert np.array_equal(_i64(out), _i64(_bs(name, False, 97, "float32"))[:, :k])
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    after = reconstruct()  # the same bits with the windows the first reconstruct left
    codec.jwin_release(dev)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_zo_utils_routes_by_stream():
    from test_gpu_gram import _as_vectors
    from test_gpu_gram_mt import _model
    from fate_llm.algo.fedkseed import codec, zo_utils
    params, groups, seeds, Z = _model()  # N = 3,000 live elements (f32 and bf16), K = 40
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    vecs = [_as_vectors(params, Z @ np.random.default_rng(5).standard_normal(len(seeds)))]
    for mode, want in (("torch_cpu", codec.project_mt_bs(specs, seeds, vecs)),
                       ("torch_rocm", codec.project_multi(specs, seeds, vecs, stream_mode="torch_rocm"))):
        got = zo_utils.seed_projections_bitsliced(groups, seeds, vecs, stream_mode=mode)
        assert got.shape == (1, len(seeds)) and torch.equal(got.view(torch.int64), want.view(torch.int64)), mode
    grads = [[None if v is None else v.to(p.dtype) for p, v in zip(params, vecs[0])]]
    for p, v in zip(params, grads[0]):
        p.grad = v  # the default: the .grad tensors
    got = zo_utils.seed_projections_bitsliced(groups, seeds, stream_mode="torch_cpu")
    assert torch.equal(got.view(torch.int64), codec.project_mt_bs(specs, seeds, grads).view(torch.int64))
