"""Bit-sliced seed-basis Gram matrix on the torch_cpu stream (fks_gram_mt_bs, codec.gram_mt_bs, the
zo_utils *_bitsliced Gram forms): G[r][c] = <z_r, z_c> over the CPU generator's MT19937 draws.

References: (a) torch's own CPU draws over the live elements (a frozen tensor contributes nothing),
exact products summed with math.fsum; (b) codec.gram_mt.  Bounds, the header's, derived: any order
of n exact products errs by at most one f64 rounding per term and sum|z_r z_c| <= sqrt(G_rr G_cc),
so n 2^-52 sqrt(G_rr G_cc) against (a) and twice that against (b).  Everything else the contract
states is bit for bit, compared as int64.  Lists: mt_layouts' G in bf16 and mixed (the bit-sliced
launch runs), R (a workgroup walks several MT blocks: the twist wraps the 624 rows and a chunk ends
inside a task; its fsum reference covers three seeds), G in f16 (no bf16 fast segment: everything
goes through the existing launches).  K: one seed, a partial block, a full block, a block plus one
seed, a full diagonal pass, a diagonal pass plus a one-seed block, and 48 (a second diagonal pass of
one block, two pair passes)."""
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

S48 = SEEDS57[:48]
NAMES = ["G:bfloat16", "G:mixed", "R", "G:float16"]


@functools.lru_cache(maxsize=None)
def _specs(name):
    from fate_llm.algo.fedkseed import codec
    lst, dev = ML.get(name), _dev()
    return tuple(codec.ParamSpec(torch.empty(n, dtype=ML.DT[d], device=dev), frozen=(i in lst.frozen))
                 for i, (n, d) in enumerate(zip(lst.sizes, lst.dts)))


@functools.lru_cache(maxsize=None)
def _bs(name, k):
    from fate_llm.algo.fedkseed import codec
    return codec.gram_mt_bs(_specs(name), S48[:k])


@functools.lru_cache(maxsize=None)
def _gram_mt(name):
    from fate_llm.algo.fedkseed import codec
    return codec.gram_mt(_specs(name), S48).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fsum(name):
    live = ML.live_mask(ML.get(name))
    z = [x.numpy().astype(np.float64)[live] for x in ML.zs(name, list(S48[:3] if name == "R" else S48))]
    ref = np.zeros((len(z), len(z)))
    for r in range(len(z)):
        for c in range(r, len(z)):
            ref[r, c] = ref[c, r] = math.fsum((z[r] * z[c]).tolist())  # exact products
    return ref, len(z[0])


def _share(got, ref, n, rows=slice(None), cols=slice(None), terms=1):
    d = np.sqrt(np.diag(ref))
    return float((np.abs(got - ref[rows, cols]) / (terms * n * U * np.outer(d[rows], d[cols]))).max())


@pytest.mark.parametrize("k", [1, 15, 16, 17, 32, 33, 48])
@pytest.mark.parametrize("name", NAMES)
def test_against_fsum_and_gram_mt(name, k):
    G = _bs(name, k)
    assert G.shape == (k, k) and G.dtype == torch.float64 and G.device.type == "cuda"
    got = G.cpu().numpy()
    ref, n = _fsum(name)
    m = slice(0, min(k, len(ref)))
    a, b = _share(got[m, m], ref, n, m, m), _share(got, _gram_mt(name), n, slice(0, k), slice(0, k), terms=2)
    print(f"{name} K={k}: share of the bound: {a:.3e} against fsum, {b:.3e} against gram_mt")
    assert a <= 1.0 and b <= 1.0 and (np.diag(got) > 0.0).all()
    assert np.array_equal(_i64(G), _i64(G).T)
    assert np.array_equal(_i64(G), _i64(_bs(name, 48))[:k, :k])  # the corner of the K = 48 call


@pytest.mark.parametrize("name", NAMES)
def test_bit_for_bit_properties(name):
    from fate_llm.algo.fedkseed import codec
    G = _i64(_bs(name, 48))
    # a cell reached once through the diagonal form and once through the pair form, in other planes
    assert np.array_equal(_i64(codec.gram_mt_bs(_specs(name), S48[16:32], S48[0:16])), G[16:32, 0:16])
    R = codec.gram_mt_bs(_specs(name), S48[:5], S48[20:40])  # 5 x 20: a partial row block, two column blocks
    assert R.shape == (5, 20) and np.array_equal(_i64(R), G[:5, 20:40])
    assert np.array_equal(_i64(codec.gram_mt_bs(_specs(name), S48[::-1])), G[::-1, ::-1])  # the list reversed


@pytest.mark.parametrize("name", ["G:mixed", "R"])
def test_shards_add_up(name):
    from fate_llm.algo.fedkseed import codec
    parts = [codec.gram_mt_bs(_specs(name), S48[:33], shard=r, nshards=3) for r in range(3)]
    assert all(np.array_equal(_i64(p), _i64(p).T) for p in parts)
    total = sum(p.cpu().numpy() for p in parts)
    # the shards' own sums (n terms between them) and the whole's, then the two additions: (2 n + 2) <= 3 n terms
    assert _share(total, _bs(name, 33).cpu().numpy(), _fsum(name)[1], terms=3) <= 1.0


def test_c_call_with_a_caller_sized_workspace_overwrites():
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev, name = _dev(), "G:mixed"
    batch = codec._Batch(list(_specs(name)), "torch_cpu", stage=False)
    s = np.array(S48[:33], dtype=np.uint64)
    nbytes = ctypes.c_size_t(0)
    N.check(N.load().fks_gram_mt_bs_workspace_size(ctypes.addressof(batch.arr), batch.n, 33, 33, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    out = torch.full((33, 33), float("nan"), dtype=torch.float64, device=dev)
    N.check(N.load().fks_gram_mt_bs(ctypes.addressof(batch.arr), batch.n, s.ctypes.data, 33, None, 0, 0, 1, out.data_ptr(),
                                    ws.data_ptr(), nbytes.value, torch.cuda.current_stream(dev).cuda_stream))
    assert np.array_equal(_i64(out), _i64(_bs(name, 33)))  # the mirror writes the lower triangle too


def test_zo_utils_forms_and_the_fit_recovers_a_delta_in_the_span():
    from test_gpu_gram import _as_vectors
    from test_gpu_gram_mt import _model
    from fate_llm.algo.fedkseed import codec, zo_utils
    params, groups, seeds, Z = _model()  # N = 3,000 live elements, K = 40, Z as torch draws it on the CPU
    specs = [codec.ParamSpec(p.data, frozen=not p.requires_grad) for p in params]
    G = zo_utils.seed_gram_bitsliced(groups, seeds, stream_mode="torch_cpu")
    assert torch.equal(G.view(torch.int64), codec.gram_mt_bs(specs, seeds).view(torch.int64))
    c = np.random.default_rng(5).standard_normal(len(seeds))
    vec = [_as_vectors(params, Z @ c)]  # delta = Z c formed in float64 and stored as f32
    c_hat = zo_utils.fit_seed_scalars_exact_bitsliced(groups, seeds, vec, stream_mode="torch_cpu").cpu().numpy()[0]
    assert np.linalg.norm(c_hat - c) / np.linalg.norm(c) <= 1e-6
    with pytest.raises(NotImplementedError, match="torch_cpu stream only"):
        zo_utils.seed_gram_bitsliced(groups, seeds, stream_mode="torch_rocm")
