"""fks_delta_accumulate on the MT19937 stream with three kernels writing one f32 buffer in one
call: list M (tests/delta_ref.py) has bf16 fast segments (the slice kernel from K = 20 on, 64
seeds per pass) and f16, f32, ragged, tiny and pair-misaligned tensors
(fks_irregular_kernel<kModeDelta>, 19 per pass), a frozen tensor and an empty one; none of its
f32 tensors is a fast segment (they are ragged, frozen, tiny or off the 16-word phase), so list
MF puts a 4096-element f32 tensor in front of it (fks_apply_kernel<kModeDelta>, 19 seeds per
pass) and leaves the layout behind it as it is.  K = 2 and 4 take the small-K plan, 5 is the
first K past it, 19 and 20 lie on the two sides of the slice kernel's threshold, 41 and 65 give
the three kernels different numbers of passes.

Reference: O.delta_accumulate bit for bit, and the independent reference of tests/delta_ref.py at
K = 5 and 41.  The delta is a guarded view pre-filled with N(0, 1) values: the guards and the
frozen tensor's range keep their bits.  A base of 8 modulo 16 gives the same bits; a base of 4
modulo 8 is refused before anything is written."""
import functools

import numpy as np
import pytest
import torch

import delta_ref as D
from test_gpu_parity import _dev, from_np, rand_params, to_np

pytestmark = pytest.mark.gpu

KS = [2, 4, 5, 19, 20, 41, 65]


@functools.lru_cache(maxsize=None)
def _inputs(k, name="M"):
    L = D.dlist(name)
    seeds, coefs = D.seeds_coefs(k, seed=200 + k)
    d0 = D.prefill(L.total, seed=9)
    return seeds, coefs, d0, D.oracle_accumulate(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0)


def _params(dev, name):
    """live parameters (the delta calls must leave them alone)"""
    from fate_llm.algo.fedkseed import codec
    L = D.dlist(name)
    arrays = [rand_params([n], d, seed=30 + i)[0] for i, (n, d) in enumerate(zip(L.sizes, L.dtypes))]
    ts = [from_np(a, d, dev) for a, d in zip(arrays, L.dtypes)]
    return arrays, ts, [codec.ParamSpec(t, frozen=f) for t, f in zip(ts, L.frozen)]


@pytest.mark.parametrize("name", ["M", "MF"])
@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("k", KS)
def test_three_kernels_one_buffer(k, shift, name):
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), D.dlist(name)
    fi = L.frozen.index(True)
    assert L.sizes[fi] == 624 * 5 and L.sizes[fi + 2] == 0 and len(L.sizes) == (14 if name == "M" else 15)
    seeds, coefs, d0, want = _inputs(k, name)
    arrays, ts, specs = _params(dev, name)
    buf, view = D.guarded(d0, dev, shift)
    codec.delta_accumulate(specs, seeds, coefs, view)
    torch.cuda.synchronize()
    assert D.guards_intact(buf, view), "a guard element was written"
    got = view.cpu().numpy()
    bad = D.bits32(got) != D.bits32(want)
    assert not bad.any(), f"list {name}, K {k}: {int(bad.sum())} of {bad.size} delta elements differ (first {int(np.argmax(bad))})"
    fz = slice(L.off[fi], L.off[fi + 1])
    assert np.array_equal(D.bits32(got)[fz], D.bits32(d0)[fz]), "the frozen tensor's range was written"
    for i, (t, a) in enumerate(zip(ts, arrays)):
        assert np.array_equal(to_np(t), a), f"parameter {i} was written"
    if k in (5, 41) and shift == 0:
        ref = D.accumulate_ref(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0, device=dev)
        assert np.array_equal(D.bits32(got), D.bits32(ref)), f"K {k}: differs from the independent reference"


@pytest.mark.parametrize("k", [4, 19, 41])
def test_launches_per_kernel(k):
    """The apply launches of one call, from the pass lengths (fks_internal.h: kBsPassSeeds = 64,
    kMaxSeedsPerPass = 19, the slice kernel from kBsMinSeeds = 20 seeds on): list M launches the
    bf16 kernel and the irregular one, list MF the f32 19-seed kernel as well."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    p19, p64 = -(-k // 19), -(-k // 64)
    bf16 = p64 if k >= 20 else p19
    for name, want in (("M", bf16 + p19), ("MF", bf16 + 2 * p19)):
        L = D.dlist(name)
        seeds, coefs, d0, _ = _inputs(k, name)
        specs = L.specs(dev)
        buf, view = D.guarded(d0, dev)
        with codec.profile() as prof:
            codec.delta_accumulate(specs, seeds, coefs, view)
        torch.cuda.synchronize()
        print(f"delta mixed path proof: list {name}, K {k}: {prof.n_apply} apply launches (expected {want})")
        assert prof.n_apply == want


def test_a_base_of_4_modulo_8_is_refused():
    """fks_delta_accumulate moves aligned f32 pairs: a delta buffer that is not 8-byte aligned is
    -FKS_EINVAL, and nothing is written."""
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), D.dlist("M")
    seeds, coefs, d0, _ = _inputs(20)
    buf, view = D.guarded(d0, dev, shift=1)
    assert view.data_ptr() % 8 == 4
    before = D.bits32(buf).copy()
    with pytest.raises(N.FksError, match="misaligned delta buffer") as e:
        codec.delta_accumulate(L.specs(dev), seeds, coefs, view)
    assert e.value.code == -22  # -FKS_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(D.bits32(buf), before)
