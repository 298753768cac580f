"""fks_delta_accumulate on the MT19937 stream where the bf16 slice kernel runs it:
fks_apply_bs_kernel<kModeDelta> (fks_kern_slice.h: 4-byte elements, f32 pairs exchanged between
neighbour lanes, the 64-bit segment walk), which every bf16 delta call of K >= 20 takes and which
the slice kernel's own tests (test_gpu_slice*.py, update chains only) never call.

Reference: O.delta_accumulate bit for bit (tests/test_delta_ref_host.py ties it to the
independent reference of tests/delta_ref.py), and the independent reference itself at K = 33
and 65.  Every delta buffer is a view inside a larger buffer with 16 guard elements of a sentinel
on each side, pre-filled with N(0, 1) values; the guards must keep their bits.

Lists (tests/delta_ref.py dlist): A, the task-path shapes of test_gpu_slice_task_path.py (16- and
48-element tensors, segments that end inside a task, an odd total, the last tensor at an odd
offset); A3 = a 3-element tensor + A: three serial draws take 8 stream words, so every later
tensor stands at phase 8 and the whole list goes to the irregular kernel, its big tensors at
odd offsets; A7 = a 7-element tensor + A: seven serial draws take 16 words, so the phase stays 0
and it is the pair alignment alone (make_layout's ptr % 8) that sends A's fast tensors to the
irregular kernel; PAR = (4096, 7, 2^16, 9, 4096 * 3, 48): the 7 and the 9 take 16 words each, so
a fast tensor, one that is irregular by its odd offset alone, and two fast ones after the parity
has flipped back write side by side; PATH, no irregular part; BLOCKS, many tasks per
wave and a segment that begins inside a task."""
import functools

import numpy as np
import pytest
import torch

import delta_ref as D
from conftest import assert_bitwise
from test_gpu_parity import _dev, from_np, rand_params, to_np

pytestmark = pytest.mark.gpu

K_SWEEP = [20, 32, 33, 64, 65, 97]  # one split pass, the FULL instantiations (32, 64), 64 + n
K_BS_PASS, K_MAX_PASS = 64, 19      # kBsPassSeeds, kMaxSeedsPerPass (fks_internal.h)


@functools.lru_cache(maxsize=None)
def _inputs(name, k):
    L = D.dlist(name)
    seeds, coefs = D.seeds_coefs(k, seed=100 + k)
    d0 = D.prefill(L.total, seed=7)
    return seeds, coefs, d0, D.oracle_accumulate(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0)


def _run(name, k, shift=0):
    """one guarded delta_accumulate; returns the view's values"""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), D.dlist(name)
    seeds, coefs, d0, _ = _inputs(name, k)
    buf, view = D.guarded(d0, dev, shift)
    codec.delta_accumulate(L.specs(dev), seeds, coefs, view)
    torch.cuda.synchronize()
    assert D.guards_intact(buf, view), f"list {name}, K {k}: a guard element was written"
    return view.cpu().numpy()


def _check(name, k, shift=0):
    got = _run(name, k, shift)
    want = _inputs(name, k)[3]
    bad = D.bits32(got) != D.bits32(want)
    assert not bad.any(), (f"list {name}, K {k}: {int(bad.sum())} of {bad.size} delta elements differ "
                           f"(first {int(np.argmax(bad))})")
    return got


@pytest.mark.parametrize("name", ["A", "A3"])
@pytest.mark.parametrize("k", K_SWEEP)
def test_k_sweep(name, k):
    got = _check(name, k)
    if k in (33, 65):  # against arithmetic that is not the oracle's
        L = D.dlist(name)
        seeds, coefs, d0, _ = _inputs(name, k)
        ref = D.accumulate_ref(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0, device=_dev())
        assert np.array_equal(D.bits32(got), D.bits32(ref)), f"list {name}, K {k}: differs from the independent reference"


@pytest.mark.parametrize("name", ["A7", "PAR"])
@pytest.mark.parametrize("k", [20, 65])
def test_odd_offsets_at_phase_0(name, k):
    """Lists that keep the stream phase and flip the offsets' parity (see the module's text)."""
    _check(name, k)


@pytest.mark.parametrize("k", K_SWEEP)
def test_k_sweep_one_slice_per_pass(k, monkeypatch):
    """FKS_BS_SLICES=1: 32-seed passes, one slice per plan chunk (read per call, fks_run.cpp)."""
    monkeypatch.setenv("FKS_BS_SLICES", "1")
    _check("A", k)


@pytest.mark.parametrize("k", [20, 64, 70])
def test_the_slice_kernel_is_what_runs(k):
    """List PATH has bf16 fast segments only, so every apply launch is the slice kernel's:
    ceil(K / 64) of them; the 19-seed kernels would take ceil(K / 19), which differs for every
    K >= 20."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), D.dlist("PATH")
    assert all(n % 16 == 0 for n in L.sizes) and all(o % 2 == 0 for o in L.off)
    seeds, coefs, d0, want = _inputs("PATH", k)
    buf, view = D.guarded(d0, dev)
    specs = L.specs(dev)
    with codec.profile() as prof:
        codec.delta_accumulate(specs, seeds, coefs, view)
    torch.cuda.synchronize()
    bs, small = -(-k // K_BS_PASS), -(-k // K_MAX_PASS)
    print(f"delta slice path proof: K {k}: {prof.n_apply} apply launches (slice kernel {bs}, 19-seed kernels {small})")
    assert bs != small and prof.n_apply == bs
    assert D.guards_intact(buf, view)
    assert np.array_equal(D.bits32(view), D.bits32(want))


def test_multi_block_chunks():
    """K = 70 = 64 + 6 on (2^20, 624 * 48 + 32): many tasks per wave, a partial last task, the
    second segment beginning inside a task; on a base of 8 modulo 16 as well."""
    for shift in (0, 2):
        _check("BLOCKS", 70, shift)


def test_window_cache(capsys):
    """A reconstruct with cache_windows=True leaves the window cache attached; delta calls of more
    than 32 seeds then take their windows through it (jw_cache in fks_run.cpp).  The delta of the
    same 70 seeds, and of 70 seeds that share 40 of them, equal what the calls give once the cache
    is released -- and the oracle.  Whether the cache had the seeds is printed, not asserted: it
    tells whether the delta plan's slice chunks (bs_hash) are the update plan's."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), D.dlist("BLOCKS")
    seeds, coefs, d0, want = _inputs("BLOCKS", 70)
    other, ocoefs = D.seeds_coefs(30, seed=501)
    seeds2, coefs2 = seeds[:40] + other, coefs[:40] + ocoefs
    arrays = rand_params(L.sizes, "bfloat16", seed=21)
    params = [from_np(a, "bfloat16", dev) for a in arrays]
    specs = [codec.ParamSpec(p, lr=1e-5, weight_decay=0.0) for p in params]
    vals = [c * 1e5 for c in coefs]

    def both():
        out = []
        for s, c in ((seeds, coefs), (seeds2, coefs2)):
            buf, view = D.guarded(d0, dev)
            codec.delta_accumulate(specs, s, c, view)
            torch.cuda.synchronize()
            assert D.guards_intact(buf, view)
            out.append(view.cpu().numpy())
        return out

    codec.jwin_release()
    try:
        codec.directional_step(specs, seeds, vals, cache_windows=True)
        attached = bool(codec._jwin)
        before = [to_np(p) for p in params]
        h0, m0 = codec.jwin_stats()
        cached = both()
        h1, m1 = codec.jwin_stats()
    finally:
        codec.jwin_release()
    plain = both()
    with capsys.disabled():
        print(f"\ndelta window cache: attached {attached}; two delta calls of 70 seeds: {h1 - h0} seeds found in the "
              f"cache, {m1 - m0} jumped into it")
    for i, (a, b) in enumerate(zip(cached, plain)):
        assert np.array_equal(D.bits32(a), D.bits32(b)), f"call {i}: the window cache changed the delta"
    assert np.array_equal(D.bits32(plain[0]), D.bits32(want))
    want2 = D.oracle_accumulate(L.sizes, L.dtypes, L.frozen, seeds2, coefs2, d0)
    assert np.array_equal(D.bits32(plain[1]), D.bits32(want2))
    for p, b in zip(params, before):  # the delta calls leave the parameters alone
        assert np.array_equal(to_np(p), b)


@pytest.mark.parametrize("case", D.EDGE_CASES)
def test_edge_values(case):
    """Accumulating into +-0, +-inf, NaN and subnormals with +-0, subnormal and overflowing
    coefficients, K = 40 (the slice kernel on the bf16 tensor, the 19-seed kernel on the f32 one),
    against the independent reference; where NaN is expected comes from the inputs alone."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), D.dlist("EDGE")
    seeds, coefs, d0 = D.edge_inputs(case)
    ref = D.accumulate_ref(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0, device=dev).cpu()
    nnan = D.check_edge_reference(case, ref, d0, D.draws_mt(L.sizes, L.dtypes, seeds[-1]))
    buf, view = D.guarded(d0, dev)
    codec.delta_accumulate(L.specs(dev), seeds, coefs, view)
    torch.cuda.synchronize()
    assert D.guards_intact(buf, view)
    print(f"delta edge values ({case}): {nnan} NaN expected of {L.total}")
    assert_bitwise(view.cpu().numpy(), ref.numpy(), "float32", f"edge case {case}")
