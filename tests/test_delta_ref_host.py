"""tests/delta_ref.py against the oracle, on the CPU: the independent references of the delta
operations (oracle generator draws folded by exact_f32.fma32; fma32 and torch's rounding for the
apply) equal oracle/fks_oracle.c's fko_delta_accumulate / fko_delta_apply (libm's fmaf) bit for
bit, NaN = NaN, on the MT19937-stream lists the GPU tests use -- at each list's smallest K there
-- and on their edge inputs.  The GPU tests' K sweeps use the oracle (0.06 s where the
independent reference takes over a second); this file is what lets them.  It also shows that the
conditions the edge cases put on the reference alone hold: the NaN sets are the ones the inputs
dictate and stay under 1 % of the elements, and the subnormal case holds non-zero subnormal sums.

List BLOCKS (1,078,016 elements, K = 70) is left to the oracle alone: no GPU test uses the
independent reference on it."""
import numpy as np
import pytest
import torch

import delta_ref as D
from conftest import assert_bitwise


def _same_f32(ref: torch.Tensor, want: np.ndarray, what):
    assert_bitwise(ref.numpy(), want, "float32", what)


@pytest.mark.parametrize("name,k", [("A", 20), ("A3", 20), ("A7", 20), ("PAR", 20), ("PATH", 20), ("M", 2), ("MF", 2)])
def test_accumulate_ref_equals_the_oracle(name, k):
    L = D.dlist(name)
    seeds, coefs = D.seeds_coefs(k, seed=11 + k)
    d0 = D.prefill(L.total)
    ref = D.accumulate_ref(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0)
    want = D.oracle_accumulate(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0)
    assert not np.isnan(want).any()
    assert np.array_equal(D.bits32(ref), D.bits32(want))
    for i, f in enumerate(L.frozen):  # a frozen tensor's range keeps its bits, the rest moved
        same = D.bits32(ref)[L.off[i]:L.off[i + 1]] == D.bits32(d0)[L.off[i]:L.off[i + 1]]
        assert same.all() if f else not same.all() or L.sizes[i] == 0, i


@pytest.mark.parametrize("case", D.EDGE_CASES)
def test_accumulate_ref_on_edge_values(case):
    L = D.dlist("EDGE")
    seeds, coefs, d0 = D.edge_inputs(case)
    ref = D.accumulate_ref(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0)
    nnan = D.check_edge_reference(case, ref, d0, D.draws_mt(L.sizes, L.dtypes, seeds[-1]))
    want = D.oracle_accumulate(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0)
    _same_f32(ref, want, case)
    print(f"delta edge case {case}: {nnan} NaN of {L.total}")
    if case != "overflow":  # finite terms leave the planted infinities as they are
        for o in L.off[:-1]:
            assert np.array_equal(D.bits32(ref)[o + 2:o + 4], D.bits32(d0)[o + 2:o + 4])


def test_edge_coefficients_are_what_they_claim():
    """1e-42 is an f32 subnormal, -1e-45 rounds to the smallest one, 1e39 to inf."""
    from exact_f32 import f32
    assert 0 < float(f32(1e-42)) < 2.0 ** -126
    assert float(f32(-1e-45)) == -(2.0 ** -149)
    assert np.isinf(f32(1e39))
    _, coefs, _ = D.edge_inputs("subnormal")
    assert all(abs(float(f32(c))) < 2.0 ** -126 for c in coefs)


@pytest.mark.parametrize("which", range(6))
def test_apply_ref_equals_the_oracle(which):
    dts, ps, delta = D.apply_inputs()
    decays = D.apply_decay_sets()[which]
    want = D.oracle_apply(dts, ps, delta, decays)
    off, nan_total, n_total, ties = 0, 0, 0, 0
    for i, (d, p) in enumerate(zip(dts, ps)):
        dl = delta[off:off + p.numel()]
        off += p.numel()
        ref = D.apply_ref(p, d, dl, decays[i])
        exp_nan = D.apply_expected_nan(p, dl, decays[i])
        assert torch.equal(torch.isnan(ref.float()), exp_nan), (i, d)
        nan_total += int(exp_nan.sum())
        n_total += p.numel()
        assert_bitwise(D.stored(ref), want[i], d, f"tensor {i} ({d}), decay {decays[i]}")
        if float(np.float32(decays[i])) == 1.0 and p.numel() > D.BAND[1]:
            # the band holds exact ties: the result lies half an ulp from p - delta (but where p is
            # a power of two and delta leads towards zero: the ulp halves there and p - delta is exact)
            b = slice(*D.BAND)
            err = (ref[b].double() - (p[b].double() - dl[b].double())).abs()
            tie = err == dl[b].double().abs()
            assert bool((tie | (err == 0)).all()), (i, d)
            ties += int((tie & (p[b].float() != 0)).sum())
    assert 0 < nan_total < n_total // 100
    if which in (0, 2, 5):
        assert ties >= 1900 * (2 if which == 5 else 6)
    # f16 overflows to inf at decay 1: 6e4 + 6e3 is beyond the largest f16
    if which == 0:
        f16 = [i for i, d in enumerate(dts) if d == "float16"][0]
        got = D.apply_ref(ps[f16], "float16", delta[sum(p.numel() for p in ps[:f16]):][:ps[f16].numel()], 1.0)
        assert bool(torch.isinf(got[5])) and bool(torch.isinf(got[6]))
