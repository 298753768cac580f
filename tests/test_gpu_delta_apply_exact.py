"""fks_delta_apply (fks_delta_apply_kernel): p = dtype(fmaf(f32(decay_i), p, -delta)), one fma and
one rounding, against tests/delta_ref.py's apply_ref (exact_f32.fma32, then torch's rounding to
the dtype) bit for bit, and against O.delta_apply.

Inputs (delta_ref.apply_inputs): f32, bf16 and f16 tensors of 4099, 4096, 7 and 1000 elements in
one list, so that one launch switches over the three dtypes; a 2,000-element band where
delta = -+ulp_dtype(p) / 2, an exact tie at decay 1 (the fma's own for f32, the rounding to
bf16 / f16 otherwise); +-0, +-inf, NaN, f16 overflow, inf - inf and a subnormal delta at the
head of every tensor; decays 1, 0.999959, 1 - 1e-9 (1 as f32), 0 and -0, each for the whole
list and the five mixed over the tensors of one call.  Where NaN is expected comes from the
inputs alone, so 'NaN matches any NaN' hides nothing.

Layout: a frozen tensor (its bits stay, its range of delta is skipped), an empty one, a
non-contiguous view (staged, written back through the view), a view at element offset 1 of
its storage, guards round delta and round the odd view; a list of frozen and empty tensors
only is a no-op."""
import numpy as np
import pytest
import torch

import delta_ref as D
from conftest import assert_bitwise
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", range(6))
def test_ties_and_edge_values(which):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    dts, ps, delta = D.apply_inputs()
    decays = D.apply_decay_sets()[which]
    ts = [p.clone().to(dev) for p in ps]
    buf, view = D.guarded(delta, dev)
    codec.delta_apply([codec.ParamSpec(t) for t in ts], view, decays)
    torch.cuda.synchronize()
    assert D.guards_intact(buf, view) and np.array_equal(D.bits32(view), D.bits32(delta)), "delta was written"
    oracle = D.oracle_apply(dts, ps, delta, decays)
    off, nnan, total = 0, 0, 0
    for i, (d, p, t) in enumerate(zip(dts, ps, ts)):
        dl = delta[off:off + p.numel()]
        off += p.numel()
        ref = D.apply_ref(p, d, dl, decays[i])
        exp_nan = D.apply_expected_nan(p, dl, decays[i])
        assert torch.equal(torch.isnan(ref.float()), exp_nan), (i, d)
        nnan += int(exp_nan.sum())
        total += p.numel()
        what = f"tensor {i} ({p.numel()} x {d}), decay {decays[i]}"
        assert_bitwise(D.stored(t), D.stored(ref), d, what)
        assert_bitwise(D.stored(t), oracle[i], d, what + " (oracle)")
    assert 0 < nnan < total // 100
    print(f"delta apply, decays {which}: {nnan} NaN expected of {total}")


def test_frozen_empty_staged_and_offset_views():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    g = torch.Generator().manual_seed(43)

    def rnd(shape, dtype):
        return (torch.randn(shape, generator=g) * 0.02).to(D.TD[dtype]).to(dev)

    base = rnd((64, 100), "bfloat16")
    base0 = base.clone()
    staged = base[:, :50]
    assert not staged.is_contiguous()
    store = torch.full((1 + 1000 + 1,), D.GUARD, dtype=torch.float16, device=dev)
    odd = store[1:1001]
    odd.copy_(rnd(1000, "float16"))
    assert odd.storage_offset() == 1 and odd.data_ptr() % 4 == 2
    dts = ["float32", "bfloat16", "float16", "bfloat16", "float16", "bfloat16"]
    ts = [rnd(4099, "float32"), rnd(1000, "bfloat16"), torch.empty(0, dtype=torch.float16, device=dev), staged, odd,
          rnd(7, "bfloat16")]
    frozen = [False, True, False, False, False, False]
    decays = [0.999959, 0.5, 1.0, 1.0, 0.999959, 0.0]
    before = [t.detach().clone().contiguous().cpu() for t in ts]
    total = sum(t.numel() for t in ts)
    delta = torch.randn(total, generator=g) * 1e-3
    buf, view = D.guarded(delta, dev, shift=2)
    codec.delta_apply([codec.ParamSpec(t, frozen=f) for t, f in zip(ts, frozen)], view, decays)
    torch.cuda.synchronize()
    assert D.guards_intact(buf, view) and np.array_equal(D.bits32(view), D.bits32(delta))
    oracle = D.oracle_apply(dts, [b.reshape(-1) for b in before], delta, decays, frozen=[int(f) for f in frozen])
    off = 0
    for i, (d, t, b) in enumerate(zip(dts, ts, before)):
        n = t.numel()
        want = b if frozen[i] else D.apply_ref(b.reshape(-1), d, delta[off:off + n], decays[i])
        off += n
        assert np.array_equal(D.to_bits(t).reshape(-1), D.to_bits(want).reshape(-1)), f"tensor {i} ({d})"
        assert np.array_equal(D.to_bits(t).reshape(-1), D.as_uint(oracle[i]).reshape(-1)), f"tensor {i} ({d}) (oracle)"
    assert not np.array_equal(D.to_bits(staged), D.to_bits(before[3]))  # written through the view
    assert np.array_equal(D.to_bits(base[:, 50:]), D.to_bits(base0[:, 50:])), "the rest of the view's base was written"
    g16 = D.to_bits(torch.tensor([D.GUARD], dtype=torch.float16))[0]
    sb = D.to_bits(store)
    assert sb[0] == g16 and sb[-1] == g16, "a guard of the odd view was written"


def test_only_frozen_and_empty_tensors():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    ts = [torch.ones(1000, dtype=torch.bfloat16, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
          torch.ones(7, dtype=torch.float32, device=dev)]
    delta = torch.full((1007,), 0.5, dtype=torch.float32)
    buf, view = D.guarded(delta, dev)
    codec.delta_apply([codec.ParamSpec(t, frozen=True) for t in ts], view, [0.5, 0.5, 0.5])
    torch.cuda.synchronize()
    assert D.guards_intact(buf, view) and bool((view == 0.5).all())
    assert bool((ts[0] == 1).all()) and bool((ts[2] == 1).all())
