"""fks_delta_accumulate on the torch_rocm stream (fks_philox_vec_kernel<kModeDelta>), the form the
seed-sharded reconstruct takes on the default stream, on the paths its tests never reached:

* whole 16-byte runs (phx_vitem with phx_load8<FKS_F32>: two 16-byte loads per run) -- taken by
  a tensor whose delta address is 16-byte aligned, for the rows whose four runs lie inside the
  tensor: from 3 x 256 x cap + 8 elements on.  List W = (8 S + 1025, 1000), S = 256 x cap, has
  two whole rows, a ragged third one and an unaligned tensor behind; W + o puts a tensor of
  1000 + o elements in front, so that the big tensor's delta address takes every offset modulo
  16 bytes, and the base itself is 0 or 8 modulo 16: the aligned combinations take whole runs,
  the others the per-item path, with the same bits;
* several dtypes in one call, within one wave and with a table longer than the LDS copy;
* live values in the buffer, and the edge values of tests/delta_ref.py.

Reference: torch's own draws on the device (torch.normal per tensor in list order after
torch.manual_seed), folded by exact_f32.fma32 there; every element is compared, and the guards
round the buffer must keep their bits."""
import numpy as np
import pytest
import torch

import delta_ref as D
from conftest import assert_bitwise
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

MODE = "torch_rocm"
DTYPES = ["float32", "bfloat16", "float16"]
K_PHX = 32  # kPhxSeeds: seeds per launch (fks_internal.h)


def _S():
    from fate_llm.algo.fedkseed import codec
    return 256 * codec.rocm_grid_cap()


def _w(front, dtype):
    sizes = [8 * _S() + 1025, 1000]
    return D.DList(sizes if front is None else [1000 + front] + sizes, dtype)


def _check(L, k, seed, shifts=(0, 2), what=""):
    """one reference, one guarded call per base alignment"""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    seeds, coefs = D.seeds_coefs(k, seed=seed, scale=1e-4)
    d0 = D.prefill(L.total, seed=5)
    ref = D.accumulate_ref_rocm(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0, dev)
    specs = L.specs(dev)
    for shift in shifts:
        buf, view = D.guarded(d0, dev, shift)
        codec.delta_accumulate(specs, seeds, coefs, view, stream_mode=MODE)
        torch.cuda.synchronize()
        assert D.guards_intact(buf, view), f"{what}, base {4 * shift} mod 16: a guard element was written"
        bad = view.view(torch.int32) != ref.view(torch.int32)
        assert not bool(bad.any()), (f"{what}, base {4 * shift} mod 16: {int(bad.sum())} of {bad.numel()} delta "
                                     f"elements differ (first {int(bad.nonzero()[0])})")
        for i, f in enumerate(L.frozen):
            if f:
                assert np.array_equal(D.bits32(view[L.off[i]:L.off[i + 1]]), D.bits32(d0)[L.off[i]:L.off[i + 1]])


@pytest.mark.parametrize("front", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 33])
def test_whole_runs_and_every_alignment(front, dtype, k):
    _dev()
    L = _w(front, dtype)
    assert max(L.sizes) >= 3 * _S() + 8  # long enough for whole runs
    _check(L, k, seed=300 + k, what=f"W front {front} {dtype} K {k}")


def test_several_dtypes_in_one_wave():
    """test_gpu_project.py's seven tensors of at most 4096 elements: a wave spans two or three
    tensors of different dtypes; the third is frozen."""
    dts = ["bfloat16", "float32", "float16", "bfloat16", "float32", "float16", "float32"]
    _check(D.DList([256, 1000, 100, 8, 200, 256, 4096], dts, frozen=(2,)), 33, seed=340, what="seven tensors")


def test_table_longer_than_the_lds_copy():
    """600 tensors of 1 .. 41 elements, three dtypes: the kernel reads its table from device memory."""
    n = 600
    _check(D.DList([(7 * i) % 41 + 1 for i in range(n)], [DTYPES[i % 3] for i in range(n)]), 33, seed=341,
           what="600 tensors")


@pytest.mark.parametrize("k", [1, 33])
def test_launches_per_pass(k):
    """One launch per 32 seeds."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    L = _w(None, "bfloat16")
    seeds, coefs = D.seeds_coefs(k, seed=350)
    delta = torch.zeros(L.total, dtype=torch.float32, device=dev)
    specs = L.specs(dev)
    with codec.profile() as prof:
        codec.delta_accumulate(specs, seeds, coefs, delta, stream_mode=MODE)
    torch.cuda.synchronize()
    print(f"delta torch_rocm path proof: K {k}: {prof.n_apply} launches (expected {-(-k // K_PHX)})")
    assert prof.n_apply == -(-k // K_PHX)


@pytest.mark.parametrize("case", D.EDGE_CASES)
def test_edge_values(case):
    """tests/delta_ref.py's edge inputs on this stream, K = 40 (two launches); where NaN is expected
    comes from the inputs and torch's last draws alone."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), D.dlist("EDGE")
    seeds, coefs, d0 = D.edge_inputs(case)
    ref = D.accumulate_ref_rocm(L.sizes, L.dtypes, L.frozen, seeds, coefs, d0, dev).cpu()
    nnan = D.check_edge_reference(case, ref, d0, D.draws_rocm(L.sizes, L.dtypes, seeds[-1], dev))
    buf, view = D.guarded(d0, dev)
    codec.delta_accumulate(L.specs(dev), seeds, coefs, view, stream_mode=MODE)
    torch.cuda.synchronize()
    assert D.guards_intact(buf, view)
    print(f"delta edge values, torch_rocm ({case}): {nnan} NaN expected of {L.total}")
    assert_bitwise(view.cpu().numpy(), ref.numpy(), "float32", f"edge case {case}")
