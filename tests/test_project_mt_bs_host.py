"""fks_project_mt_bs without a device: header and exports, fks_project_mt_multi's argument errors on
both flavours of the CPU generator's stream, the torch_rocm refusal, the workspace arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_project_mt_multi_host import EINVAL, ENOTSUP, FAKE, FLAGS, ROOT, SIZES, _err, _lib, _tensors, _vecs


def _call(L, arr, nt, vecs, nvec=2, k=2, shard=0, nshards=1, out=FAKE + (1 << 31), ws=FAKE + (1 << 32),
          ws_bytes=1 << 30, seeds=True):
    s = np.array([1, 2, 3][:max(k, 1)], dtype=np.uint64)
    return L.fks_project_mt_bs(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None, k,
                               ctypes.addressof(vecs) if vecs is not None else None, nvec, shard, nshards, out, ws,
                               ws_bytes, None)


def _size(L, arr, nt, k, nvec):
    nbytes = ctypes.c_size_t(0)
    rc = L.fks_project_mt_bs_workspace_size(ctypes.addressof(arr), nt, k, nvec, ctypes.byref(nbytes))
    return rc, nbytes.value


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "fks.h")).read()
    for name in ("fks_project_mt_bs", "fks_project_mt_bs_workspace_size"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("what,kw", [
    ("negative nvec", dict(nvec=-1)), ("null out", dict(out=None)), ("misaligned out", dict(out=FAKE + (1 << 31) + 4)),
    ("shard past the end", dict(shard=2, nshards=2)), ("negative shard", dict(shard=-1, nshards=2)),
    ("no shards", dict(shard=0, nshards=0)), ("null workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=FAKE + (1 << 32) + 4)), ("workspace too small", dict(ws_bytes=64)),
    ("null seeds", dict(seeds=False)), ("negative k", dict(k=-1)),
])
def test_einval_from_the_scalar_arguments(what, kw, flags):
    N, L = _lib()
    arr = _tensors(N, SIZES, flags)
    assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2), **kw) == -EINVAL and _err(L), what


@pytest.mark.parametrize("flags", FLAGS)
def test_einval_from_the_vector_list(flags):
    N, L = _lib()
    nt, arr = len(SIZES), _tensors(N, SIZES, flags)
    assert _call(L, arr, nt, None) == -EINVAL and "vector" in _err(L)  # NULL vecs, nvec > 0, nt > 0
    v = _vecs(N, SIZES, 2)
    v[nt + 2].dtype = 3  # a dtype outside the three
    assert _call(L, arr, nt, v) == -EINVAL and "dtype" in _err(L)
    v = _vecs(N, SIZES, 2)
    v[nt + 0].data = None  # a live tensor's entry of the second vector
    assert _call(L, arr, nt, v) == -EINVAL and "vector 1, tensor 0" in _err(L)
    for dtype, off in ((1, 1), (2, 1), (0, 2)):  # 2-byte types at an odd address, f32 at addr + 2
        v = _vecs(N, SIZES, 2, dtype=dtype)
        v[2].data += off
        assert _call(L, arr, nt, v) == -EINVAL and "misaligned" in _err(L), (dtype, off)
    v = _vecs(N, SIZES, 2, dtype=0)
    v[2].data += 4  # aligned to the element size only is enough: the error that remains is the workspace's
    assert _call(L, arr, nt, v, ws_bytes=64) == -EINVAL and "workspace" in _err(L)


def test_refuses_the_rocm_stream_and_takes_the_trivial_calls():
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2)) == -ENOTSUP
    assert "FKS_STREAM_ROCM" in _err(L) and re.search(r"\bfks_project_multi\b", _err(L))
    assert _size(L, arr, len(SIZES), 4, 1)[0] == -ENOTSUP
    arr = _tensors(N, SIZES, 0)
    for kw in (dict(k=0), dict(nvec=0)):  # nothing to compute: no workspace, no device
        assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2), ws=None, ws_bytes=0, out=None, **kw) == 0, _err(L)


def test_workspace_grows_with_k_up_to_a_pass_and_is_constant_from_there():
    N, L = _lib()
    sizes = [4096, 1000, 3, 700_016, 7, 65536, 3_000_001]

    def size(k, nvec=1, dtype=1):
        rc, b = _size(L, _tensors(N, sizes, 0, dtype=dtype, frozen_at=-1), len(sizes), k, nvec)
        assert rc == 0, _err(L)
        return b

    by_k = [size(k) for k in range(0, 66)]
    assert all(b >= a for a, b in zip(by_k, by_k[1:])) and by_k[1] < by_k[32] < by_k[64] and by_k[-1] % 8 == 0
    assert len({by_k[64], by_k[65], size(97), size(4096), size(10**6)}) == 1
    assert size(64, nvec=3) > size(64, nvec=1)  # the per-call table
    assert size(64, dtype=0) < size(64)  # f32 tensors have no bit-sliced windows: 19 seeds' at most
    arr = _tensors(N, sizes, 0, frozen_at=-1)
    v = _vecs(N, sizes, 1, frozen_at=-1)
    need = size(2)
    assert _call(L, arr, len(sizes), v, nvec=1, k=2, ws_bytes=need - 1) == -EINVAL  # one byte short is refused
    assert "workspace" in _err(L) and str(need) in _err(L)
