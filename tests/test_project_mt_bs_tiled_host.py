"""fks_project_mt_bs_tiled without a device: header and exports, fks_project_mt_bs's argument errors,
the torch_rocm refusal, the trivial calls."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_project_mt_multi_host import EINVAL, ENOTSUP, FAKE, FLAGS, ROOT, SIZES, _err, _lib, _tensors, _vecs


def _call(L, arr, nt, vecs, nvec=2, k=2, shard=0, nshards=1, out=FAKE + (1 << 31), ws=FAKE + (1 << 32),
          ws_bytes=1 << 30, seeds=True):
    s = np.array([1, 2, 3][:max(k, 1)], dtype=np.uint64)
    return L.fks_project_mt_bs_tiled(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None, k,
                                     ctypes.addressof(vecs) if vecs is not None else None, nvec, shard, nshards, out, ws,
                                     ws_bytes, None)


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "fks.h")).read()
    for name in ("fks_project_mt_bs_tiled", "fks_project_mt_bs_tiled_workspace_size"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("what,kw", [
    ("negative nvec", dict(nvec=-1)), ("null out", dict(out=None)), ("misaligned out", dict(out=FAKE + (1 << 31) + 4)),
    ("shard past the end", dict(shard=2, nshards=2)), ("negative shard", dict(shard=-1, nshards=2)),
    ("no shards", dict(shard=0, nshards=0)), ("null workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=FAKE + (1 << 32) + 4)), ("workspace too small", dict(ws_bytes=64)),
    ("null seeds", dict(seeds=False)), ("negative k", dict(k=-1)), ("null vecs", dict(vecs=None)),
    ("bad vector dtype", dict(bad=lambda v, nt: setattr(v[nt + 2], "dtype", 3))),
    ("null vector pointer", dict(bad=lambda v, nt: setattr(v[nt + 0], "data", None))),
    ("misaligned vector pointer", dict(bad=lambda v, nt: setattr(v[2], "data", v[2].data + 1))),
])
def test_einval_before_any_device_work(what, kw, flags):
    N, L = _lib()
    arr, vecs = _tensors(N, SIZES, flags), _vecs(N, SIZES, 2)
    kw = dict(kw)
    kw.pop("bad", lambda v, nt: None)(vecs, len(SIZES))
    assert _call(L, arr, len(SIZES), kw.pop("vecs", vecs), **kw) == -EINVAL and _err(L), what


def test_refuses_the_rocm_stream_and_takes_the_trivial_calls():
    N, L = _lib()
    nbytes = ctypes.c_size_t(0)
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2)) == -ENOTSUP
    assert "FKS_STREAM_ROCM" in _err(L) and re.search(r"\bfks_project_multi\b", _err(L))
    assert L.fks_project_mt_bs_tiled_workspace_size(ctypes.addressof(arr), len(SIZES), 4, 1, ctypes.byref(nbytes)) == -ENOTSUP
    arr = _tensors(N, SIZES, 0)
    for nt, kw in ((len(SIZES), dict(k=0)), (len(SIZES), dict(nvec=0)), (0, dict(k=0))):  # nothing to compute: no device
        assert _call(L, arr, nt, _vecs(N, SIZES, 2), ws=None, ws_bytes=0, out=None, **kw) == 0, _err(L)
    assert L.fks_project_mt_bs_tiled_workspace_size(ctypes.addressof(arr), 0, 4, 3, ctypes.byref(nbytes)) == 0  # no tensors
