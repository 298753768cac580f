"""fks_expand_mt_bs without a device (pointers are fake and never dereferenced): header and exports,
fks_expand_mt_multi's argument errors with the same code on both flavours of the CPU generator's
stream, the torch_rocm refusal, the workspace against its stated layout."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_expand_host import EINVAL, ENOTSUP, FAKE, ROOT, SIZES, _err, _lib, _outs, _tensors
from test_expand_mt_host import CPU, LIBM, WS_SIZES
from test_expand_mt_host import _call as _multi_call


def _call(L, arr, nt, outs, nvec=2, k=2, shard=0, nshards=1, ws=FAKE + (1 << 32), ws_bytes=1 << 30, seeds=True,
          coefs=True, betas=False):
    s = np.arange(1, max(k, 1) + 1, dtype=np.uint64)
    c = np.ones(max(k, 1) * max(nvec, 1), dtype=np.float64)
    b = np.full(max(nvec, 1), 0.5, dtype=np.float64)
    return L.fks_expand_mt_bs(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None,
                              c.ctypes.data if coefs else None, k, ctypes.addressof(outs) if outs is not None else None,
                              b.ctypes.data if betas else None, nvec, shard, nshards, ws, ws_bytes, None)


def _size(L, arr, nt, k, nvec=1, shard=0, nshards=1, fn="fks_expand_mt_bs_workspace_size"):
    nbytes = ctypes.c_size_t(0)
    rc = getattr(L, fn)(ctypes.addressof(arr), nt, k, nvec, shard, nshards, ctypes.byref(nbytes))
    assert rc == 0, _err(L)
    return nbytes.value


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    with open(os.path.join(ROOT, "include", "fks.h")) as f:
        hdr = f.read()
    for name in ("fks_expand_mt_bs", "fks_expand_mt_bs_workspace_size"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive


@pytest.mark.parametrize("flags", [CPU, LIBM])
@pytest.mark.parametrize("what,kw", [
    ("negative nvec", dict(nvec=-1)), ("shard past the end", dict(shard=2, nshards=2)),
    ("negative shard", dict(shard=-1, nshards=2)), ("no shards", dict(shard=0, nshards=0)),
    ("null workspace", dict(ws=None)), ("misaligned workspace", dict(ws=FAKE + (1 << 32) + 4)),
    ("workspace too small", dict(ws_bytes=64)), ("workspace too small, with betas", dict(ws_bytes=64, betas=True)),
    ("workspace without the staging area", dict(k=33, ws_bytes=4 * 74_096)),
    ("null seeds", dict(seeds=False)), ("null coefs", dict(coefs=False)), ("negative k", dict(k=-1)),
])
def test_einval_from_the_scalar_arguments_as_expand_mt_multi(what, kw, flags):
    N, L = _lib()
    arr = _tensors(N, SIZES, flags)
    assert _multi_call(L, arr, len(SIZES), _outs(N, SIZES, 2), **kw) == -EINVAL, what
    assert _call(L, arr, len(SIZES), _outs(N, SIZES, 2), **kw) == -EINVAL and _err(L), what


def test_einval_from_the_output_list_and_the_trivial_calls():
    N, L = _lib()
    nt, arr = len(SIZES), _tensors(N, SIZES, CPU)
    assert _call(L, arr, nt, None) == -EINVAL and "output" in _err(L)  # NULL outs, nvec > 0, nt > 0
    v = _outs(N, SIZES, 2)
    v[nt + 2].dtype = 3  # a dtype outside the three
    assert _call(L, arr, nt, v) == -EINVAL and "dtype" in _err(L)
    v = _outs(N, SIZES, 2)
    v[nt + 0].data = None  # a live tensor's entry of the second output
    assert _call(L, arr, nt, v) == -EINVAL and "output 1, tensor 0" in _err(L)
    for dtype, off in ((0, 2), (1, 1), (2, 1)):  # f32 at 2 bytes, 2-byte types at an odd address
        v = _outs(N, SIZES, 2, dtype=dtype)
        v[2].data += off
        assert _call(L, arr, nt, v) == -EINVAL and "misaligned" in _err(L), (dtype, off)
    v = _outs(N, SIZES, 2, dtype=1)
    v[2].data += 2  # aligned to the element size only is enough: the error that remains is the workspace's
    assert _call(L, arr, nt, v, ws_bytes=64) == -EINVAL and "workspace" in _err(L)
    mixed = _tensors(N, SIZES, CPU)
    mixed[2].flags |= N.STREAM_ROCM
    assert _call(L, mixed, nt, _outs(N, SIZES, 2)) == -EINVAL and "same z stream" in _err(L)
    assert _call(L, arr, nt, None, nvec=0, ws=None, ws_bytes=0) == 0, _err(L)  # no outputs: no workspace, no device
    assert _call(L, arr, 0, None, ws=None, ws_bytes=0) == 0, _err(L)  # no tensors


def test_refuses_the_rocm_stream():
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, len(SIZES), _outs(N, SIZES, 2)) == -ENOTSUP
    assert "FKS_STREAM_ROCM" in _err(L) and re.search(r"\bfks_expand_multi\b", _err(L))
    nbytes = ctypes.c_size_t(0)
    assert L.fks_expand_mt_bs_workspace_size(ctypes.addressof(arr), len(SIZES), 4, 2, 0, 1, ctypes.byref(nbytes)) == -ENOTSUP


@pytest.mark.parametrize("dtype", [0, 1])
def test_workspace_against_its_layout(dtype):
    """[table | windows | sink | staging area].  bf16 (dtype 1): WS_SIZES holds bf16 fast segments AND
    irregular work, so the windows grow to 32 seeds and the staging area appears past 19; f32: no
    bit-sliced pass, fks_expand_mt_multi's sizes at every k."""
    N, L = _lib()
    nt, total = len(WS_SIZES), sum(WS_SIZES)
    arr = _tensors(N, WS_SIZES, CPU, dtype=dtype, frozen_at=-1)
    multi = lambda k, *a: _size(L, arr, nt, k, 1, *a, fn="fks_expand_mt_multi_workspace_size")  # noqa: E731
    size = lambda k, *a: _size(L, arr, nt, k, 1, *a)  # noqa: E731
    assert size(0) == multi(0) and size(0) % 8 == 0  # no seeds: fks_expand_mt_multi's path
    if dtype == 0:
        assert [size(k) for k in (19, 32, 33)] == [multi(k) for k in (19, 32, 33)]
        return
    w19 = multi(2) - multi(1)  # one seed's windows of a 19-seed pass
    win = lambda k: size(k) - size(0) - (4 * total if k > 19 else 0)  # noqa: E731  (staged past 19: the irregular work)
    w32, rem = divmod(win(32), 32)  # ... and of a bit-sliced pass: the slice kernel's plan, an even chunk count
    assert rem == 0 and w32 % (4 * 624 * 2) == 0 and 32 * w32 > 19 * w19
    for k in (1, 2, 19, 20, 31):  # one area, the larger of the two passes; no staging area up to 19 seeds
        assert win(k) == max(min(k, 19) * w19, k * w32), k
    assert size(33) == size(32) and size(4055) == size(32)  # the windows stop at 32 seeds
    only = _tensors(N, [4096, 65536], CPU, dtype=1, frozen_at=-1)  # bf16 fast segments alone
    assert _size(L, only, 2, 33) - _size(L, only, 2, 32) == 4 * (4096 + 65536)  # staged from 33 seeds on
    st = [_size(L, only, 2, 33, 1, sh, 2) - _size(L, only, 2, 32, 1, sh, 2) for sh in range(2)]  # two shards:
    assert all(0 < x < 4 * (4096 + 65536) for x in st) and sum(st) >= 4 * (4096 + 65536), st  # their spans cover the list
    arr = _tensors(N, WS_SIZES, CPU)  # (_outs leaves the frozen tensor's entry NULL)
    need = size(33)
    assert _call(L, arr, nt, _outs(N, WS_SIZES, 1), nvec=1, k=33, ws_bytes=need - 1) == -EINVAL  # one byte short is refused
    assert "workspace" in _err(L) and str(need) in _err(L)
