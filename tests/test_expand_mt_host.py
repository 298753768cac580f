"""fks_expand_mt_multi from the host side, on a machine without a GPU: pointers are fake and never
dereferenced.  The symbols are in the header and exported; every argument error is -EINVAL, raised
from the arguments alone, before any device work, with a message; a FKS_STREAM_ROCM list is
-ENOTSUP naming fks_expand_multi; the trivial calls succeed; the workspace has no staging area up
to 19 seeds and one of 4 bytes per element of the shard's span beyond; codec.expand_mt_multi
raises its ValueErrors, and zo_utils.seed_expansion_on_stream_ refuses CPU parameters, before a
device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_expand_host import EINVAL, ENOTSUP, FAKE, FROZEN_AT, ROOT, SIZES, _err, _lib, _outs, _tensors

CPU, LIBM = 0, 16  # flags of the CPU generator's stream and its FKS_LIBM flavour


def _call(L, arr, nt, outs, nvec=2, k=2, shard=0, nshards=1, ws=FAKE + (1 << 32), ws_bytes=1 << 30, seeds=True,
          coefs=True, betas=False):
    s = np.arange(1, max(k, 1) + 1, dtype=np.uint64)
    c = np.ones(max(k, 1) * max(nvec, 1), dtype=np.float64)
    b = np.full(max(nvec, 1), 0.5, dtype=np.float64)
    return L.fks_expand_mt_multi(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None,
                                 c.ctypes.data if coefs else None, k,
                                 ctypes.addressof(outs) if outs is not None else None, b.ctypes.data if betas else None,
                                 nvec, shard, nshards, ws, ws_bytes, None)


def _size(L, arr, nt, k, nvec, shard=0, nshards=1):
    nbytes = ctypes.c_size_t(0)
    rc = L.fks_expand_mt_multi_workspace_size(ctypes.addressof(arr), nt, k, nvec, shard, nshards, ctypes.byref(nbytes))
    assert rc == 0, _err(L)
    return nbytes.value


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    with open(os.path.join(ROOT, "include", "fks.h")) as f:
        hdr = f.read()
    for name in ("fks_expand_mt_multi", "fks_expand_mt_multi_workspace_size"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive


@pytest.mark.parametrize("flags", [CPU, LIBM])
@pytest.mark.parametrize("what,kw", [
    ("negative nvec", dict(nvec=-1)),
    ("shard past the end", dict(shard=2, nshards=2)),
    ("negative shard", dict(shard=-1, nshards=2)),
    ("no shards", dict(shard=0, nshards=0)),
    ("null workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=FAKE + (1 << 32) + 4)),
    ("workspace too small", dict(ws_bytes=64)),
    ("workspace too small, with betas", dict(ws_bytes=64, betas=True)),
    ("workspace without the staging area", dict(k=20, ws_bytes=4 * 74_096)),
    ("null seeds", dict(seeds=False)),
    ("null coefs", dict(coefs=False)),
    ("negative k", dict(k=-1)),
])
def test_einval_from_the_scalar_arguments(what, kw, flags):
    N, L = _lib()
    assert LIBM == N.LIBM
    arr = _tensors(N, SIZES, flags)
    assert _call(L, arr, len(SIZES), _outs(N, SIZES, 2), **kw) == -EINVAL, what
    assert _err(L), what


def test_einval_from_the_output_list():
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, CPU)
    assert _call(L, arr, nt, None) == -EINVAL and "output" in _err(L)  # NULL outs, nvec > 0, nt > 0
    for dt in (3, -1):  # a dtype outside the three
        v = _outs(N, SIZES, 2)
        v[nt + 2].dtype = dt
        assert _call(L, arr, nt, v) == -EINVAL and "dtype" in _err(L)
    v = _outs(N, SIZES, 2)
    v[nt + 0].data = None  # a live tensor's entry of the second output
    assert _call(L, arr, nt, v) == -EINVAL and "output 1, tensor 0" in _err(L)
    for dtype, off in ((0, 2), (0, 1), (1, 1), (2, 1)):  # f32 at 2 bytes, 2-byte types at an odd address
        v = _outs(N, SIZES, 2, dtype=dtype)
        v[2].data += off
        assert _call(L, arr, nt, v) == -EINVAL and "misaligned" in _err(L), (dtype, off)
    # aligned to the element size only is enough: the error that remains is the workspace's
    for dtype, off in ((0, 4), (1, 2), (2, 2)):
        v = _outs(N, SIZES, 2, dtype=dtype)
        v[2].data += off
        assert _call(L, arr, nt, v, ws_bytes=64) == -EINVAL and "workspace" in _err(L), (dtype, off)
    # the entries of the empty and of the frozen tensor are ignored, whatever they hold
    v = _outs(N, SIZES, 2)
    for m in range(2):
        v[m * nt + 1].dtype = 77
        v[m * nt + FROZEN_AT].dtype = -5
        v[m * nt + FROZEN_AT].data = 3
    assert _call(L, arr, nt, v, ws_bytes=64) == -EINVAL and "workspace" in _err(L)
    # a bad tensor list is refused like everywhere: mixed streams
    mixed = _tensors(N, SIZES, CPU)
    mixed[2].flags |= N.STREAM_ROCM
    assert _call(L, mixed, nt, _outs(N, SIZES, 2)) == -EINVAL and "same z stream" in _err(L)


def test_refuses_the_rocm_stream():
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, len(SIZES), _outs(N, SIZES, 2)) == -ENOTSUP
    assert "fks_expand_multi" in _err(L) and "FKS_STREAM_ROCM" in _err(L)
    nbytes = ctypes.c_size_t(0)
    rc = L.fks_expand_mt_multi_workspace_size(ctypes.addressof(arr), len(SIZES), 4, 2, 0, 1, ctypes.byref(nbytes))
    assert rc == -ENOTSUP and "fks_expand_multi" in _err(L)
    # ... and the torch_rocm call names this one for the CPU generator's stream
    from test_expand_host import _call as rocm_call
    assert rocm_call(L, _tensors(N, SIZES, CPU), len(SIZES), _outs(N, SIZES, 2)) == -ENOTSUP
    assert "fks_expand_mt_multi" in _err(L)


def test_trivial_calls_succeed():
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, CPU)
    assert _call(L, arr, nt, None, nvec=0, ws=None, ws_bytes=0) == 0, _err(L)  # no outputs
    assert _call(L, arr, nt, None, nvec=0, k=0, ws=None, ws_bytes=0, seeds=False, coefs=False) == 0, _err(L)
    assert _call(L, arr, 0, None, ws=None, ws_bytes=0) == 0, _err(L)  # no tensors
    assert _call(L, arr, 0, None, nvec=0, k=0, ws=None, ws_bytes=0, seeds=False, coefs=False) == 0, _err(L)
    empty = _tensors(N, [0, 0], CPU, frozen_at=-1)  # an all-empty list: nothing to write
    assert _call(L, empty, 2, _outs(N, [0, 0], 2), ws=None, ws_bytes=0) == 0, _err(L)
    assert _call(L, empty, 2, _outs(N, [0, 0], 2), k=0, ws=None, ws_bytes=0, seeds=False, coefs=False) == 0, _err(L)
    frozen = _tensors(N, [0, 0, 0, 5], CPU)  # ... and one whose only elements are frozen
    assert _call(L, frozen, 4, _outs(N, [0, 0, 0, 5], 2), ws=None, ws_bytes=0) == 0, _err(L)
    assert _size(L, arr, 0, 4, 3) >= 0 and _size(L, arr, nt, 0, 0) >= 0
    small = ctypes.c_size_t(0)
    assert L.fks_expand_mt_multi_workspace_size(ctypes.addressof(arr), 1, 1, 1, 0, 1, None) == -EINVAL
    assert L.fks_expand_mt_multi_workspace_size(ctypes.addressof(arr), 1, -1, 1, 0, 1, ctypes.byref(small)) == -EINVAL
    assert L.fks_expand_mt_multi_workspace_size(ctypes.addressof(arr), 1, 1, -1, 0, 1, ctypes.byref(small)) == -EINVAL
    assert L.fks_expand_mt_multi_workspace_size(ctypes.addressof(arr), 1, 1, 1, 1, 1, ctypes.byref(small)) == -EINVAL


WS_SIZES = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001]  # every tensor live


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_workspace_size_and_the_staging_area(dtype):
    N, L = _lib()
    nt = len(WS_SIZES)
    arr = _tensors(N, WS_SIZES, CPU, dtype=dtype, frozen_at=-1)
    total = sum(WS_SIZES)
    # up to one pass: the table, the windows of min(k, 19) seeds, the sink -- no staging area
    by_k = [_size(L, arr, nt, k, 1) for k in (0, 1, 2, 19)]
    assert by_k[0] < by_k[1] < by_k[2] < by_k[3]
    assert by_k[2] - by_k[1] == by_k[1] - by_k[0]  # one seed's windows each
    assert by_k[3] - by_k[0] == 19 * (by_k[1] - by_k[0])
    assert (by_k[1] - by_k[0]) % (4 * 624) == 0  # 624 words per seed and plan chunk
    # one more seed: the same windows, and 4 bytes per element of the shard's span
    assert _size(L, arr, nt, 20, 1) - by_k[3] == 4 * total
    assert _size(L, arr, nt, 4055, 1) == _size(L, arr, nt, 20, 1)  # ... whatever the number of passes
    # one staging area whatever the output count: an output more costs its table entries only
    per_out = _size(L, arr, nt, 20, 2) - _size(L, arr, nt, 20, 1)
    assert 0 < per_out <= 16 * (nt + 16) + 256
    assert _size(L, arr, nt, 19, 2) - by_k[3] == per_out
    # the staging area follows the shard: it does not grow with the shard count, every shard's
    # fits the whole list's, and the shards' spans cover the list
    prev = 4 * total
    for ns in (1, 2, 3):
        st = [_size(L, arr, nt, 20, 1, sh, ns) - _size(L, arr, nt, 19, 1, sh, ns) for sh in range(ns)]
        assert all(0 < x <= prev for x in st), (ns, st)
        assert sum(st) >= 4 * total, (ns, st)
        assert max(st) <= 4 * (total // ns + 2 * 624 + 32), (ns, st)  # whole MT blocks, a ragged tensor's 16 tail words
        prev = max(st)
    # frozen and empty tensors at the ends shorten the span
    arr2 = _tensors(N, [5000] + WS_SIZES + [0, 40], CPU, dtype=dtype, frozen_at=0)
    arr2[nt + 2].flags |= N.FROZEN
    assert _size(L, arr2, nt + 3, 20, 1) - _size(L, arr2, nt + 3, 19, 1) == 4 * total


# ---- codec.expand_mt_multi ----
def test_codec_expand_mt_multi_value_errors_come_before_any_device_access():
    from fate_llm.algo.fedkseed import codec
    t = torch.zeros(16)  # CPU tensors: any device access would raise something else
    specs = [codec.ParamSpec(t), codec.ParamSpec(torch.zeros(4), frozen=True)]
    ok = [[torch.zeros(16), None]]
    with pytest.raises(ValueError, match="shard"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], ok, shard=1, nshards=1)
    with pytest.raises(ValueError, match="coefs must be 1 x 2"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0, 3.0]], ok)
    with pytest.raises(ValueError, match="betas"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], ok, betas=[0.0, 1.0])
    with pytest.raises(ValueError, match="one tensor per spec"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], [[torch.zeros(16)]])
    with pytest.raises(ValueError, match="not frozen and has no tensor"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], [[None, None]])
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], [[torch.zeros(16, dtype=torch.float64), None]])
    with pytest.raises(ValueError, match="16 elements are needed"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], [[torch.zeros(15), None]])
    with pytest.raises(ValueError, match="not contiguous"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], [[torch.zeros(32)[::2], None]])
    o = torch.zeros(16)
    with pytest.raises(ValueError, match="same data_ptr"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0], [1.0, 2.0]], [[o, None], [o, None]])
    with pytest.raises(ValueError, match="staging_bytes"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], ok, staging_bytes=-1)
    # a valid call on CPU tensors reaches the device check: there is no CPU path
    with pytest.raises(ValueError, match="HIP device"):
        codec.expand_mt_multi(specs, [1, 2], [[1.0, 2.0]], ok)
    assert "stream_mode" not in codec.expand_mt_multi.__code__.co_varnames  # the stream is always torch_cpu


def test_seed_expansion_on_stream_refuses_cpu_parameters_without_touching_a_gpu():
    from fate_llm.algo.fedkseed import zo_utils
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="HIP device"):  # CPU parameters resolve to torch_cpu: no CPU path
        zo_utils.seed_expansion_on_stream_([{"params": [p]}], [1], [1.0])
    assert p.grad is None  # refused before the default output was created
    with pytest.raises(ValueError, match="HIP device"):
        zo_utils.seed_expansions_on_stream_([{"params": [p]}], [1], [[1.0]], [[torch.zeros(8)]], stream_mode="torch_cpu")
    # the torch_rocm-only functions keep refusing the stream, and name the routed call's target
    with pytest.raises(NotImplementedError, match="expand_mt_multi"):
        zo_utils.seed_expansion_([{"params": [p]}], [1], [1.0], outputs=[torch.zeros(8)])
    assert zo_utils.seed_expansions_on_stream_([], [1], [], []) == []
