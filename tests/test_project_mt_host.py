"""Host-side checks of the MT19937-stream projection's C ABI and Python entry point (no device
needed): every argument error of fks_project_mt is raised from the arguments alone, before any
device work, with a message; the workspace size is positive, monotone in the tensor list and no
constant; codec.project_mt has no CPU path."""
import ctypes

import numpy as np
import pytest
import torch

EINVAL, ENOTSUP = 22, 95
FAKE = 0x7F0000001000  # a plausible, 4 KiB-aligned device address that is never dereferenced


def _lib():
    from fate_llm.algo.fedkseed import _native
    return _native, _native.load()


def _tensors(N, sizes, flags, dtype=1):
    arr = (N.FksTensor * max(1, len(sizes)))()
    at = FAKE
    for i, n in enumerate(sizes):
        arr[i].data = at if n else None
        arr[i].numel = n
        arr[i].dtype = dtype
        arr[i].flags = flags
        at += 4 * n + 4096 - (4 * n) % 4096
    return arr


def _project(L, arr, nt, k=2, vec=FAKE + (1 << 30), shard=0, nshards=1, out=FAKE + (1 << 31), ws=FAKE + (1 << 32),
             ws_bytes=1 << 30, seeds=True):
    s = np.array([1, 2, 3][:max(k, 1)], dtype=np.uint64)
    return L.fks_project_mt(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None, k, vec, shard, nshards, out,
                            ws, ws_bytes, None)


def _err(L):
    return L.fks_last_error().decode()


def test_project_mt_symbols_and_abi():
    N, L = _lib()
    assert "fks_project_mt" in N.EXPORTED and "fks_project_mt_workspace_size" in N.EXPORTED
    assert L.fks_abi_version() == 1


@pytest.mark.parametrize("flags", [0, 16])  # the CPU generator's stream, and its FKS_LIBM flavour
@pytest.mark.parametrize("what,kw", [
    ("null vec", dict(vec=None)),
    ("misaligned vec", dict(vec=FAKE + (1 << 30) + 4)),
    ("null out", dict(out=None)),
    ("misaligned out", dict(out=FAKE + (1 << 31) + 4)),
    ("shard past the end", dict(shard=2, nshards=2)),
    ("negative shard", dict(shard=-1, nshards=2)),
    ("no shards", dict(shard=0, nshards=0)),
    ("null workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=FAKE + (1 << 32) + 4)),
    ("workspace too small", dict(ws_bytes=64)),
    ("null seeds", dict(seeds=False)),
    ("negative k", dict(k=-1)),
])
def test_project_mt_einval(what, kw, flags):
    N, L = _lib()
    assert flags in (0, N.LIBM)
    arr = _tensors(N, [4096, 0, 70_000, 5], flags)
    assert _project(L, arr, 4, **kw) == -EINVAL, what
    assert _err(L), what


def test_project_mt_workspace_one_byte_short():
    """the size the size call reports is what the call asks for"""
    N, L = _lib()
    arr = _tensors(N, [4096, 0, 70_000, 5], 0)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_project_mt_workspace_size(ctypes.addressof(arr), 4, 2, ctypes.byref(nbytes)) == 0, _err(L)
    assert _project(L, arr, 4, ws_bytes=nbytes.value - 1) == -EINVAL
    assert "workspace" in _err(L) and str(nbytes.value) in _err(L)


def test_project_mt_refuses_the_rocm_stream():
    N, L = _lib()
    arr = _tensors(N, [4096, 70_000], N.STREAM_ROCM, dtype=0)
    assert _project(L, arr, 2) == -ENOTSUP
    assert "fks_project " in _err(L) + " " and "FKS_STREAM_ROCM" in _err(L)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_project_mt_workspace_size(ctypes.addressof(arr), 2, 4, ctypes.byref(nbytes)) == -ENOTSUP
    assert "fks_project " in _err(L) + " "


def test_project_mt_trivial_calls_succeed():
    N, L = _lib()
    arr = _tensors(N, [4096], 0)
    assert _project(L, arr, 1, k=0, vec=None, out=None, ws=None, ws_bytes=0) == 0  # no seeds: nothing to do
    assert _project(L, arr, 0, k=0, vec=None, out=None, ws=None, ws_bytes=0) == 0  # no tensors either
    nbytes = ctypes.c_size_t(0)
    assert L.fks_project_mt_workspace_size(ctypes.addressof(arr), 0, 4, ctypes.byref(nbytes)) == 0
    empty = _tensors(N, [0, 0], 0)
    assert L.fks_project_mt_workspace_size(ctypes.addressof(empty), 2, 4, ctypes.byref(nbytes)) == 0
    assert _project(L, empty, 2, k=0, vec=None, out=None, ws=None, ws_bytes=0) == 0  # an all-empty list


def test_project_mt_workspace_size_positive_and_monotone():
    N, L = _lib()
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001, 40_000_000]
    for dtype in (0, 1, 2):
        prev = 0
        for nt in range(1, len(sizes) + 1):
            arr = _tensors(N, sizes[:nt], 0, dtype=dtype)
            nbytes = ctypes.c_size_t(0)
            assert L.fks_project_mt_workspace_size(ctypes.addressof(arr), nt, 20, ctypes.byref(nbytes)) == 0, _err(L)
            assert nbytes.value > 0 and nbytes.value >= prev
            prev = nbytes.value
        small = ctypes.c_size_t(0)
        arr = _tensors(N, sizes[:1], 0, dtype=dtype)
        assert L.fks_project_mt_workspace_size(ctypes.addressof(arr), 1, 1, ctypes.byref(small)) == 0
        assert small.value < prev  # the size follows the list: it is no constant
    assert L.fks_project_mt_workspace_size(ctypes.addressof(arr), 1, 1, None) == -EINVAL
    assert L.fks_project_mt_workspace_size(ctypes.addressof(arr), 1, -1, ctypes.byref(small)) == -EINVAL


def test_codec_project_mt_has_no_cpu_path():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]
    with pytest.raises(ValueError, match="no CPU path"):
        codec.project_mt(specs, [1, 2], torch.zeros(16))


def test_zo_utils_docstrings_name_both_streams():
    from fate_llm.algo.fedkseed import codec, zo_utils
    assert "project_mt" in zo_utils.seed_projections.__doc__ and "project_mt" in codec.project.__doc__
    assert "torch_cpu" in codec.project_mt.__doc__
