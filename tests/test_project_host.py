"""Host-side checks of the seed-basis projection's C ABI and Python entry point (no device
needed): every argument error of fks_project is raised from the arguments alone, before any
device work, with a message; the workspace size is positive and monotone in the tensor list;
codec.project refuses the torch_cpu stream before it touches a device."""
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
    return L.fks_project(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None, k, vec, shard, nshards, out, ws,
                         ws_bytes, None)


def _err(L):
    return L.fks_last_error().decode()


def test_project_symbols_and_abi():
    N, L = _lib()
    assert "fks_project" in N.EXPORTED and "fks_project_workspace_size" in N.EXPORTED
    assert L.fks_abi_version() == 1


@pytest.mark.parametrize("what,kw", [
    ("null vec", dict(vec=None)),
    ("misaligned vec", dict(vec=FAKE + (1 << 30) + 4)),
    ("null out", dict(out=None)),
    ("misaligned out", dict(out=FAKE + (1 << 31) + 4)),
    ("shard past the end", dict(shard=2, nshards=2)),
    ("negative shard", dict(shard=-1, nshards=2)),
    ("no shards", dict(shard=0, nshards=0)),
    ("null workspace", dict(ws=None)),
    ("workspace too small", dict(ws_bytes=64)),
    ("null seeds", dict(seeds=False)),
    ("negative k", dict(k=-1)),
])
def test_project_einval(what, kw):
    N, L = _lib()
    arr = _tensors(N, [4096, 0, 70_000], N.STREAM_ROCM)
    assert _project(L, arr, 3, **kw) == -EINVAL, what
    assert _err(L), what


@pytest.mark.parametrize("flags", [0, 16])  # the CPU generator's stream, and its FKS_LIBM flavour
def test_project_refuses_the_cpu_stream(flags):
    N, L = _lib()
    assert flags in (0, N.LIBM)
    arr = _tensors(N, [4096, 70_000], flags, dtype=0)
    assert _project(L, arr, 2) == -ENOTSUP
    assert "torch_cpu" in _err(L) and "FKS_STREAM_ROCM" in _err(L)
    if flags:
        assert "FKS_LIBM" in _err(L)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_project_workspace_size(ctypes.addressof(arr), 2, 4, ctypes.byref(nbytes)) == -ENOTSUP
    assert "torch_cpu" in _err(L)


def test_project_trivial_calls_succeed():
    N, L = _lib()
    arr = _tensors(N, [4096], N.STREAM_ROCM)
    assert _project(L, arr, 1, k=0, vec=None, out=None, ws=None, ws_bytes=0) == 0  # no seeds: nothing to do
    assert _project(L, arr, 0, k=0, vec=None, out=None, ws=None, ws_bytes=0) == 0  # no tensors either
    nbytes = ctypes.c_size_t(0)
    assert L.fks_project_workspace_size(ctypes.addressof(arr), 0, 4, ctypes.byref(nbytes)) == 0


def test_project_workspace_size_positive_and_monotone():
    N, L = _lib()
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001, 40_000_000]
    prev = 0
    for nt in range(1, len(sizes) + 1):
        arr = _tensors(N, sizes[:nt], N.STREAM_ROCM)
        nbytes = ctypes.c_size_t(0)
        assert L.fks_project_workspace_size(ctypes.addressof(arr), nt, 33, ctypes.byref(nbytes)) == 0, _err(L)
        assert nbytes.value > 0 and nbytes.value >= prev
        prev = nbytes.value
    small = ctypes.c_size_t(0)
    arr = _tensors(N, sizes[:1], N.STREAM_ROCM)
    assert L.fks_project_workspace_size(ctypes.addressof(arr), 1, 1, ctypes.byref(small)) == 0
    assert small.value < prev  # the size follows the list: it is no constant
    assert L.fks_project_workspace_size(ctypes.addressof(arr), 1, 1, None) == -EINVAL
    assert L.fks_project_workspace_size(ctypes.addressof(arr), 1, -1, ctypes.byref(small)) == -EINVAL


def test_codec_project_refuses_torch_cpu_before_touching_a_device():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]  # CPU tensors: any device access would raise something else
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        codec.project(specs, [1, 2], torch.zeros(16), stream_mode="torch_cpu")


def test_zo_utils_exports():
    from fate_llm.algo.fedkseed import zo_utils
    assert callable(zo_utils.seed_projections) and callable(zo_utils.fit_seed_scalars)
    assert "expectation" in zo_utils.fit_seed_scalars.__doc__
