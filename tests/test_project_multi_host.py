"""Host-side checks of fks_project_multi's C ABI and of codec.project_multi (no device
needed): every argument error is raised from the arguments alone, before any device work,
with a message; the trivial calls succeed; the workspace grows with the vector count up to the
per-pass cap and with the table; codec.project_multi raises its ValueErrors and refuses the
torch_cpu stream before it touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

EINVAL, ENOTSUP = 22, 95
FAKE = 0x7F0000001000  # a plausible, 4 KiB-aligned device address that is never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [4096, 0, 70_000, 5]  # the second is empty, the last frozen
FROZEN_AT = 3


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
        arr[i].flags = flags | (N.FROZEN if i == FROZEN_AT else 0)
        at += 4 * n + 4096 - (4 * n) % 4096
    return arr


def _vecs(N, sizes, nvec, dtype=1):
    """nvec x nt entries; those of the empty and of the frozen tensor stay NULL"""
    v = (N.FksVec * max(1, nvec * len(sizes)))()
    at = FAKE + (1 << 36)
    for m in range(nvec):
        for i, n in enumerate(sizes):
            if n and i != FROZEN_AT:
                v[m * len(sizes) + i].data = at
                v[m * len(sizes) + i].dtype = dtype
            at += 4 * n + 4096 - (4 * n) % 4096
    return v


def _call(L, arr, nt, vecs, nvec=2, k=2, shard=0, nshards=1, out=FAKE + (1 << 31), ws=FAKE + (1 << 32),
          ws_bytes=1 << 30, seeds=True):
    s = np.array([1, 2, 3][:max(k, 1)], dtype=np.uint64)
    return L.fks_project_multi(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None, k,
                               ctypes.addressof(vecs) if vecs is not None else None, nvec, shard, nshards, out, ws,
                               ws_bytes, None)


def _err(L):
    return L.fks_last_error().decode()


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    with open(os.path.join(ROOT, "include", "fks.h")) as f:
        hdr = f.read()
    for name in ("fks_project_multi", "fks_project_multi_workspace_size"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert re.search(r"typedef struct fks_vec\s*\{", hdr)
    assert ctypes.sizeof(N.FksVec) == 16
    assert L.fks_abi_version() == 1  # additive


@pytest.mark.parametrize("what,kw", [
    ("negative nvec", dict(nvec=-1)),
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
def test_einval_from_the_scalar_arguments(what, kw):
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2), **kw) == -EINVAL, what
    assert _err(L), what


def test_einval_from_the_vector_list():
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, nt, None) == -EINVAL and "vector" in _err(L)  # NULL vecs, nvec > 0, nt > 0
    for dt in (3, -1):  # a dtype outside the three
        v = _vecs(N, SIZES, 2)
        v[nt + 2].dtype = dt
        assert _call(L, arr, nt, v) == -EINVAL and "dtype" in _err(L)
    v = _vecs(N, SIZES, 2)
    v[nt + 0].data = None  # a live tensor's entry of the second vector
    assert _call(L, arr, nt, v) == -EINVAL and "vector 1, tensor 0" in _err(L)
    for dtype, off in ((0, 2), (0, 1), (1, 1), (2, 1)):  # f32 at 2 bytes, 2-byte types at an odd address
        v = _vecs(N, SIZES, 2, dtype=dtype)
        v[2].data += off
        assert _call(L, arr, nt, v) == -EINVAL and "misaligned" in _err(L), (dtype, off)
    # aligned to the element size only is enough: the error that remains is the workspace's
    for dtype, off in ((0, 4), (1, 2), (2, 2)):
        v = _vecs(N, SIZES, 2, dtype=dtype)
        v[2].data += off
        assert _call(L, arr, nt, v, ws_bytes=64) == -EINVAL and "workspace" in _err(L), (dtype, off)
    # the entries of the empty and of the frozen tensor are ignored, whatever they hold
    v = _vecs(N, SIZES, 2)
    for m in range(2):
        v[m * nt + 1].dtype = 77
        v[m * nt + FROZEN_AT].dtype = -5
        v[m * nt + FROZEN_AT].data = 3
    assert _call(L, arr, nt, v, ws_bytes=64) == -EINVAL and "workspace" in _err(L)


@pytest.mark.parametrize("flags", [0, 16])  # the CPU generator's stream, and its FKS_LIBM flavour
def test_refuses_the_cpu_stream(flags):
    N, L = _lib()
    assert flags in (0, N.LIBM)
    arr = _tensors(N, SIZES, flags, dtype=0)
    assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2)) == -ENOTSUP
    assert "fks_project" in _err(L) and "torch_cpu" in _err(L) and "FKS_STREAM_ROCM" in _err(L)
    if flags:
        assert "FKS_LIBM" in _err(L)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_project_multi_workspace_size(ctypes.addressof(arr), len(SIZES), 4, 2, ctypes.byref(nbytes)) == -ENOTSUP
    assert "torch_cpu" in _err(L)


def test_trivial_calls_succeed():
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    v = _vecs(N, SIZES, 2)
    assert _call(L, arr, nt, v, k=0, out=None, ws=None, ws_bytes=0) == 0, _err(L)  # no seeds
    assert _call(L, arr, nt, None, nvec=0, out=None, ws=None, ws_bytes=0) == 0, _err(L)  # no vectors
    assert _call(L, arr, 0, None, out=None, ws=None, ws_bytes=0, k=0) == 0, _err(L)  # no tensors, no seeds
    assert _call(L, arr, 0, None, nvec=0, k=0, out=None, ws=None, ws_bytes=0) == 0, _err(L)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_project_multi_workspace_size(ctypes.addressof(arr), 0, 4, 3, ctypes.byref(nbytes)) == 0
    assert L.fks_project_multi_workspace_size(ctypes.addressof(arr), nt, 0, 0, ctypes.byref(nbytes)) == 0


def test_workspace_size():
    N, L = _lib()
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001]

    def size(nt, nvec, k=33):
        arr = _tensors(N, sizes[:nt], N.STREAM_ROCM)
        nbytes = ctypes.c_size_t(0)
        assert L.fks_project_multi_workspace_size(ctypes.addressof(arr), nt, k, nvec, ctypes.byref(nbytes)) == 0, _err(L)
        return nbytes.value

    single = ctypes.c_size_t(0)
    arr = _tensors(N, sizes, N.STREAM_ROCM)
    assert L.fks_project_workspace_size(ctypes.addressof(arr), len(sizes), 33, ctypes.byref(single)) == 0
    by_nvec = [size(len(sizes), m) for m in range(1, 10)]
    assert all(b >= a for a, b in zip(by_nvec, by_nvec[1:])) and by_nvec[-1] > by_nvec[4]
    # the vector table (16 bytes per vector and tensor, rounded to 256) grows with every vector,
    # the partials with the first four only (the vectors of one pass)
    assert by_nvec[0] >= single.value and by_nvec[3] >= 4 * single.value
    assert max(b - a for a, b in zip(by_nvec[4:], by_nvec[5:])) <= 256 < by_nvec[3] - by_nvec[2]
    by_nt = [size(nt, 3) for nt in range(1, len(sizes) + 1)]
    assert all(b >= a for a, b in zip(by_nt, by_nt[1:])) and by_nt[0] < by_nt[-1]
    small = ctypes.c_size_t(0)
    assert L.fks_project_multi_workspace_size(ctypes.addressof(arr), 1, 1, 1, None) == -EINVAL
    assert L.fks_project_multi_workspace_size(ctypes.addressof(arr), 1, -1, 1, ctypes.byref(small)) == -EINVAL
    assert L.fks_project_multi_workspace_size(ctypes.addressof(arr), 1, 1, -1, ctypes.byref(small)) == -EINVAL


def test_codec_project_multi_refuses_torch_cpu_before_touching_a_device():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]  # CPU tensors: any device access would raise something else
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        codec.project_multi(specs, [1, 2], [[torch.zeros(16)]], stream_mode="torch_cpu")
    with pytest.raises(NotImplementedError, match="torch_cpu"):  # "auto" on CPU tensors resolves to torch_cpu
        codec.project_multi(specs, [1, 2], [[torch.zeros(16)]], stream_mode="auto")


@pytest.mark.parametrize("what,vectors", [
    ("None for a spec that is not frozen", lambda: [[torch.zeros(16), None, None]]),
    ("too few entries", lambda: [[torch.zeros(16), torch.zeros(8)]]),
    ("wrong element count", lambda: [[torch.zeros(16), torch.zeros(9), None]]),
    ("wrong element count in the second vector",
     lambda: [[torch.zeros(16), torch.zeros(8), None], [torch.zeros(15), torch.zeros(8), None]]),
    ("non-float dtype", lambda: [[torch.zeros(16), torch.zeros(8, dtype=torch.int32), None]]),
    ("wrong device", lambda: [[torch.zeros(16), torch.zeros(8, device="meta"), None]]),
])
def test_codec_project_multi_value_errors(what, vectors):
    """Raised from the arguments, before the spec list reaches a device (CPU specs would
    raise the codec's "no CPU path" error there, with another message)."""
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16)), codec.ParamSpec(torch.zeros(8)),
             codec.ParamSpec(torch.zeros(4), frozen=True)]
    with pytest.raises(ValueError, match="vector"):
        codec.project_multi(specs, [1, 2], vectors(), stream_mode="torch_rocm")
    with pytest.raises(ValueError, match="shard"):
        codec.project_multi(specs, [1], [[torch.zeros(16), torch.zeros(8), None]], stream_mode="torch_rocm", shard=2,
                            nshards=2)


def test_zo_utils_exports():
    from fate_llm.algo.fedkseed import codec, zo_utils
    assert callable(zo_utils.seed_projections_multi) and callable(zo_utils.fit_seed_scalars_multi)
    for f, g in ((zo_utils.seed_projections, "seed_projections_multi"),
                 (zo_utils.fit_seed_scalars, "fit_seed_scalars_multi"), (codec.project, "project_multi")):
        assert g in f.__doc__  # the staged forms point to the in-place ones
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="grad"):
        zo_utils.seed_projections_multi([{"params": [p]}], [1], stream_mode="torch_rocm")
    with pytest.raises(ValueError, match="one vector per parameter"):
        zo_utils.seed_projections_multi([{"params": [p]}], [1], [[]], stream_mode="torch_rocm")
