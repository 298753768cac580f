"""Host-side checks of fks_project_mt_multi's C ABI, of codec.project_mt_multi and of the routed
zo_utils forms (no device needed): every argument error is raised from the arguments alone,
before any device work, with a message, on the CPU generator's stream and on its FKS_LIBM
flavour; a list of the torch_rocm stream is refused with the name of the call for that stream;
the trivial calls succeed; the workspace size is positive, monotone in the tensor list and in the
vector count, and no constant; codec.project_mt_multi raises its ValueErrors before the library
is loaded and has no CPU path."""
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


def _tensors(N, sizes, flags, dtype=1, frozen_at=FROZEN_AT):
    arr = (N.FksTensor * max(1, len(sizes)))()
    at = FAKE
    for i, n in enumerate(sizes):
        arr[i].data = at if n else None
        arr[i].numel = n
        arr[i].dtype = dtype
        arr[i].flags = flags | (N.FROZEN if i == frozen_at else 0)
        at += 4 * n + 4096 - (4 * n) % 4096
    return arr


def _vecs(N, sizes, nvec, dtype=1, frozen_at=FROZEN_AT):
    """nvec x nt entries; those of the empty and of the frozen tensor stay NULL"""
    v = (N.FksVec * max(1, nvec * len(sizes)))()
    at = FAKE + (1 << 36)
    for m in range(nvec):
        for i, n in enumerate(sizes):
            if n and i != frozen_at:
                v[m * len(sizes) + i].data = at
                v[m * len(sizes) + i].dtype = dtype
            at += 4 * n + 4096 - (4 * n) % 4096
    return v


def _call(L, arr, nt, vecs, nvec=2, k=2, shard=0, nshards=1, out=FAKE + (1 << 31), ws=FAKE + (1 << 32),
          ws_bytes=1 << 30, seeds=True):
    s = np.array([1, 2, 3][:max(k, 1)], dtype=np.uint64)
    return L.fks_project_mt_multi(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None, k,
                                  ctypes.addressof(vecs) if vecs is not None else None, nvec, shard, nshards, out, ws,
                                  ws_bytes, None)


def _size(L, arr, nt, k, nvec):
    nbytes = ctypes.c_size_t(0)
    rc = L.fks_project_mt_multi_workspace_size(ctypes.addressof(arr), nt, k, nvec, ctypes.byref(nbytes))
    return rc, nbytes.value


def _err(L):
    return L.fks_last_error().decode()


FLAGS = [0, 16]  # the CPU generator's stream, and its FKS_LIBM flavour


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    with open(os.path.join(ROOT, "include", "fks.h")) as f:
        hdr = f.read()
    for name in ("fks_project_mt_multi", "fks_project_mt_multi_workspace_size"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive
    # the Python constant mirrors the library's vectors per pass
    from fate_llm.algo.fedkseed import codec
    with open(os.path.join(ROOT, "fate-llm_amd", "csrc", "fks_project_mt.h")) as f:
        cap = int(re.search(r"^#define FKS_PMT_MAX_VEC (\d+)$", f.read(), re.M).group(1))
    assert 2 <= cap <= 4 and codec.PROJECT_MT_PASS_VECTORS == cap


@pytest.mark.parametrize("flags", FLAGS)
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
def test_einval_from_the_scalar_arguments(what, kw, flags):
    N, L = _lib()
    assert flags in (0, N.LIBM)
    arr = _tensors(N, SIZES, flags)
    assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2), **kw) == -EINVAL, what
    assert _err(L), what


@pytest.mark.parametrize("flags", FLAGS)
def test_einval_from_the_vector_list(flags):
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, flags)
    assert _call(L, arr, nt, None) == -EINVAL and "vector" in _err(L)  # NULL vecs, nvec > 0, nt > 0
    for dt in (3, -1):  # a dtype outside the three
        v = _vecs(N, SIZES, 2)
        v[nt + 2].dtype = dt
        assert _call(L, arr, nt, v) == -EINVAL and "dtype" in _err(L)
    v = _vecs(N, SIZES, 2)
    v[nt + 0].data = None  # a live tensor's entry of the second vector
    assert _call(L, arr, nt, v) == -EINVAL and "vector 1, tensor 0" in _err(L)
    for dtype, off in ((1, 1), (2, 1), (0, 2), (0, 1)):  # 2-byte types at an odd address, f32 at addr + 2
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


@pytest.mark.parametrize("flags", FLAGS)
def test_workspace_one_byte_short(flags):
    """the size the size call reports is what the call asks for"""
    N, L = _lib()
    arr = _tensors(N, SIZES, flags)
    rc, nbytes = _size(L, arr, len(SIZES), 2, 2)
    assert rc == 0 and nbytes > 0, _err(L)
    assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2), ws_bytes=nbytes - 1) == -EINVAL
    assert "workspace" in _err(L) and str(nbytes) in _err(L)


def test_refuses_the_rocm_stream():
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM, dtype=0)
    assert _call(L, arr, len(SIZES), _vecs(N, SIZES, 2)) == -ENOTSUP
    assert "fks_project_multi" in _err(L) and "FKS_STREAM_ROCM" in _err(L)
    rc, _ = _size(L, arr, len(SIZES), 4, 2)
    assert rc == -ENOTSUP and "fks_project_multi" in _err(L)


@pytest.mark.parametrize("flags", FLAGS)
def test_trivial_calls_succeed(flags):
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, flags)
    v = _vecs(N, SIZES, 2)
    assert _call(L, arr, nt, v, k=0, out=None, ws=None, ws_bytes=0) == 0, _err(L)  # no seeds
    assert _call(L, arr, nt, None, nvec=0, out=None, ws=None, ws_bytes=0) == 0, _err(L)  # no vectors
    assert _call(L, arr, 0, None, out=None, ws=None, ws_bytes=0, k=0) == 0, _err(L)  # no tensors, no seeds
    assert _call(L, arr, 0, None, nvec=0, k=0, out=None, ws=None, ws_bytes=0) == 0, _err(L)
    empty = _tensors(N, [0, 0], flags, frozen_at=-1)
    assert _call(L, empty, 2, _vecs(N, [0, 0], 2), k=0, out=None, ws=None, ws_bytes=0) == 0, _err(L)  # all empty
    assert _size(L, arr, 0, 4, 3)[0] == 0
    assert _size(L, arr, nt, 0, 0)[0] == 0
    assert _size(L, empty, 2, 4, 2)[0] == 0


def test_workspace_size_positive_monotone_and_no_constant():
    N, L = _lib()
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001, 40_000_000]
    for dtype in (0, 1, 2):
        prev = 0
        for nt in range(1, len(sizes) + 1):  # as the list grows
            arr = _tensors(N, sizes[:nt], 0, dtype=dtype, frozen_at=-1)
            rc, nbytes = _size(L, arr, nt, 20, 3)
            assert rc == 0 and nbytes > 0 and nbytes >= prev, _err(L)
            prev = nbytes
        rc, small = _size(L, _tensors(N, sizes[:1], 0, dtype=dtype, frozen_at=-1), 1, 20, 3)
        assert rc == 0 and small < prev  # the size follows the list: it is no constant
        arr = _tensors(N, sizes, 0, dtype=dtype, frozen_at=-1)
        by_nvec = [_size(L, arr, len(sizes), 20, m)[1] for m in range(1, 10)]  # as nvec grows
        assert all(b >= a for a, b in zip(by_nvec, by_nvec[1:])) and by_nvec[-1] > by_nvec[0]
        single = ctypes.c_size_t(0)
        assert L.fks_project_mt_workspace_size(ctypes.addressof(arr), len(sizes), 20, ctypes.byref(single)) == 0
        assert by_nvec[0] >= single.value  # the one-vector layout behind the table
    arr = _tensors(N, sizes[:1], 0)
    small = ctypes.c_size_t(0)
    assert L.fks_project_mt_multi_workspace_size(ctypes.addressof(arr), 1, 1, 1, None) == -EINVAL
    assert L.fks_project_mt_multi_workspace_size(ctypes.addressof(arr), 1, -1, 1, ctypes.byref(small)) == -EINVAL
    assert L.fks_project_mt_multi_workspace_size(ctypes.addressof(arr), 1, 1, -1, ctypes.byref(small)) == -EINVAL


def test_codec_project_mt_multi_has_no_cpu_path():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]
    with pytest.raises(ValueError, match="no CPU path"):
        codec.project_mt_multi(specs, [1, 2], [[torch.zeros(16)]])


@pytest.mark.parametrize("what,vectors", [
    ("None for a spec that is not frozen", lambda: [[torch.zeros(16), None, None]]),
    ("too few entries", lambda: [[torch.zeros(16), torch.zeros(8)]]),
    ("wrong element count", lambda: [[torch.zeros(16), torch.zeros(9), None]]),
    ("wrong element count in the second vector",
     lambda: [[torch.zeros(16), torch.zeros(8), None], [torch.zeros(15), torch.zeros(8), None]]),
    ("integer tensor", lambda: [[torch.zeros(16), torch.zeros(8, dtype=torch.int32), None]]),
])
def test_codec_project_mt_multi_value_errors(what, vectors, monkeypatch):
    """Raised from the arguments, before the library is loaded (CPU specs would raise the codec's
    "no CPU path" error after these checks, with another message)."""
    from fate_llm.algo.fedkseed import _native, codec

    def no_load():
        raise AssertionError("the library was loaded before the argument checks")

    monkeypatch.setattr(_native, "load", no_load)
    specs = [codec.ParamSpec(torch.zeros(16)), codec.ParamSpec(torch.zeros(8)),
             codec.ParamSpec(torch.zeros(4), frozen=True)]
    with pytest.raises(ValueError, match="vector"):
        codec.project_mt_multi(specs, [1, 2], vectors())
    with pytest.raises(ValueError, match="shard"):
        codec.project_mt_multi(specs, [1], [[torch.zeros(16), torch.zeros(8), None]], shard=2, nshards=2)


def test_zo_utils_routed_forms():
    from fate_llm.algo.fedkseed import codec, zo_utils
    for f in (zo_utils.seed_projections_in_place, zo_utils.fit_seed_scalars_in_place):
        assert "project_multi" in f.__doc__ and "project_mt_multi" in f.__doc__  # both codec calls
    for f, g in ((zo_utils.seed_projections_multi, "seed_projections_in_place"),
                 (zo_utils.fit_seed_scalars_multi, "fit_seed_scalars_in_place"),
                 (codec.project_multi, "project_mt_multi")):
        assert g in f.__doc__  # the torch_rocm-only forms point to the routed ones
    with pytest.raises(NotImplementedError, match="torch_cpu") as e:
        codec.project_multi([codec.ParamSpec(torch.zeros(16))], [1], [[torch.zeros(16)]], stream_mode="torch_cpu")
    assert "project_mt_multi" in str(e.value)
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="grad"):
        zo_utils.seed_projections_in_place([{"params": [p]}], [1], stream_mode="torch_cpu")
    with pytest.raises(ValueError, match="one vector per parameter"):
        zo_utils.seed_projections_in_place([{"params": [p]}], [1], [[]], stream_mode="torch_cpu")
