"""Host-side checks of fks_expand_multi's C ABI, of its launch cuts and of codec.expand_multi
(no device needed; fake device addresses, nothing dereferenced): every argument error is raised
from the arguments alone, before any device work, with a message; the trivial calls succeed; the
workspace grows with k (the seed table) and with the output count; the launch cuts tile the
shard's items exactly, fall on row boundaries and hold at most W seed-elements or a single row;
codec.expand_multi raises its ValueErrors and refuses the torch_cpu stream before it touches a
device."""
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


def _outs(N, sizes, nvec, dtype=1):
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


def _call(L, arr, nt, outs, nvec=2, k=2, shard=0, nshards=1, ws=FAKE + (1 << 32), ws_bytes=1 << 30, seeds=True,
          coefs=True, betas=False):
    s = np.array([1, 2, 3][:max(k, 1)], dtype=np.uint64)
    c = np.ones(max(k, 1) * max(nvec, 1), dtype=np.float64)
    b = np.full(max(nvec, 1), 0.5, dtype=np.float64)
    return L.fks_expand_multi(ctypes.addressof(arr), nt, s.ctypes.data if seeds else None,
                              c.ctypes.data if coefs else None, k,
                              ctypes.addressof(outs) if outs is not None else None, b.ctypes.data if betas else None,
                              nvec, shard, nshards, ws, ws_bytes, None)


def _err(L):
    return L.fks_last_error().decode()


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    with open(os.path.join(ROOT, "include", "fks.h")) as f:
        hdr = f.read()
    for name in ("fks_expand_multi", "fks_expand_multi_workspace_size", "fks_expand_launch_cuts"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive


@pytest.mark.parametrize("what,kw", [
    ("negative nvec", dict(nvec=-1)),
    ("shard past the end", dict(shard=2, nshards=2)),
    ("negative shard", dict(shard=-1, nshards=2)),
    ("no shards", dict(shard=0, nshards=0)),
    ("null workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=FAKE + (1 << 32) + 4)),
    ("workspace too small", dict(ws_bytes=64)),
    ("workspace too small, with betas", dict(ws_bytes=64, betas=True)),
    ("null seeds", dict(seeds=False)),
    ("null coefs", dict(coefs=False)),
    ("negative k", dict(k=-1)),
])
def test_einval_from_the_scalar_arguments(what, kw):
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, len(SIZES), _outs(N, SIZES, 2), **kw) == -EINVAL, what
    assert _err(L), what


def test_einval_from_the_output_list():
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
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


@pytest.mark.parametrize("flags", [0, 16])  # the CPU generator's stream, and its FKS_LIBM flavour
def test_refuses_the_cpu_stream(flags):
    N, L = _lib()
    assert flags in (0, N.LIBM)
    arr = _tensors(N, SIZES, flags, dtype=0)
    assert _call(L, arr, len(SIZES), _outs(N, SIZES, 2)) == -ENOTSUP
    assert "fks_delta_accumulate" in _err(L) and "torch_cpu" in _err(L) and "FKS_STREAM_ROCM" in _err(L)
    assert ("FKS_LIBM" in _err(L)) == bool(flags)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_expand_multi_workspace_size(ctypes.addressof(arr), len(SIZES), 4, 2, ctypes.byref(nbytes)) == -ENOTSUP
    assert "fks_delta_accumulate" in _err(L)


def test_trivial_calls_succeed():
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, nt, None, nvec=0, ws=None, ws_bytes=0) == 0, _err(L)  # no outputs
    assert _call(L, arr, 0, None, ws=None, ws_bytes=0) == 0, _err(L)  # no tensors
    assert _call(L, arr, 0, None, nvec=0, k=0, ws=None, ws_bytes=0, seeds=False, coefs=False) == 0, _err(L)
    empty = _tensors(N, [0, 0], N.STREAM_ROCM, frozen_at=-1)  # an all-empty list: nothing to write
    assert _call(L, empty, 2, _outs(N, [0, 0], 2), ws=None, ws_bytes=0) == 0, _err(L)
    frozen = _tensors(N, [0, 0, 0, 5], N.STREAM_ROCM)  # ... and one whose only elements are frozen
    assert _call(L, frozen, 4, _outs(N, [0, 0, 0, 5], 2), ws=None, ws_bytes=0) == 0, _err(L)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_expand_multi_workspace_size(ctypes.addressof(arr), 0, 4, 3, ctypes.byref(nbytes)) == 0
    assert L.fks_expand_multi_workspace_size(ctypes.addressof(arr), nt, 0, 0, ctypes.byref(nbytes)) == 0


def test_workspace_size():
    N, L = _lib()
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001]

    def size(nt, nvec, k=33):
        arr = _tensors(N, sizes[:nt], N.STREAM_ROCM)
        nbytes = ctypes.c_size_t(0)
        assert L.fks_expand_multi_workspace_size(ctypes.addressof(arr), nt, k, nvec, ctypes.byref(nbytes)) == 0, _err(L)
        return nbytes.value

    nt = len(sizes)
    by_k = [size(nt, 1, k) for k in (0, 1, 33, 70, 4096)]  # the seed table: 8 bytes per seed + 4 per coefficient
    assert all(b >= a for a, b in zip(by_k, by_k[1:])) and by_k[0] < by_k[2] < by_k[4]
    assert by_k[4] - by_k[0] >= 12 * 4096
    by_nvec = [size(nt, m, 4096) for m in range(1, 10)]  # ... and 4 bytes per seed and output more
    assert all(b - a >= 4 * 4096 for a, b in zip(by_nvec, by_nvec[1:]))
    # one output's table entry per tensor piece: 16 bytes each, rounded to 256
    assert size(nt, 1, 0) >= 16 * (nt - 1) and size(nt, 9, 0) >= 9 * 16 * (nt - 1)
    # nothing of the model's size: the 7-tensor list's whole workspace at K = 4096, four outputs
    assert by_nvec[3] < 1 << 20
    arr = _tensors(N, sizes, N.STREAM_ROCM)
    small = ctypes.c_size_t(0)
    assert L.fks_expand_multi_workspace_size(ctypes.addressof(arr), 1, 1, 1, None) == -EINVAL
    assert L.fks_expand_multi_workspace_size(ctypes.addressof(arr), 1, -1, 1, ctypes.byref(small)) == -EINVAL
    assert L.fks_expand_multi_workspace_size(ctypes.addressof(arr), 1, 1, -1, ctypes.byref(small)) == -EINVAL


# ---- the launch cuts, as arithmetic (fks_expand_launch_cuts: the pure function of fks_phx.cpp) ----
CUT_SIZES = [4096, 1000, 3, 700_001, 7, 65536, 2_000_000]
CUT_FROZEN = 2


def _rows(sizes, frozen, cap):
    """(items, row boundaries) of the list under torch's launch policy with a grid cap: a tensor of n
    elements has stride S = 256 min(ceil(n / 256), cap) and ceil(n / 4 S) rows of S items"""
    at, rows = 0, {0}
    for i, n in enumerate(sizes):
        if n == 0 or i == frozen:
            continue
        S = 256 * min((n + 255) // 256, cap)
        for _ in range((n - 1) // (4 * S) + 1):
            at += S
            rows.add(at)
    return at, rows


def _cuts(N, L, sizes, k, work, cap, shard=0, nshards=1):
    arr = _tensors(N, sizes, N.STREAM_ROCM, frozen_at=CUT_FROZEN)
    n = ctypes.c_int32(0)
    buf = (ctypes.c_int64 * 4096)()
    assert L.fks_expand_launch_cuts(ctypes.addressof(arr), len(sizes), k, shard, nshards, work, cap, buf, 4096,
                                    ctypes.byref(n)) == 0, _err(L)
    assert n.value <= 4096
    return list(buf[:n.value])


@pytest.mark.parametrize("cap", [2048, 8, 1])
@pytest.mark.parametrize("k", [0, 1, 33, 4096])
@pytest.mark.parametrize("work", [1, 4 * 256 * 33, 1 << 20, 1 << 24, 1 << 37])
def test_launch_cuts_tile_the_items_at_row_boundaries_within_the_work_bound(cap, k, work):
    N, L = _lib()
    items, rows = _rows(CUT_SIZES, CUT_FROZEN, cap)
    c = _cuts(N, L, CUT_SIZES, k, work, cap)
    assert c[0] == 0 and c[-1] == items  # the cuts tile the items exactly ...
    assert all(a < b for a, b in zip(c, c[1:]))
    assert set(c) <= rows  # ... each at a row boundary
    srows = sorted(rows)
    for a, b in zip(c, c[1:]):  # at most `work` seed-elements, or a single row
        assert 4 * (b - a) * max(k, 1) <= work or srows[srows.index(a) + 1] == b, (a, b)
    # greedy: no launch but the last could have taken the next row as well
    for a, b in zip(c[:-1], c[1:-1]):
        nxt = srows[srows.index(b) + 1]
        assert 4 * (nxt - a) * max(k, 1) > work, (a, b, nxt)


def test_launch_cuts_of_shards_and_the_default_bound():
    N, L = _lib()
    items, rows = _rows(CUT_SIZES, CUT_FROZEN, 8)
    ends = []
    for sh in range(3):
        c = _cuts(N, L, CUT_SIZES, 33, 1 << 22, 8, shard=sh, nshards=3)
        assert set(c) <= rows and len(c) >= 3
        ends.append((c[0], c[-1]))
    assert ends[0][0] == 0 and ends[2][1] == items and ends[0][1] == ends[1][0] and ends[1][1] == ends[2][0]
    # the default bound, 2^37 seed-elements: this list at K = 4096 is one launch; FKS_EXPAND_WORK overrides it per call
    assert len(_cuts(N, L, CUT_SIZES, 4096, 0, 8)) == 2
    os.environ["FKS_EXPAND_WORK"] = str(1 << 22)
    try:
        assert _cuts(N, L, CUT_SIZES, 33, 0, 8) == _cuts(N, L, CUT_SIZES, 33, 1 << 22, 8)
    finally:
        del os.environ["FKS_EXPAND_WORK"]
    # nothing to do: no boundaries at all
    assert _cuts(N, L, [0, 0], 33, 1 << 22, 8) == []


# ---- codec.expand_multi ----
def test_codec_expand_multi_refuses_torch_cpu_before_touching_a_device():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]  # CPU tensors: any device access would raise something else
    with pytest.raises(NotImplementedError, match="delta_accumulate"):
        codec.expand_multi(specs, [1, 2], [[1.0, 2.0]], [[torch.zeros(16)]], stream_mode="torch_cpu")
    with pytest.raises(NotImplementedError, match="delta_accumulate"):  # "auto" on CPU tensors resolves to torch_cpu
        codec.expand_multi(specs, [1, 2], [[1.0, 2.0]], [[torch.zeros(16)]], stream_mode="auto")


def _same_ptr_twice():
    t = torch.zeros(16)
    return [[t, torch.zeros(8), None], [t, torch.zeros(8), None]]


@pytest.mark.parametrize("what,outputs,coefs", [
    ("None for a spec that is not frozen", lambda: [[torch.zeros(16), None, None]], [[1.0, 2.0]]),
    ("too few entries", lambda: [[torch.zeros(16), torch.zeros(8)]], [[1.0, 2.0]]),
    ("wrong element count", lambda: [[torch.zeros(16), torch.zeros(9), None]], [[1.0, 2.0]]),
    ("wrong dtype", lambda: [[torch.zeros(16), torch.zeros(8, dtype=torch.float64), None]], [[1.0, 2.0]]),
    ("integer dtype", lambda: [[torch.zeros(16), torch.zeros(8, dtype=torch.int32), None]], [[1.0, 2.0]]),
    ("wrong device", lambda: [[torch.zeros(16), torch.zeros(8, device="meta"), None]], [[1.0, 2.0]]),
    ("not contiguous", lambda: [[torch.zeros(32)[::2], torch.zeros(8), None]], [[1.0, 2.0]]),
    ("the same data_ptr twice", _same_ptr_twice, [[1.0, 2.0], [3.0, 4.0]]),
    ("coefs K x M instead of M x K", lambda: [[torch.zeros(16), torch.zeros(8), None]], [[1.0], [2.0]]),
    ("coefs of another length", lambda: [[torch.zeros(16), torch.zeros(8), None]], [1.0, 2.0, 3.0]),
    ("one coefficient row for two outputs",
     lambda: [[torch.zeros(16), torch.zeros(8), None], [torch.zeros(16), torch.zeros(8), None]], [[1.0, 2.0]]),
])
def test_codec_expand_multi_value_errors(what, outputs, coefs):
    """Raised from the arguments, before the spec list reaches a device (CPU specs would raise the
    codec's "no CPU path" error there, with another message)."""
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16)), codec.ParamSpec(torch.zeros(8)),
             codec.ParamSpec(torch.zeros(4), frozen=True)]
    with pytest.raises(ValueError, match="output|coefs"):
        codec.expand_multi(specs, [1, 2], coefs, outputs(), stream_mode="torch_rocm")


def test_codec_expand_multi_shard_and_beta_errors():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]
    with pytest.raises(ValueError, match="shard"):
        codec.expand_multi(specs, [1], [[1.0]], [[torch.zeros(16)]], stream_mode="torch_rocm", shard=2, nshards=2)
    with pytest.raises(ValueError, match="betas"):
        codec.expand_multi(specs, [1], [[1.0]], [[torch.zeros(16)]], betas=[0.0, 1.0], stream_mode="torch_rocm")


def test_zo_utils_exports():
    from fate_llm.algo.fedkseed import zo_utils
    assert callable(zo_utils.seed_expansion_) and callable(zo_utils.seed_expansions_)
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="one output per parameter"):
        zo_utils.seed_expansion_([{"params": [p]}], [1], [1.0], outputs=[], stream_mode="torch_rocm")
    with pytest.raises(ValueError, match="one scalar list per output list"):
        zo_utils.seed_expansions_([{"params": [p]}], [1], [[1.0], [2.0]], [[torch.zeros(8)]], stream_mode="torch_rocm")
    with pytest.raises(NotImplementedError, match="delta_accumulate"):  # CPU parameters resolve to torch_cpu
        zo_utils.seed_expansion_([{"params": [p]}], [1], [1.0], outputs=[torch.zeros(8)])
