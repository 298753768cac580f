"""fks_gram_mt without a device: the header and the exports, every argument error with its message
over both flavours of the CPU generator's stream, the refusal of the torch_rocm stream, the trivial
calls, the workspace arithmetic, the pass tiling of fks_gram_mt_passes, and the Python layers'
checks that run before a device is touched.  tests/test_gram_host.py's scheme for the other stream."""
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
FLAGS = [0, 16]  # the CPU generator's stream, and its FKS_LIBM flavour


def _lib():
    from fate_llm.algo.fedkseed import _native
    return _native, _native.load()


def _tile():
    from fate_llm.algo.fedkseed import codec
    return codec.GRAM_MT_PASS_ROWS, codec.GRAM_MT_PASS_COLS


def _ks():
    NR, NC = _tile()
    return [0, 1, NR, NR + 1, NC, NC + 1, 37, 100]


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


def _call(L, arr, nt, kr=3, kc=2, rows=True, cols=True, shard=0, nshards=1, out=FAKE + (1 << 31),
          ws=FAKE + (1 << 32), ws_bytes=1 << 30):
    r = np.arange(1, max(kr, 1) + 1, dtype=np.uint64)
    c = np.arange(11, max(kc, 1) + 11, dtype=np.uint64)
    return L.fks_gram_mt(ctypes.addressof(arr), nt, r.ctypes.data if rows else None, kr,
                         c.ctypes.data if cols else None, kc, shard, nshards, out, ws, ws_bytes, None)


def _err(L):
    return L.fks_last_error().decode()


def _size(L, arr, nt, kr, kc):
    nbytes = ctypes.c_size_t(0)
    assert L.fks_gram_mt_workspace_size(ctypes.addressof(arr), nt, kr, kc, ctypes.byref(nbytes)) == 0, _err(L)
    return nbytes.value


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    with open(os.path.join(ROOT, "include", "fks.h")) as f:
        hdr = f.read()
    for name in ("fks_gram_mt", "fks_gram_mt_workspace_size", "fks_gram_mt_passes"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("what,kw", [
    ("null row seeds", dict(rows=False)),
    ("negative krows", dict(kr=-1)),
    ("negative kcols", dict(kc=-1)),
    ("null out", dict(out=None)),
    ("misaligned out", dict(out=FAKE + (1 << 31) + 4)),
    ("null out, symmetric", dict(cols=False, kc=0, out=None)),
    ("shard past the end", dict(shard=2, nshards=2)),
    ("negative shard", dict(shard=-1, nshards=2)),
    ("no shards", dict(shard=0, nshards=0)),
    ("kcols neither 0 nor krows without column seeds", dict(cols=False, kc=2)),
    ("null workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=FAKE + (1 << 32) + 4)),
    ("workspace too small", dict(ws_bytes=64)),
    ("workspace too small, symmetric", dict(cols=False, kc=3, ws_bytes=64)),
])
def test_einval_from_the_arguments(what, kw, flags):
    N, L = _lib()
    assert flags in (0, N.LIBM)
    arr = _tensors(N, SIZES, flags)
    assert _call(L, arr, len(SIZES), **kw) == -EINVAL, what
    assert _err(L), what


def test_refuses_the_rocm_stream():
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    for kw in (dict(), dict(cols=False, kc=0)):
        assert _call(L, arr, len(SIZES), **kw) == -ENOTSUP
        assert "fks_gram_mt" in _err(L) and "FKS_STREAM_ROCM" in _err(L)
        assert re.search(r"\bfks_gram\b(?!_)", _err(L)), "the message names fks_gram as that stream's call"
    nbytes = ctypes.c_size_t(0)
    assert L.fks_gram_mt_workspace_size(ctypes.addressof(arr), len(SIZES), 4, 4, ctypes.byref(nbytes)) == -ENOTSUP
    assert re.search(r"\bfks_gram\b(?!_)", _err(L))


@pytest.mark.parametrize("flags", FLAGS)
def test_trivial_calls_succeed(flags):
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, flags)
    none = dict(out=None, ws=None, ws_bytes=0)
    assert _call(L, arr, nt, kr=0, rows=False, **none) == 0, _err(L)             # no row seeds
    assert _call(L, arr, nt, kr=0, kc=0, rows=False, cols=False, **none) == 0, _err(L)  # symmetric, K = 0
    assert _call(L, arr, nt, kc=0, **none) == 0, _err(L)                         # column seeds given, none of them
    assert _call(L, arr, 0, kr=0, kc=0, **none) == 0, _err(L)                    # no tensors
    nbytes = ctypes.c_size_t(0)
    assert L.fks_gram_mt_workspace_size(ctypes.addressof(arr), 0, 4, 3, ctypes.byref(nbytes)) == 0
    assert L.fks_gram_mt_workspace_size(ctypes.addressof(arr), nt, 0, 0, ctypes.byref(nbytes)) == 0
    assert L.fks_gram_mt_workspace_size(ctypes.addressof(arr), nt, 1, 1, None) == -EINVAL
    assert L.fks_gram_mt_workspace_size(ctypes.addressof(arr), nt, -1, 1, ctypes.byref(nbytes)) == -EINVAL
    assert L.fks_gram_mt_workspace_size(ctypes.addressof(arr), nt, 1, -1, ctypes.byref(nbytes)) == -EINVAL


def test_workspace_follows_the_list_and_not_the_seed_counts():
    N, L = _lib()
    NR, NC = _tile()
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001]

    def size(nt, kr, kc):
        return _size(L, _tensors(N, sizes[:nt], 0, frozen_at=-1), nt, kr, kc)

    by_nt = [size(nt, 37, 37) for nt in range(1, len(sizes) + 1)]
    assert all(b >= a for a, b in zip(by_nt, by_nt[1:])) and by_nt[0] < by_nt[-1]
    assert by_nt[0] % 8 == 0 and by_nt[-1] % 8 == 0
    assert len({size(len(sizes), kr, kc) for kr, kc in [(1, 1), (NR, NC), (4096, 4096), (1, 10**6)]}) == 1
    # nothing of the model's size: two tiles' windows and a pass's rows, a few KiB per plan chunk
    assert by_nt[-1] <= 64 << 20
    # one byte short is refused, the size itself passes the check (the call then needs a device, so
    # only the refusal is run here)
    arr = _tensors(N, sizes, 0, frozen_at=-1)
    assert _call(L, arr, len(sizes), ws_bytes=by_nt[-1] - 1) == -EINVAL
    assert "workspace" in _err(L) and str(by_nt[-1]) in _err(L)


def _passes(L, kr, kc, symmetric):
    n = ctypes.c_int32(0)
    assert L.fks_gram_mt_passes(kr, kc, int(symmetric), None, 0, ctypes.byref(n)) == 0, _err(L)
    buf = (ctypes.c_int32 * max(1, 4 * n.value))()
    m = ctypes.c_int32(0)
    assert L.fks_gram_mt_passes(kr, kc, int(symmetric), buf, n.value, ctypes.byref(m)) == 0, _err(L)
    assert m.value == n.value
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


def test_python_constants_are_the_tallest_and_widest_pass():
    _, L = _lib()
    NR, NC = _tile()
    p = _passes(L, 1000, 1000, False)
    assert max(nr for _, nr, _, _ in p) == NR and max(nc for _, _, _, nc in p) == NC
    assert 1 <= NR <= NC and NR + NC <= 19 and NR * NC <= 64


def test_symmetric_passes_cover_the_upper_triangle_once():
    _, L = _lib()
    NR, NC = _tile()
    for k in _ks():
        for kc in (0, k):  # both spellings of the symmetric call's kcols
            passes = _passes(L, k, kc, True)
            cover = np.zeros((k, k), np.int32)
            diag = np.zeros((k, k), bool)
            for r0, nr, c0, nc in passes:
                assert 1 <= nr <= NR and 1 <= nc <= NC and 0 <= r0 and r0 + nr <= k and 0 <= c0 and c0 + nc <= k
                cover[r0:r0 + nr, c0:c0 + nc] += 1
                if c0 == r0:  # the row tile's diagonal pass
                    diag[r0:r0 + nr, c0:c0 + nc] = True
            r, c = np.indices((k, k))
            assert (cover[c >= r] == 1).all(), "every pair c >= r exactly once"
            assert (cover <= 1).all()
            assert diag[(cover > 0) & (c < r)].all(), "a pair c < r lies inside its row tile's diagonal pass"
            assert (r // NR == c // NR)[(cover > 0) & (c < r)].all()


def test_rectangular_passes_cover_every_cell_once():
    _, L = _lib()
    NR, NC = _tile()
    for kr in _ks():
        for kc in _ks():
            passes = _passes(L, kr, kc, False)
            cover = np.zeros((kr, kc), np.int32)
            for r0, nr, c0, nc in passes:
                assert 1 <= nr <= NR and 1 <= nc <= NC and 0 <= r0 and r0 + nr <= kr and 0 <= c0 and c0 + nc <= kc
                cover[r0:r0 + nr, c0:c0 + nc] += 1
            assert (cover == 1).all()
            assert len(passes) == -(-kr // NR) * -(-kc // NC)


def test_passes_argument_errors_and_cap():
    _, L = _lib()
    NR, NC = _tile()
    n = ctypes.c_int32(0)
    buf = (ctypes.c_int32 * 8)()
    assert L.fks_gram_mt_passes(-1, 0, 0, None, 0, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_mt_passes(3, -1, 0, None, 0, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_mt_passes(3, 2, 1, None, 0, ctypes.byref(n)) == -EINVAL  # symmetric: kcols 0 or krows
    assert L.fks_gram_mt_passes(3, 3, 1, None, 0, None) == -EINVAL
    assert L.fks_gram_mt_passes(3, 3, 1, None, 2, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_mt_passes(3, 3, 1, buf, -1, ctypes.byref(n)) == -EINVAL
    # a cap below the count: the first passes, and the whole count
    assert L.fks_gram_mt_passes(100, 100, 0, buf, 2, ctypes.byref(n)) == 0
    assert n.value == len(_passes(L, 100, 100, False)) and tuple(buf[:8]) == (0, NR, 0, NC, 0, NR, NC, NC)


def test_codec_gram_mt_checks_before_touching_a_device():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]  # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="no CPU path"):
        codec.gram_mt(specs, [1, 2])
    with pytest.raises(ValueError, match="shard"):
        codec.gram_mt(specs, [1], shard=2, nshards=2)
    out = codec.gram_mt([], [1, 2, 3])  # no specs: zeros on the CPU
    assert out.shape == (3, 3) and out.dtype == torch.float64 and out.device.type == "cpu" and not out.any()
    assert codec.gram_mt([], [1, 2, 3], [4]).shape == (3, 1)
    # the torch_rocm-only names point to the new ones
    assert "gram_mt" in codec.gram.__doc__


def test_zo_utils_on_stream_forms():
    from fate_llm.algo.fedkseed import zo_utils
    p = torch.nn.Parameter(torch.zeros(64))
    for mode in ("torch_cpu", "torch_rocm"):
        with pytest.raises(ValueError, match="seed 7 "):
            zo_utils.fit_seed_scalars_exact_on_stream([{"params": [p]}], [3, 7, 11, 7], [[torch.zeros(64)]],
                                                      stream_mode=mode)
    assert "synchronises" in zo_utils.fit_seed_scalars_exact_on_stream.__doc__.lower()
    assert "fit_seed_scalars_exact_on_stream" in zo_utils.fit_seed_scalars_exact.__doc__
    assert "seed_gram_on_stream" in zo_utils.seed_gram.__doc__
    out = zo_utils.seed_gram_on_stream([], [1, 2, 3], stream_mode="torch_cpu")  # no parameters: zeros on the CPU
    assert out.shape == (3, 3) and not out.any()
