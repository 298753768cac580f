"""Host-side checks of the tiled seed-basis Gram matrix (fks_gram_tiled, fks_gram_tiled_workspace_size,
fks_gram_tiled_passes, codec.gram_tiled, zo_utils.seed_gram_tiled / fit_seed_scalars_exact_tiled); no
device needed.  As tests/test_gram_host.py for fks_gram: every argument error of the C call is raised
from the arguments alone, before any device work, with a message; the trivial calls succeed; the
workspace follows the work items and not the seed counts and stays far below the model's size; the
pass tiling covers what it must."""
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
KS = [0, 1, 15, 16, 17, 64, 65, 85, 200]


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


def _call(L, arr, nt, kr=3, kc=2, rows=True, cols=True, shard=0, nshards=1, out=FAKE + (1 << 31),
          ws=FAKE + (1 << 32), ws_bytes=1 << 30):
    r = np.arange(1, max(kr, 1) + 1, dtype=np.uint64)
    c = np.arange(11, max(kc, 1) + 11, dtype=np.uint64)
    return L.fks_gram_tiled(ctypes.addressof(arr), nt, r.ctypes.data if rows else None, kr,
                            c.ctypes.data if cols else None, kc, shard, nshards, out, ws, ws_bytes, None)


def _err(L):
    return L.fks_last_error().decode()


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    with open(os.path.join(ROOT, "include", "fks.h")) as f:
        hdr = f.read()
    for name in ("fks_gram_tiled", "fks_gram_tiled_workspace_size", "fks_gram_tiled_passes"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive
    assert "NOT fks_gram's order" in hdr  # the header says that the two calls do not share their bits


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
def test_einval_from_the_arguments(what, kw):
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    assert _call(L, arr, len(SIZES), **kw) == -EINVAL, what
    assert _err(L), what


@pytest.mark.parametrize("flags", [0, 16])  # the CPU generator's stream, and its FKS_LIBM flavour
def test_refuses_the_cpu_stream(flags):
    N, L = _lib()
    assert flags in (0, N.LIBM)
    arr = _tensors(N, SIZES, flags, dtype=0)
    for kw in (dict(), dict(cols=False, kc=0)):
        assert _call(L, arr, len(SIZES), **kw) == -ENOTSUP
        assert "fks_gram_tiled" in _err(L) and "torch_cpu" in _err(L) and "FKS_STREAM_ROCM" in _err(L)
        if flags:
            assert "FKS_LIBM" in _err(L)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_gram_tiled_workspace_size(ctypes.addressof(arr), len(SIZES), 4, 4, ctypes.byref(nbytes)) == -ENOTSUP
    assert "torch_cpu" in _err(L)


def test_trivial_calls_succeed():
    N, L = _lib()
    nt = len(SIZES)
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    none = dict(out=None, ws=None, ws_bytes=0)
    assert _call(L, arr, nt, kr=0, rows=False, **none) == 0, _err(L)             # no row seeds
    assert _call(L, arr, nt, kr=0, kc=0, rows=False, cols=False, **none) == 0, _err(L)  # symmetric, K = 0
    assert _call(L, arr, nt, kc=0, **none) == 0, _err(L)                         # column seeds given, none of them
    assert _call(L, arr, 0, kr=0, kc=0, **none) == 0, _err(L)                    # no tensors
    nbytes = ctypes.c_size_t(0)
    assert L.fks_gram_tiled_workspace_size(ctypes.addressof(arr), 0, 4, 3, ctypes.byref(nbytes)) == 0
    assert L.fks_gram_tiled_workspace_size(ctypes.addressof(arr), nt, 0, 0, ctypes.byref(nbytes)) == 0
    assert L.fks_gram_tiled_workspace_size(ctypes.addressof(arr), nt, 1, 1, None) == -EINVAL
    assert L.fks_gram_tiled_workspace_size(ctypes.addressof(arr), nt, -1, 1, ctypes.byref(nbytes)) == -EINVAL
    assert L.fks_gram_tiled_workspace_size(ctypes.addressof(arr), nt, 1, -1, ctypes.byref(nbytes)) == -EINVAL


def _ws(N, L, sizes, kr, kc, dtype=1):
    arr = _tensors(N, sizes, N.STREAM_ROCM, dtype=dtype, frozen_at=-1)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_gram_tiled_workspace_size(ctypes.addressof(arr), len(sizes), kr, kc, ctypes.byref(nbytes)) == 0, _err(L)
    return nbytes.value


def test_workspace_follows_the_items_and_not_the_seed_counts():
    N, L = _lib()
    from fate_llm.algo.fedkseed import codec
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001]
    by_nt = [_ws(N, L, sizes[:nt], 37, 37) for nt in range(1, len(sizes) + 1)]
    assert all(b >= a for a, b in zip(by_nt, by_nt[1:])) and by_nt[0] < by_nt[-1]
    assert by_nt[0] >= 256 and by_nt[0] % 8 == 0
    assert len({_ws(N, L, sizes, k, k) for k in (1, 37, 4096)}) == 1
    assert len({_ws(N, L, sizes, kr, kc) for kr, kc in [(0, 0), (1, 1), (64, 64), (65, 17), (1, 10**6)]}) == 1
    # the workgroup partials of one pass and nothing else: 8 bytes x the tile's cells per workgroup
    tr, tc = codec._gram_tiled_tile()
    assert tr % 16 == 0 and tc % 16 == 0 and tc >= tr
    assert by_nt[-1] % (8 * tr * tc) == 0
    # a list of one 256-item chunk is one workgroup
    assert _ws(N, L, [7], 5, 5) == 8 * tr * tc


def test_workspace_of_the_7b_layout_is_far_below_the_model():
    """The 291 tensors of the Llama-2-7B layout in bf16, on the caps the library falls back to
    without a device (an MI355X's) or on the device's own: tens of MiB at most, the same for
    every K."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    N, L = _lib()
    numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
    assert len(numels) == 291
    sizes = {_ws(N, L, numels, k, k, dtype=1) for k in (1, 37, 4096)}
    assert len(sizes) == 1
    nbytes = sizes.pop()
    print(f"fks_gram_tiled workspace, 7B bf16 layout: {nbytes} bytes")
    assert 0 < nbytes < 64 << 20


def _passes(L, kr, kc, symmetric):
    n = ctypes.c_int32(0)
    assert L.fks_gram_tiled_passes(kr, kc, int(symmetric), None, 0, ctypes.byref(n)) == 0, _err(L)
    buf = (ctypes.c_int32 * max(1, 4 * n.value))()
    m = ctypes.c_int32(0)
    assert L.fks_gram_tiled_passes(kr, kc, int(symmetric), buf, n.value, ctypes.byref(m)) == 0, _err(L)
    assert m.value == n.value
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


def _tile():
    from fate_llm.algo.fedkseed import codec
    return codec._gram_tiled_tile()


@pytest.mark.parametrize("k", KS)
def test_symmetric_passes_cover_the_upper_triangle(k):
    _, L = _lib()
    TR, TC = _tile()
    for kc in (0, k):  # both spellings of the symmetric call's kcols
        cover = np.zeros((k, k), np.int32)
        for r0, nr, c0, nc in _passes(L, k, kc, True):
            assert 1 <= nr <= TR and 1 <= nc <= TC and 0 <= r0 and r0 + nr <= k and 0 <= c0 and c0 + nc <= k
            assert c0 >= r0, "a pass on or above the diagonal"
            cover[r0:r0 + nr, c0:c0 + nc] += 1
        r, c = np.indices((k, k))
        assert (cover[c >= r] >= 1).all(), "every pair c >= r at least once"
        assert (cover <= 1).all()
        # the waste is bounded: below the diagonal only cells whose row and column share a row tile
        assert (r // TR == c // TR)[(cover > 0) & (c < r)].all()


@pytest.mark.parametrize("kr", KS)
@pytest.mark.parametrize("kc", KS)
def test_rectangular_passes_cover_every_cell_once(kr, kc):
    _, L = _lib()
    TR, TC = _tile()
    passes = _passes(L, kr, kc, False)
    cover = np.zeros((kr, kc), np.int32)
    for r0, nr, c0, nc in passes:
        assert 1 <= nr <= TR and 1 <= nc <= TC and 0 <= r0 and r0 + nr <= kr and 0 <= c0 and c0 + nc <= kc
        cover[r0:r0 + nr, c0:c0 + nc] += 1
    assert (cover == 1).all()
    assert len(passes) == -(-kr // TR) * -(-kc // TC)


def test_pass_count_of_k_4096():
    _, L = _lib()
    TR, TC = _tile()
    n = len(_passes(L, 4096, 0, True))
    old = ctypes.c_int32(0)
    assert L.fks_gram_passes(4096, 0, 1, None, 0, ctypes.byref(old)) == 0
    rows = 4096 // TR
    want = sum(-(-(4096 - r * TR) // TC) for r in range(rows))
    assert n == want and n * 16 < old.value, \
        f"symmetric K = 4096: {n} passes of {TR} x {TC} seeds (fks_gram: {old.value} of 4 x 32)"
    if (TR, TC) == (64, 64):
        assert n == 2080, f"symmetric K = 4096: {n} passes"


def test_passes_argument_errors_and_cap():
    _, L = _lib()
    TR, TC = _tile()
    n = ctypes.c_int32(0)
    buf = (ctypes.c_int32 * 8)()
    assert L.fks_gram_tiled_passes(-1, 0, 0, None, 0, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_tiled_passes(3, -1, 0, None, 0, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_tiled_passes(3, 2, 1, None, 0, ctypes.byref(n)) == -EINVAL  # symmetric: kcols 0 or krows
    assert L.fks_gram_tiled_passes(3, 3, 1, None, 0, None) == -EINVAL
    assert L.fks_gram_tiled_passes(3, 3, 1, None, 2, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_tiled_passes(3, 3, 1, buf, -1, ctypes.byref(n)) == -EINVAL
    # a cap below the count: the first passes, and the whole count
    assert L.fks_gram_tiled_passes(300, 300, 0, buf, 2, ctypes.byref(n)) == 0
    assert n.value == len(_passes(L, 300, 300, False)) and tuple(buf[:8]) == (0, TR, 0, TC, 0, TR, TC, TC)


def test_fit_seed_scalars_exact_tiled_refuses_duplicate_seeds():
    from fate_llm.algo.fedkseed import zo_utils
    p = torch.nn.Parameter(torch.zeros(64))
    with pytest.raises(ValueError, match="seed 7 "):
        zo_utils.fit_seed_scalars_exact_tiled([{"params": [p]}], [3, 7, 11, 7], [[torch.zeros(64)]],
                                              stream_mode="torch_rocm")
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        zo_utils.fit_seed_scalars_exact_tiled([{"params": [p]}], [3, 7], [[torch.zeros(64)]], stream_mode="torch_cpu")
    assert "synchronis" in zo_utils.fit_seed_scalars_exact_tiled.__doc__.lower()


def test_codec_gram_tiled_refuses_torch_cpu_and_bad_shards_before_touching_a_device():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]  # CPU tensors: any device access would raise something else
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        codec.gram_tiled(specs, [1, 2], stream_mode="torch_cpu")
    with pytest.raises(NotImplementedError, match="torch_cpu"):  # "auto" on CPU tensors resolves to torch_cpu
        codec.gram_tiled(specs, [1, 2], [3], stream_mode="auto")
    with pytest.raises(ValueError, match="shard"):
        codec.gram_tiled(specs, [1], stream_mode="torch_rocm", shard=2, nshards=2)
    out = codec.gram_tiled([], [1, 2, 3], stream_mode="torch_rocm")  # no specs: zeros on the CPU
    assert out.shape == (3, 3) and out.dtype == torch.float64 and out.device.type == "cpu" and not out.any()
    assert codec.gram_tiled([], [1, 2, 3], [4], stream_mode="torch_rocm").shape == (3, 1)
