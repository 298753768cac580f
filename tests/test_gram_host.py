"""Host-side checks of the seed-basis Gram matrix (fks_gram, fks_gram_workspace_size,
fks_gram_passes, codec.gram, zo_utils.seed_gram / fit_seed_scalars_exact); no device needed.
Every argument error of the C call is raised from the arguments alone, before any device work,
with a message; the trivial calls succeed; the workspace follows the work items and not the seed
counts; the pass tiling covers what it must, once; the host solver agrees with numpy's
least squares and refuses a singular matrix."""
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
KS = [0, 1, 4, 5, 32, 33, 37, 100]


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
    return L.fks_gram(ctypes.addressof(arr), nt, r.ctypes.data if rows else None, kr,
                      c.ctypes.data if cols else None, kc, shard, nshards, out, ws, ws_bytes, None)


def _err(L):
    return L.fks_last_error().decode()


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    with open(os.path.join(ROOT, "include", "fks.h")) as f:
        hdr = f.read()
    for name in ("fks_gram", "fks_gram_workspace_size", "fks_gram_passes"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive


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
        assert "fks_gram" in _err(L) and "torch_cpu" in _err(L) and "FKS_STREAM_ROCM" in _err(L)
        if flags:
            assert "FKS_LIBM" in _err(L)
    nbytes = ctypes.c_size_t(0)
    assert L.fks_gram_workspace_size(ctypes.addressof(arr), len(SIZES), 4, 4, ctypes.byref(nbytes)) == -ENOTSUP
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
    assert L.fks_gram_workspace_size(ctypes.addressof(arr), 0, 4, 3, ctypes.byref(nbytes)) == 0
    assert L.fks_gram_workspace_size(ctypes.addressof(arr), nt, 0, 0, ctypes.byref(nbytes)) == 0
    assert L.fks_gram_workspace_size(ctypes.addressof(arr), nt, 1, 1, None) == -EINVAL
    assert L.fks_gram_workspace_size(ctypes.addressof(arr), nt, -1, 1, ctypes.byref(nbytes)) == -EINVAL
    assert L.fks_gram_workspace_size(ctypes.addressof(arr), nt, 1, -1, ctypes.byref(nbytes)) == -EINVAL


def test_workspace_follows_the_items_and_not_the_seed_counts():
    N, L = _lib()
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001]

    def size(nt, kr, kc):
        arr = _tensors(N, sizes[:nt], N.STREAM_ROCM, frozen_at=-1)
        nbytes = ctypes.c_size_t(0)
        assert L.fks_gram_workspace_size(ctypes.addressof(arr), nt, kr, kc, ctypes.byref(nbytes)) == 0, _err(L)
        return nbytes.value

    by_nt = [size(nt, 37, 37) for nt in range(1, len(sizes) + 1)]
    assert all(b >= a for a, b in zip(by_nt, by_nt[1:])) and by_nt[0] < by_nt[-1]
    assert by_nt[0] >= 256 and by_nt[0] % 8 == 0
    assert len({size(len(sizes), kr, kc) for kr, kc in [(0, 0), (1, 1), (4, 32), (5, 33), (4096, 4096), (1, 10**6)]}) == 1
    # the block partials of one pass and nothing else: 8 bytes x rows of a pass x 32 columns per workgroup
    from fate_llm.algo.fedkseed import codec
    assert by_nt[-1] % (8 * codec.GRAM_PASS_ROWS * 32) == 0


def _passes(L, kr, kc, symmetric):
    n = ctypes.c_int32(0)
    assert L.fks_gram_passes(kr, kc, int(symmetric), None, 0, ctypes.byref(n)) == 0, _err(L)
    buf = (ctypes.c_int32 * max(1, 4 * n.value))()
    m = ctypes.c_int32(0)
    assert L.fks_gram_passes(kr, kc, int(symmetric), buf, n.value, ctypes.byref(m)) == 0, _err(L)
    assert m.value == n.value
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


def _nr():
    from fate_llm.algo.fedkseed import codec
    assert codec.GRAM_PASS_ROWS >= 4
    # the Python constant is the library's: the tallest pass of a tall call
    assert max(nr for _, nr, _, _ in _passes(_lib()[1], 1000, 1, False)) == codec.GRAM_PASS_ROWS
    return codec.GRAM_PASS_ROWS


@pytest.mark.parametrize("k", KS)
def test_symmetric_passes_cover_the_upper_triangle_once(k):
    _, L = _lib()
    NR = _nr()
    for kc in (0, k):  # both spellings of the symmetric call's kcols
        passes = _passes(L, k, kc, True)
        cover = np.zeros((k, k), np.int32)
        diag = np.zeros((k, k), bool)
        for r0, nr, c0, nc in passes:
            assert 1 <= nr <= NR and 1 <= nc <= 32 and 0 <= r0 and r0 + nr <= k and 0 <= c0 and c0 + nc <= k
            cover[r0:r0 + nr, c0:c0 + nc] += 1
            if c0 < r0 + nr and r0 < c0 + nc:  # a tile that meets the diagonal band of its own rows
                diag[r0:r0 + nr, c0:c0 + nc] = True
        r, c = np.indices((k, k))
        assert (cover[c >= r] == 1).all(), "every pair c >= r exactly once"
        assert (cover <= 1).all()
        assert diag[(cover > 0) & (c < r)].all(), "a pair c < r lies inside a diagonal tile"
        # the waste is bounded: below the diagonal only cells whose row and column share a row tile
        assert (r // NR == c // NR)[(cover > 0) & (c < r)].all()


@pytest.mark.parametrize("kr", KS)
@pytest.mark.parametrize("kc", KS)
def test_rectangular_passes_cover_every_cell_once(kr, kc):
    _, L = _lib()
    NR = _nr()
    passes = _passes(L, kr, kc, False)
    cover = np.zeros((kr, kc), np.int32)
    for r0, nr, c0, nc in passes:
        assert 1 <= nr <= NR and 1 <= nc <= 32 and 0 <= r0 and r0 + nr <= kr and 0 <= c0 and c0 + nc <= kc
        cover[r0:r0 + nr, c0:c0 + nc] += 1
    assert (cover == 1).all()
    assert len(passes) == -(-kr // NR) * -(-kc // 32)


def test_passes_argument_errors_and_cap():
    _, L = _lib()
    n = ctypes.c_int32(0)
    buf = (ctypes.c_int32 * 8)()
    assert L.fks_gram_passes(-1, 0, 0, None, 0, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_passes(3, -1, 0, None, 0, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_passes(3, 2, 1, None, 0, ctypes.byref(n)) == -EINVAL  # symmetric: kcols 0 or krows
    assert L.fks_gram_passes(3, 3, 1, None, 0, None) == -EINVAL
    assert L.fks_gram_passes(3, 3, 1, None, 2, ctypes.byref(n)) == -EINVAL
    assert L.fks_gram_passes(3, 3, 1, buf, -1, ctypes.byref(n)) == -EINVAL
    # a cap below the count: the first passes, and the whole count
    assert L.fks_gram_passes(100, 100, 0, buf, 2, ctypes.byref(n)) == 0
    assert n.value == len(_passes(L, 100, 100, False)) and tuple(buf[:8]) == (0, _nr(), 0, 32, 0, _nr(), 32, 32)


def test_solver_against_lstsq():
    from fate_llm.algo.fedkseed import zo_utils
    rng = np.random.default_rng(7)
    Z = rng.standard_normal((3000, 40))
    d = rng.standard_normal((3, 3000))
    want = np.stack([np.linalg.lstsq(Z, v, rcond=None)[0] for v in d])
    got = zo_utils._solve_normal_equations(Z.T @ Z, d @ Z)
    assert got.shape == (3, 40) and got.dtype == np.float64
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"normal equations against lstsq: relative {err:.2e}")
    assert err <= 1e-9


def test_solver_refuses_a_singular_matrix():
    from fate_llm.algo.fedkseed import zo_utils
    rng = np.random.default_rng(8)
    Z = rng.standard_normal((30, 40))  # K larger than N: rank 30
    with pytest.raises(ValueError, match="positive definite"):
        zo_utils._solve_normal_equations(Z.T @ Z - 1e-6 * np.eye(40), np.ones((1, 40)))
    Z = rng.standard_normal((300, 5))
    Z[:, 4] = Z[:, 1]  # a repeated column; the shift keeps rounding from hiding it
    with pytest.raises(ValueError, match="positive definite"):
        zo_utils._solve_normal_equations(Z.T @ Z - 1e-9 * np.eye(5), np.ones((1, 5)))


def test_fit_seed_scalars_exact_refuses_duplicate_seeds():
    from fate_llm.algo.fedkseed import zo_utils
    p = torch.nn.Parameter(torch.zeros(64))
    with pytest.raises(ValueError, match="seed 7 "):
        zo_utils.fit_seed_scalars_exact([{"params": [p]}], [3, 7, 11, 7], [[torch.zeros(64)]], stream_mode="torch_rocm")
    for f in (zo_utils.fit_seed_scalars, zo_utils.fit_seed_scalars_multi, zo_utils.fit_seed_scalars_in_place):
        assert "fit_seed_scalars_exact" in f.__doc__  # the approximate forms point to the exact one
    assert "synchronises" in zo_utils.fit_seed_scalars_exact.__doc__.lower()


def test_codec_gram_refuses_torch_cpu_and_bad_shards_before_touching_a_device():
    from fate_llm.algo.fedkseed import codec
    specs = [codec.ParamSpec(torch.zeros(16))]  # CPU tensors: any device access would raise something else
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        codec.gram(specs, [1, 2], stream_mode="torch_cpu")
    with pytest.raises(NotImplementedError, match="torch_cpu"):  # "auto" on CPU tensors resolves to torch_cpu
        codec.gram(specs, [1, 2], [3], stream_mode="auto")
    with pytest.raises(ValueError, match="shard"):
        codec.gram(specs, [1], stream_mode="torch_rocm", shard=2, nshards=2)
    out = codec.gram([], [1, 2, 3], stream_mode="torch_rocm")  # no specs: zeros on the CPU
    assert out.shape == (3, 3) and out.dtype == torch.float64 and out.device.type == "cpu" and not out.any()
    assert codec.gram([], [1, 2, 3], [4], stream_mode="torch_rocm").shape == (3, 1)
