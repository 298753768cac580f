"""fks_gram_mt_bs without a device: header and exports, the argument errors fks_gram_mt_tiled has,
the torch_rocm refusal, the workspace arithmetic and the passes' two forms."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gram_mt_host import EINVAL, ENOTSUP, FAKE, FLAGS, ROOT, SIZES, _err, _lib, _tensors

T = 16  # seeds of a block (csrc/fks_gram_mt_tiled.h kGmtTile); a diagonal pass holds two
KS = [1, 16, 17, 32, 33, 64]


def _call(L, arr, nt, kr=3, kc=2, rows=True, cols=True, shard=0, nshards=1, out=FAKE + (1 << 31),
          ws=FAKE + (1 << 32), ws_bytes=1 << 30):
    r = np.arange(1, max(kr, 1) + 1, dtype=np.uint64)
    c = np.arange(11, max(kc, 1) + 11, dtype=np.uint64)
    return L.fks_gram_mt_bs(ctypes.addressof(arr), nt, r.ctypes.data if rows else None, kr,
                            c.ctypes.data if cols else None, kc, shard, nshards, out, ws, ws_bytes, None)


def _size(L, arr, nt, kr, kc):
    nbytes = ctypes.c_size_t(0)
    rc = L.fks_gram_mt_bs_workspace_size(ctypes.addressof(arr), nt, kr, kc, ctypes.byref(nbytes))
    return rc, nbytes.value


def test_symbols_in_the_header_and_exported():
    N, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "fks.h")).read()
    for name in ("fks_gram_mt_bs", "fks_gram_mt_bs_workspace_size", "fks_gram_mt_bs_passes"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in N.EXPORTED and hasattr(L, name)
    assert L.fks_abi_version() == 1  # additive


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("what,kw", [
    ("null row seeds", dict(rows=False)), ("negative krows", dict(kr=-1)),
    ("negative kcols", dict(kc=-1)), ("null out", dict(out=None)),
    ("misaligned out", dict(out=FAKE + (1 << 31) + 4)), ("null out, symmetric", dict(cols=False, kc=0, out=None)),
    ("shard past the end", dict(shard=2, nshards=2)), ("no shards", dict(shard=0, nshards=0)),
    ("kcols neither 0 nor krows without column seeds", dict(cols=False, kc=2)), ("null workspace", dict(ws=None)),
    ("misaligned workspace", dict(ws=FAKE + (1 << 32) + 4)), ("workspace too small", dict(ws_bytes=64)),
    ("workspace too small, symmetric", dict(cols=False, kc=3, ws_bytes=64)),
])
def test_einval_from_the_arguments(what, kw, flags):
    N, L = _lib()
    arr = _tensors(N, SIZES, flags)
    assert _call(L, arr, len(SIZES), **kw) == -EINVAL and _err(L), what


def test_refuses_the_rocm_stream():
    N, L = _lib()
    arr = _tensors(N, SIZES, N.STREAM_ROCM)
    for kw in (dict(), dict(cols=False, kc=0)):
        assert _call(L, arr, len(SIZES), **kw) == -ENOTSUP
        assert "FKS_STREAM_ROCM" in _err(L) and re.search(r"\bfks_gram_tiled\b", _err(L))
    assert _size(L, arr, len(SIZES), 4, 4)[0] == -ENOTSUP and re.search(r"\bfks_gram_tiled\b", _err(L))


def test_workspace_follows_the_list_and_not_the_seed_counts():
    N, L = _lib()
    sizes = [4096, 1000, 3, 700_001, 7, 65536, 3_000_001]

    def size(nt, kr, kc):
        rc, b = _size(L, _tensors(N, sizes[:nt], 0, frozen_at=-1), nt, kr, kc)
        assert rc == 0, _err(L)
        return b

    whole = size(len(sizes), 37, 37)
    assert size(1, 37, 37) < whole and whole % 8 == 0
    assert {size(len(sizes), kr, kc) for kr, kc in [(1, 1), (T, T), (64, 64), (4096, 4096), (1, 10**6)]} == {whole}
    arr = _tensors(N, sizes, 0, frozen_at=-1)
    assert _call(L, arr, len(sizes), ws_bytes=whole - 1) == -EINVAL  # one byte short is refused
    assert "workspace" in _err(L) and str(whole) in _err(L)


def _passes(L, kr, kc, symmetric):
    n, m = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.fks_gram_mt_bs_passes(kr, kc, int(symmetric), None, 0, ctypes.byref(n)) == 0, _err(L)
    buf = (ctypes.c_int32 * max(1, 4 * n.value))()
    assert L.fks_gram_mt_bs_passes(kr, kc, int(symmetric), buf, n.value, ctypes.byref(m)) == 0, _err(L)
    assert m.value == n.value
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


@pytest.mark.parametrize("kr", KS)
def test_the_passes_forms_cover_every_cell_once(kr):
    _, L = _lib()
    r, c = np.indices((kr, kr))
    for kc, symmetric in [(0, True), (kr, True)] + [(k, False) for k in KS]:
        passes = _passes(L, kr, kc, symmetric)
        cover = np.zeros((kr, kr if symmetric else kc), np.int32)
        ndiag = 0
        for r0, nr, c0, nc in passes:
            assert r0 + nr <= cover.shape[0] and c0 + nc <= cover.shape[1] and r0 % T == 0 and c0 % T == 0
            if symmetric and c0 == r0:  # the diagonal form: the pairs c >= r of up to 32 consecutive seeds
                assert 1 <= nr == nc <= 2 * T and r0 % (2 * T) == 0
                cover[r0:r0 + nr, c0:c0 + nc] += np.triu(np.ones((nr, nr), np.int32))
                ndiag += 1
            else:  # the pair form: one block against one block
                assert 1 <= nr <= T and 1 <= nc <= T and (c0 > r0 or not symmetric)
                cover[r0:r0 + nr, c0:c0 + nc] += 1
        if symmetric:  # every pair c >= r once, nothing below the diagonal
            assert (cover[c >= r] == 1).all() and (cover[c < r] == 0).all() and ndiag == -(-kr // (2 * T))
        else:
            assert (cover == 1).all() and len(passes) == -(-kr // T) * -(-kc // T)
    assert len(_passes(L, 64, 0, True)) == 6  # two diagonal and four pair passes


def test_zo_utils_refuse_the_default_stream():
    import torch
    from fate_llm.algo.fedkseed import zo_utils
    groups = [{"params": [torch.nn.Parameter(torch.zeros(32))]}]
    for fn, args in ((zo_utils.seed_gram_bitsliced, ()), (zo_utils.fit_seed_scalars_exact_bitsliced, ([[torch.zeros(32)]],))):
        with pytest.raises(NotImplementedError, match="torch_cpu stream only.*torch_rocm"):
            fn(groups, [1, 2], *args, stream_mode="torch_rocm")
