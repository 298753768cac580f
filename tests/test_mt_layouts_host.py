"""tests/mt_layouts.py from the host side, on a machine without a GPU (fake pointers, never
dereferenced): the mirror's stream length equals fks_stream_length for every list -- G in its four
dtype variants, R, the 32 sweep cases --, its count of table entries equals the one
fks_expand_mt_multi_workspace_size lays its table out for, and the lists hold what the device tests
rely on to reach the kernels' branches:

  G  ten fast segments with one non-f16 dtype, three of them inside MT block 0, block 1 wholly
     inside the frozen gap, fast segments after tiny groups, after the ragged pair and after the
     frozen stretch, four runs, 32 tiny elements; mixed, both non-f16 dtypes keep fast segments and
     the f32 launch walks a long stretch of blocks with no segment of its own;
  R  360 fast segments, 40 runs, 800 tiny elements, 1,816 MT blocks, segment starts at every
     16-aligned phase of the block;
  sweep: over the 32 cases enough of them with fast segments, with a gap between two segments of
     one dtype, with three segments of a dtype in one block, with both dtypes' segments, with runs
     at a non-zero phase and with tiny elements.

These are conditions on the inputs, not on the library: they keep the device tests from passing on
layouts that never reach the branches."""
import ctypes

import pytest

import mt_layouts as ML
from test_expand_host import FAKE, _err, _lib

CPU = 0  # the flag of the CPU generator's stream
LISTS = ML.G_NAMES + ["R"] + [f"sweep{c}" for c in range(ML.SWEEP)]


def _get(name):
    return ML.sweep(int(name[5:])) if name.startswith("sweep") else ML.named(name)


def _tensors(N, lst):
    """the list as the device tests pass it: fake 16-byte aligned addresses"""
    code = {"float32": N.F32, "bfloat16": N.BF16, "float16": N.F16}
    arr = (N.FksTensor * max(1, len(lst.sizes)))()
    at = FAKE
    for i, (n, d) in enumerate(zip(lst.sizes, lst.dts)):
        arr[i].data = at if n else None
        arr[i].numel = n
        arr[i].dtype = code[d]
        arr[i].flags = CPU | (N.FROZEN if i in lst.frozen else 0)
        at += 4 * n + 256 - (4 * n) % 256
    return arr


@pytest.mark.parametrize("name", LISTS)
def test_mirror_equals_the_library(name):
    N, L = _lib()
    lst = _get(name)
    m = ML.mirror_of(lst)
    arr = _tensors(N, lst)
    nt = len(lst.sizes)
    words = ctypes.c_int64(-1)
    assert L.fks_stream_length(ctypes.addressof(arr), nt, ctypes.byref(words)) == 0, _err(L)
    assert words.value == m.stream_len
    # 16 outputs more are 256 bytes per table entry, whatever the alignment of the table's end

    def size(nvec, shard=0, nshards=1):
        nbytes = ctypes.c_size_t(0)
        rc = L.fks_expand_mt_multi_workspace_size(ctypes.addressof(arr), nt, 1, nvec, shard, nshards,
                                                  ctypes.byref(nbytes))
        assert rc == 0, _err(L)
        return nbytes.value

    assert size(32) - size(16) == 256 * (len(m.segs) + len(m.runs) + len(m.tiny))


def test_facts_of_G():
    for d in ("bfloat16", "float32"):
        m = ML.mirror_of(ML.named("G:" + d))
        assert sum(ML.G_SIZES) == 15088 and ML.nblocks(m) == 25
        assert [s.tensor for s in m.segs] == [0, 3, 4, 6, 8, 11, 14, 16, 19, 20]
        assert sum(s.start + s.numel <= ML.MT_N for s in m.segs) == 3  # three inside MT block 0
        f = ML.facts(m)
        assert f["gap"] and f["three_in_a_block"] and f["empty_block_between"]
        # block 1 lies wholly inside the frozen tensor's words
        froz = sum(ML.G_SIZES[:5]) - 8 + 16  # the 5 + 3 serial values are 4 pairs: 16 words
        assert froz == 80 == m.segs[2].start + m.segs[2].numel and m.segs[3].start == froz + 1248
        assert froz <= ML.MT_N and 2 * ML.MT_N <= froz + 1248
        # after the tiny groups (tensors 1, 2; 7; 9, 10; 17, 18), the ragged pair (12, 13), the frozen stretch (5)
        assert all(ML.G_SIZES[s.tensor - 1] < 16 for s in m.segs if s.tensor in (3, 8, 11, 19))
        assert [r.tensor for r in m.runs] == [12, 12, 13, 13] and m.segs[6].tensor == 14
        assert m.runs[2].start % 16 == 8 and m.segs[6].start % 16 == 0
        assert len(m.tiny) == 32 and sum(t.sin for t in m.tiny) == 16
    m = ML.mirror_of(ML.named("G:float16"))
    assert not m.segs and len(m.runs) == 10 + 4 and len(m.tiny) == 32
    lst = ML.named("G:mixed")
    m = ML.mirror_of(lst)
    assert set(lst.dts) == set(ML.CYC)
    b, f = ML.segs_of(m, "bfloat16"), ML.segs_of(m, "float32")
    assert len(b) >= 2 and len(f) >= 2 and ML.facts(m)["both"]
    # the f32 launch walks at least 17 blocks in a row with no segment of its own
    gaps = [y.start // ML.MT_N - (x.start + x.numel - 1) // ML.MT_N - 1 for x, y in zip(f, f[1:])]
    assert max(gaps) >= 17
    # the f16 tensors of fast shape become runs at phase 0
    assert all(r.dtype == "float16" and r.start % 16 == 0 for r in m.runs if r.tensor not in (12, 13))
    assert sum(r.tensor not in (12, 13) for r in m.runs) == 10 - len(b) - len(f) > 0


def test_facts_of_R():
    lst = ML.named("R")
    m = ML.mirror_of(lst)
    assert len(lst.sizes) == 800 and sum(lst.sizes) == 1_132_000 and ML.nblocks(m) == 1816
    assert (len(m.segs), len(m.runs), len(m.tiny)) == (360, 40, 800)
    assert ML.nblocks(m) > 3 * 600  # more blocks than plan chunks on a device of up to 600 CUs
    assert len({s.start % ML.MT_N for s in m.segs}) == ML.MT_N // 16  # every 16-aligned phase of the block
    f = ML.facts(m)
    assert f["gap"] and f["three_in_a_block"] and f["both"] and not f["odd_phase_run"]
    for d in ("bfloat16", "float32"):  # the other dtype's periods are whole blocks without a segment
        assert ML.facts(ML.Mirror(ML.segs_of(m, d), [], [], m.stream_len))["empty_block_between"]


def test_the_sweep_reaches_the_branches():
    fs = [ML.facts(ML.mirror_of(ML.sweep(c))) for c in range(ML.SWEEP)]
    count = {k: sum(bool(f[k]) for f in fs) for k in fs[0]}
    print(count, max(sum(ML.sweep(c).sizes) for c in range(ML.SWEEP)))
    assert ML.SWEEP == 32
    assert count["fast"] >= 20
    assert count["gap"] >= 12
    assert count["three_in_a_block"] >= 6
    assert count["both"] >= 6
    assert count["odd_phase_run"] >= 8
    assert count["tiny"] >= 8
    assert all(4 <= len(ML.sweep(c).sizes) for c in range(ML.SWEEP))
    assert any("float32" in ML.sweep(c).dts for c in range(ML.SWEEP))
