"""fks_project_mt and fks_project_mt_multi (codec.project_mt, codec.project_mt_multi) over the lists
of tests/mt_layouts.py -- their fast kernels hold two copies of the segment lookup that
fks_expand_mt_kernel shares, and tests/test_gpu_project_mt.py's lists give a launch at most one
segment after word 0.  Reference and bound are that file's: torch's CPU draws per tensor in the
tensor's dtype, the f64 math.fsum of the exact products, and |got - ref| <= n 2^-52 sum|v z|, which
holds for every order of summation (derived there, not tuned); one-hot vectors are exact:
float64(v) float64(z).

  G (four dtype variants): several segments in MT block 0, a block wholly inside a frozen gap, fast
    segments after irregular work; mixed, a launch of one dtype sees the other's segments as gaps.
    One-hot probes at the first and last element of every tensor, elements 7, 8 and 15 of every
    fast segment, both sides of every MT block boundary inside a fast segment or a run, and every
    tiny element pin the element-to-word mapping there.  Shards of five blocks and more shards
    than blocks on G:mixed.
  R: a workgroup walks several blocks, the lookahead crosses into gaps and into the other dtype's
    stretches; a 1,200-entry table of vector pieces.  K = 19, to bound the reference's host time.
  sweep (32 cases): gaps, several segments in a block, both dtypes, odd-phase runs, tiny groups."""
import functools
import math

import numpy as np
import pytest
import torch

import mt_layouts as ML
from test_gpu_expand_mt import SEEDS57
from test_gpu_parity import _dev
from test_gpu_project_mt import U, _dense_vec, _f64, _i64
from test_gpu_project_mt_multi import VDT, _off_boundary

pytestmark = pytest.mark.gpu

SEEDS = SEEDS57[:20]  # tests/test_gpu_project_mt.py's 20 seeds
LISTS = ML.G_NAMES + ["R"] + [f"sweep{c}" for c in range(ML.SWEEP)]


def _k(name):
    return 19 if name == "R" else 20


@functools.lru_cache(maxsize=None)
def _specs(name):
    """one spec list per list, kept for the session (a stable plan key)"""
    from fate_llm.algo.fedkseed import codec
    lst, dev = ML.get(name), _dev()
    return tuple(codec.ParamSpec(torch.empty(n, dtype=ML.DT[d], device=dev), frozen=(i in lst.frozen))
                 for i, (n, d) in enumerate(zip(lst.sizes, lst.dts)))


@functools.lru_cache(maxsize=None)
def _vectors(name):
    """Three f32 vectors over the concatenation (CPU): the dense vector, and two whose pieces hold
    values of f32, bf16 and f16 rotating over the tensors (|v| < 65504: finite as f16), so that the
    same values can be read in place in those dtypes; with the piece dtypes of the two."""
    lst = ML.get(name)
    off = ML.offsets(lst.sizes)
    dense = _dense_vec(off[-1])
    out, dts = [dense], []
    for m in range(2):
        v = (torch.roll(dense, 1000 * m) * (1e-2 * (1 + m))).clamp(-6e4, 6e4)
        dt = [VDT[(i + m) % 3] for i in range(len(lst.sizes))]
        for i in range(len(lst.sizes)):
            v[off[i]:off[i + 1]] = v[off[i]:off[i + 1]].to(dt[i]).float()
        out.append(v)
        dts.append(dt)
    return out, dts


@functools.lru_cache(maxsize=None)
def _case(name):
    """Per vector of _vectors and seed: the reference projection and sum|v z| over the live
    elements; computed once per list and shared."""
    lst = ML.get(name)
    live = ML.live_mask(lst)
    k = _k(name)
    v64 = [v.numpy().astype(np.float64)[live] for v in _vectors(name)[0]]
    ref, sabs = np.zeros((3, k)), np.zeros((3, k))
    for s, z in enumerate(ML.zs(name, SEEDS57[:k])):
        z64 = z.numpy().astype(np.float64)[live]
        for m in range(3):
            p = v64[m] * z64  # exact products
            ref[m, s] = math.fsum(p.tolist())
            sabs[m, s] = float(np.abs(p).sum())
    return {"ref": ref, "sabs": sabs, "n": int(live.sum()), "off": ML.offsets(lst.sizes)}


def _within(got, c, m, what):
    k = got.shape[0]
    err, bound = np.abs(got - c["ref"][m, :k]), c["n"] * U * c["sabs"][m, :k]
    assert (err <= bound).all(), (what, m, err, bound)


# ---- 1. dense vectors
@pytest.mark.parametrize("name", LISTS)
def test_dense_projection_within_f64_sum_bound(name):
    """codec.project_mt on the dense vector, and codec.project_mt_multi on two vectors read in place,
    per-tensor pieces one element past a 16-byte boundary, their dtypes rotating: all within the
    bound, and the in-place rows equal project_mt on the vectors' f32 copies bit for bit."""
    from fate_llm.algo.fedkseed import codec
    dev, lst, c, k = _dev(), ML.get(name), _case(name), _k(name)
    specs = _specs(name)
    what = f"list {name}, sizes {list(lst.sizes)}, dtypes {list(lst.dts)}, K {k}"
    vecs, dts = _vectors(name)
    off = c["off"]
    _within(_f64(codec.project_mt(specs, SEEDS[:k], vecs[0].to(dev))), c, 0, what)
    lists = []
    for m in range(2):
        wide = vecs[1 + m].to(dev)
        lists.append([None if i in lst.frozen else _off_boundary(wide[off[i]:off[i + 1]], dts[m][i], dev)
                      for i in range(len(lst.sizes))])
    got = codec.project_mt_multi(specs, SEEDS[:k], lists)
    for m in range(2):
        _within(_f64(got[m]), c, 1 + m, what)
        want = _i64(codec.project_mt(specs, SEEDS[:k], vecs[1 + m].to(dev)))
        assert np.array_equal(_i64(got[m]), want), (what, m, np.nonzero(_i64(got[m]) != want)[0].tolist())


# ---- 2. one-hot probes
def _probes(name):
    lst = ML.get(name)
    m = ML.mirror_of(lst)
    off = ML.offsets(lst.sizes)
    out = set()
    for i, n in enumerate(lst.sizes):
        if n:
            out |= {off[i], off[i + 1] - 1}
    for s in m.segs:
        out |= {s.elem + 7, s.elem + 8, s.elem + 15}
    for x in list(m.segs) + list(m.runs):  # both sides of the MT block boundaries inside it
        limit = x.limit if isinstance(x, ML.Run) else x.numel
        for w in range(-(-x.start // ML.MT_N) * ML.MT_N, x.start + x.numel, ML.MT_N):
            out |= {x.elem + e for e in (w - x.start - 1, w - x.start) if 0 <= e < limit}
    out |= {t.elem for t in m.tiny}
    return sorted(out)


@pytest.mark.parametrize("name", ML.G_NAMES)
def test_one_hot_is_exact(name):
    """The probes as rows of project_mt_multi, 64 vectors a call (the library takes them in batches
    over the same seeds): row m is float64(v) float64(z[e_m]) for every seed, bit for bit but for
    the sign of a zero, and exactly zero for a frozen element."""
    from fate_llm.algo.fedkseed import codec
    dev, lst = _dev(), ML.get(name)
    specs = _specs(name)
    off = ML.offsets(lst.sizes)
    live = ML.live_mask(lst)
    probes = _probes(name)
    assert len(probes) >= 2 * sum(1 for n in lst.sizes if n) - 2 + 32
    z = np.stack([t.numpy().astype(np.float64) for t in ML.zs(name, SEEDS57[:20])])  # [20, total]
    assert (z[:, probes] != 0.0).mean() > 0.9
    v = float(np.float32(-3.1415927))
    rows = 64
    bufs = torch.zeros((rows, off[-1]), dtype=torch.float32, device=dev)
    lists = [[None if i in lst.frozen else bufs[m, off[i]:off[i + 1]] for i in range(len(lst.sizes))]
             for m in range(rows)]
    bad = []
    for p0 in range(0, len(probes), rows):
        batch = probes[p0:p0 + rows]
        bufs.zero_()
        bufs[torch.arange(len(batch)), torch.tensor(batch)] = v
        got = codec.project_mt_multi(specs, SEEDS, lists[:len(batch)]).cpu().numpy()
        for m, e in enumerate(batch):
            want = np.float64(v) * z[:, e] if live[e] else np.zeros(20)
            if not np.array_equal(got[m], want):
                bad.append((e, int((got[m] != want).sum())))
    assert not bad, f"list {name}: (element, seeds that differ): {bad}"


# ---- 3. shards
@pytest.mark.parametrize("nshards", [5, 32])
def test_shards_on_G_mixed(nshards):
    """Every shard's projection, summed over the shards in f64, against the dense reference within
    the same bound: at 32 seven shards hold no MT block and one holds only the block inside the
    frozen gap; they return exact zeros."""
    from fate_llm.algo.fedkseed import codec
    name = "G:mixed"
    dev, c = _dev(), _case(name)
    dense = _vectors(name)[0][0].to(dev)
    parts = [_f64(codec.project_mt(_specs(name), SEEDS, dense, shard=r, nshards=nshards)) for r in range(nshards)]
    total = np.array([math.fsum(p[s] for p in parts) for s in range(20)])
    _within(total, c, 0, f"{nshards} shards")
    assert sum(not p.view(np.int64).any() for p in parts) >= (8 if nshards == 32 else 0)
