"""Seed-basis projection on the torch_cpu stream (fks_project_mt, codec.project_mt, and
zo_utils.seed_projections / fit_seed_scalars routed there): out[s] = <vec, z_s>, z_s the CPU
generator's MT19937 draw.

The reference is torch's CPU generator, which is what the reference implementation draws on this
stream: torch.manual_seed(s), then torch.normal(0, 1, (n,), dtype) per tensor in order on the CPU
(frozen ones drawn and dropped), widened to float64 and dotted with vec by math.fsum of the
products -- each exact in f64 (24 x 24 significand bits), so fsum returns the correctly rounded
exact value.  test_gpu_project.py's scheme with the draw moved to the CPU.

Bound of the dense tests: the kernels add exact products in f64 in some fixed order; ANY order
of n terms errs by at most (n - 1) u sum|v z| (1 + O(n u)), u = 2^-53, so
|got - ref| <= n 2^-52 sum|v z| holds for every correct implementation (derived, not tuned).
One-hot calls need no bound: every other product is an exact zero, so the result equals
float64(v) float64(z_s[e]) (a z of exactly 0, which the 8-bit uniforms of bf16 give once in 256
draws, makes both sides a zero).

Tensor list, per dtype, the smallest that reaches every branch of the two kernels:
  1,048,576  fast; 1,681 MT blocks, so plan chunks of 2 and 3 blocks and chunk-to-chunk carries
  4,096      fast
  3, frozen  serial draws; leaves a cached second value behind
  1,000      the stream is at phase 8: a run at a non-zero phase, a ragged head with its last 16
             elements masked, 16 fresh tail words
  7          its first element takes the value the frozen tensor cached, across the run before it
  65,536     an irregular run whose 16-blocks straddle MT block boundaries
  0          empty
  48         a short run at a non-zero phase
(for f16 every run is irregular); k = 1 (a partial pass), 19 (one full pass), 20 (full + partial).

The bounds above leave the summation order free, but fks.h promises one fixed order, so the bits
are pinned too: tests/golden/project_mt_parent.json holds what the library of a recorded commit
returned for this list (tests/golden/make_project_mt_parent.py writes it with record_bits below)."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
DTYPES = ["float32", "bfloat16", "float16"]
SIZES = [1 << 20, 4096, 3, 1000, 7, 65536, 0, 48]
FROZEN = 2
_g = torch.Generator().manual_seed(20261020)
SEEDS = [0, 2**32 - 1, 2**32 + 1] + torch.randint(0, 2**32, (17,), generator=_g).tolist()  # 20
KS = [1, 19, 20]
U = 2.0 ** -52
MT_N = 624


def _offsets(sizes):
    return [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]


def _stream_pos(sizes):
    """stream word of every tensor's first draw (fks.h: numel >= 16 draws numel words, + 16 for
    a ragged tail; serial draws take 4 words per new Box-Muller pair, the second value cached)"""
    pos, cached, out = 0, False, []
    for n in sizes:
        out.append(pos)
        if n >= 16:
            pos += n + (16 if n % 16 else 0)
        else:
            for _ in range(n):
                if not cached:
                    pos += 4
                cached = not cached
    return out, pos


def _probes(sizes, dev):
    off = _offsets(sizes)
    pos, stream_len = _stream_pos(sizes)
    local = [set() for _ in sizes]
    for i, n in enumerate(sizes):
        local[i] |= {0, n - 1}
    big, ragged, tiny, irr = 0, 3, 4, 5
    n = sizes[ragged]
    local[ragged] |= {n - 16, n - 17, n - 1, 1, 8, 15, 16}
    local[FROZEN] |= set(range(sizes[FROZEN]))  # every serial element
    local[tiny] |= set(range(sizes[tiny]))
    # both sides of MT block boundaries and of plan chunk boundaries of the big tensor
    nblocks = -(-stream_len // MT_N)
    nchunks = min(nblocks, 3 * torch.cuda.get_device_properties(dev).multi_processor_count)
    for b in (1, 2, 840, 1680):
        local[big] |= {MT_N * b - 1, MT_N * b, MT_N * b - 9, MT_N * b + 8}
    for c in (1, 2, 3, nchunks // 2, nchunks // 2 + 1):
        b = nblocks * c // nchunks
        local[big] |= {MT_N * b - 1, MT_N * b}
    local[big] |= {16000 + x for x in (0, 7, 8, 15)}  # elements 0, 7, 8, 15 of a 16-block
    # the irregular run: 16-blocks on both sides of, and straddling, an MT block boundary
    e0 = (-pos[irr]) % MT_N + 20 * MT_N
    local[irr] |= {e0 - 17, e0 - 9, e0 - 8, e0 - 1, e0, e0 + 7, e0 + 8}
    out = []
    for i, s in enumerate(local):
        out += [off[i] + e for e in sorted(s) if 0 <= e < sizes[i]]
    return out


def _draw(dts, sizes, seed):
    """float64 z of one seed over the concatenation, as the reference draws it on the CPU"""
    torch.manual_seed(seed)
    z = [torch.normal(mean=0, std=1, size=(n,), dtype=DT[d]) for d, n in zip(dts, sizes)]
    return torch.cat([t.float() for t in z]).numpy().astype(np.float64)


def _dense_vec(total, seed=5):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(total, generator=g)
    big = torch.rand(total, generator=g) < 0.01
    return torch.where(big, v * 1e6, v)


@functools.lru_cache(maxsize=None)
def _specs(dtype):
    """one spec list per dtype, kept for the session (a stable plan key)"""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    return tuple(codec.ParamSpec(torch.empty(n, dtype=DT[dtype], device=dev), frozen=(i == FROZEN))
                 for i, n in enumerate(SIZES))


def _reference(dts, sizes, vec, seeds, probes, live, draw=_draw):
    v64 = vec.numpy().astype(np.float64)
    ref, sabs, zp = [], [], []
    for s in seeds:
        z = draw(dts, sizes, s)
        p = (v64 * z)[live]  # exact products
        ref.append(math.fsum(p.tolist()))
        sabs.append(float(np.abs(p).sum()))
        zp.append(z[probes].copy())
    return np.array(ref), np.array(sabs), np.array(zp)


@functools.lru_cache(maxsize=None)
def _case(dtype):
    """Computed once per dtype and shared: the dense vector, and per seed the reference
    projection, sum|v z| and the reference z at the probed elements."""
    off = _offsets(SIZES)
    live = np.ones(off[-1], bool)
    live[off[FROZEN]:off[FROZEN + 1]] = False
    vec = _dense_vec(off[-1])
    probes = np.array(_probes(SIZES, _dev()))
    ref, sabs, zp = _reference([dtype] * len(SIZES), SIZES, vec, SEEDS, probes, live)
    return {"off": off, "vec": vec, "ref": ref, "sabs": sabs, "n": int(live.sum()), "probes": probes, "zp": zp,
            "live": live}


def _f64(t):
    return t.cpu().numpy()


def _i64(t):
    return t.cpu().numpy().view(np.int64)


def _one_hot(specs, seeds, total, probes, zp, live, dev, v=float(np.float32(-3.1415927)), **kw):
    """(element, seeds that differ) of the probes whose one-hot projection is not v z"""
    from fate_llm.algo.fedkseed import codec
    vec = torch.zeros(total, dtype=torch.float32, device=dev)
    bad = []
    for pi, e in enumerate(probes):
        vec[e] = v
        got = _f64(codec.project_mt(specs, seeds, vec, **kw))
        vec[e] = 0.0
        want = np.float64(v) * zp[:len(seeds), pi] if live[e] else np.zeros(len(seeds))
        if not np.array_equal(got, want):  # bit for bit but for the sign of a zero
            bad.append((e, int((got != want).sum())))
    return bad


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "project_mt_parent.json")


def _cu_count():
    return int(torch.cuda.get_device_properties(_dev()).multi_processor_count)


def record_bits():
    """The int64 bit patterns of codec.project_mt over SIZES, the dense vector and the 20 SEEDS
    (one full and one partial pass), per dtype, and for fp32 under the libm flavour."""
    from fate_llm.algo.fedkseed import codec
    dense = _case("float32")["vec"].to(_dev())  # the vector does not depend on the dtype
    bits = {d: _i64(codec.project_mt(_specs(d), SEEDS, dense)).tolist() for d in DTYPES}
    codec.set_cpu_fp32_flavour("libm")
    try:
        bits["float32_libm"] = _i64(codec.project_mt(_specs("float32"), SEEDS, dense)).tolist()
    finally:
        codec.set_cpu_fp32_flavour(None)
    return bits


def test_bits_equal_parent_recording():
    """The summation order is part of the interface (fks.h: one fixed order): every result equals,
    bit for bit, what the recorded commit's library returned.  The order is a function of the
    plan's chunk count, which follows the device's CU count: on another device nothing is pinned."""
    with open(GOLDEN) as f:
        gold = json.load(f)
    if _cu_count() != gold["cu_count"]:
        pytest.skip(f"recorded on a device of {gold['cu_count']} CUs, this one has {_cu_count()}")
    got = record_bits()
    assert sorted(got) == sorted(gold["bits"])
    for name, want in gold["bits"].items():
        assert len(want) == len(SEEDS)
        differ = [i for i, (a, b) in enumerate(zip(got[name], want)) if a != b]
        assert not differ, f"{name}: seeds {differ} differ from commit {gold['commit']} (build {gold['build_id']})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", KS)
def test_dense_projection_within_f64_sum_bound(dtype, k):
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    got = codec.project_mt(_specs(dtype), SEEDS[:k], c["vec"].to(dev))
    assert got.dtype == torch.float64 and got.shape == (k,) and got.device.type == "cuda"
    got = _f64(got)
    err, bound = np.abs(got - c["ref"][:k]), c["n"] * U * c["sabs"][:k]
    print(f"{dtype} k={k}: max |got - ref| / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", KS)
def test_one_hot_is_exact(dtype, k):
    """Pins the element-to-word mapping and the dtype rounding of z: a dropped, doubled or
    misplaced element shows here."""
    c = _case(dtype)
    probes = c["probes"].tolist()
    zp = c["zp"]
    if k != 20:  # the full list of probes once; the other pass shapes on every fourth
        probes, zp = probes[::4], zp[:, ::4]
    assert (c["zp"][:, c["live"][c["probes"]]] != 0.0).mean() > 0.9
    bad = _one_hot(_specs(dtype), SEEDS[:k], c["off"][-1], probes, zp, c["live"], _dev())
    assert not bad, f"(element, seeds that differ): {bad}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_and_empty_tensors(dtype):
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    off = c["off"]
    specs = _specs(dtype)
    # non-zero only over the frozen tensor's range: nothing
    vec = torch.zeros(off[-1], dtype=torch.float32, device=dev)
    vec[off[FROZEN]:off[FROZEN + 1]] = 7.5
    assert np.array_equal(_i64(codec.project_mt(specs, SEEDS, vec)), np.zeros(len(SEEDS), np.int64))
    # the frozen range is never read: NaN there reaches no result
    dense = c["vec"].to(dev)
    whole = _i64(codec.project_mt(specs, SEEDS, dense))
    dense[off[FROZEN]:off[FROZEN + 1]] = float("nan")
    assert np.array_equal(_i64(codec.project_mt(specs, SEEDS, dense)), whole)
    # the list without its empty tensor: the same bits
    sp = [s for s in specs if s.tensor.numel()]
    assert np.array_equal(_i64(codec.project_mt(sp, SEEDS, dense)), whole)
    # no seeds: an empty float64 tensor
    none = codec.project_mt(specs, [], dense)
    assert none.dtype == torch.float64 and none.numel() == 0


def test_mixed_dtype_list():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    dts = ["bfloat16", "float32", "float16", "bfloat16", "float32"]
    sizes = [1 << 18, 4096, 4096, 1000, 5]
    off = _offsets(sizes)
    total = off[-1]
    probes = sorted({o + x for o, n in zip(off, sizes) for x in (0, 1, n // 2, n - 17, n - 1) if 0 <= x < n})
    vec = _dense_vec(total, seed=31)
    live = np.ones(total, bool)
    ref, sabs, zp = _reference(dts, sizes, vec, SEEDS, np.array(probes), live)
    specs = [codec.ParamSpec(torch.empty(n, dtype=DT[d], device=dev)) for d, n in zip(dts, sizes)]
    got = _f64(codec.project_mt(specs, SEEDS, vec.to(dev)))
    err, bound = np.abs(got - ref), total * U * sabs
    print(f"mixed: max |got - ref| / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all(), (err, bound)
    bad = _one_hot(specs, SEEDS, total, probes, zp, live, dev, v=float(np.float32(2.7182817)))
    assert not bad, f"(element, seeds that differ): {bad}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nshards", [2, 3])
def test_shards(dtype, nshards):
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    specs = _specs(dtype)
    k = 20
    dense = c["vec"].to(dev)
    parts = [_f64(codec.project_mt(specs, SEEDS[:k], dense, shard=r, nshards=nshards)) for r in range(nshards)]
    total = np.array([math.fsum(p[s] for p in parts) for s in range(k)])
    err, bound = np.abs(total - c["ref"][:k]), c["n"] * U * c["sabs"][:k]
    assert (err <= bound).all(), (err, bound)
    # one-hot: one shard returns the whole call's value, the others exactly +0.  The ranges are
    # stream words; the first two tensors are fast and start at word 0, so there a word is an
    # element of the concatenation and names the owner
    ranges = [codec.shard_range(specs, r, nshards, stream_mode="torch_cpu") for r in range(nshards)]
    assert ranges[0][0] == 0 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    fast_end = c["off"][2]
    edges = [e for lo, hi in ranges for e in (lo - 1, lo, hi - 1, hi) if 0 <= e < fast_end]
    assert len(edges) >= 2 * (nshards - 1), "the shard boundaries lie inside the fast tensors"
    vec = torch.zeros(c["off"][-1], dtype=torch.float32, device=dev)
    for e in sorted(set(edges + c["probes"][::9].tolist())):
        if not c["live"][e]:
            continue
        vec[e] = 1.75
        whole = _i64(codec.project_mt(specs, SEEDS[:k], vec))
        assert whole.any()
        got = [_i64(codec.project_mt(specs, SEEDS[:k], vec, shard=r, nshards=nshards)) for r in range(nshards)]
        vec[e] = 0.0
        owners = [r for r in range(nshards) if np.array_equal(got[r], whole)]
        assert len(owners) == 1, (e, owners)
        assert all(not got[r].any() for r in range(nshards) if r != owners[0]), e  # +0 bit for bit
        if e < fast_end:
            assert ranges[owners[0]][0] <= e < ranges[owners[0]][1], (e, owners, ranges)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_overwrites_and_ignores_the_address(dtype):
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    specs = _specs(dtype)
    dense = c["vec"].to(dev)
    a = _i64(codec.project_mt(specs, SEEDS, dense))
    b = _i64(codec.project_mt(specs, SEEDS, dense))
    assert np.array_equal(a, b)
    # vec at two different 8-byte aligned addresses
    buf = torch.empty(dense.numel() + 2, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[2:].copy_(dense)
    assert buf[2:].data_ptr() % 16 == 8
    assert np.array_equal(_i64(codec.project_mt(specs, SEEDS, buf[2:])), a)
    # the C call overwrites its output (here pre-filled with NaN), it does not accumulate
    L = N.load()
    batch = codec._Batch(specs, "torch_cpu", stage=False)
    seeds = np.array(SEEDS, dtype=np.uint64)
    out = torch.full((len(SEEDS),), float("nan"), dtype=torch.float64, device=dev)
    nbytes = ctypes.c_size_t(0)
    N.check(L.fks_project_mt_workspace_size(ctypes.addressof(batch.arr), batch.n, len(SEEDS), ctypes.byref(nbytes)))
    assert nbytes.value > 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(L.fks_project_mt(ctypes.addressof(batch.arr), batch.n, seeds.ctypes.data, len(SEEDS), dense.data_ptr(), 0, 1,
                             out.data_ptr(), ws.data_ptr(), nbytes.value, stream))
    assert np.array_equal(_i64(out), a)
    # ... also when the shard holds nothing (a list of empty and frozen tensors): zeroed
    out.fill_(float("nan"))
    sp0 = [codec.ParamSpec(torch.empty(0, dtype=DT[dtype], device=dev)),
           codec.ParamSpec(torch.empty(5, dtype=DT[dtype], device=dev), frozen=True)]
    b0 = codec._Batch(sp0, "torch_cpu", stage=False)
    v0 = torch.ones(5, dtype=torch.float32, device=dev)
    N.check(L.fks_project_mt(ctypes.addressof(b0.arr), b0.n, seeds.ctypes.data, len(SEEDS), v0.data_ptr(), 0, 1,
                             out.data_ptr(), None, 0, stream))
    assert np.array_equal(_i64(out), np.zeros(len(SEEDS), np.int64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_adjoint_of_delta_accumulate(dtype):
    """<Z c, v> = <c, Z^T v>.  delta_accumulate rounds every element's K fmas to f32 -- the
    only inexact step: |delta_e - sum_s f32(c_s) z_s(e)| <= K 2^-24 sum_s |f32(c_s) z_s(e)| --
    and the projection errs by the dense bound per seed (test_gpu_project.py's bound)."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    sizes = [4096, 3, 1000, 7]
    K = 5
    seeds = SEEDS[3:3 + K]
    g = torch.Generator().manual_seed(9)
    coefs = (torch.randn(K, generator=g, dtype=torch.float64) * 3).tolist()
    c32 = np.array(coefs, dtype=np.float32).astype(np.float64)
    specs = [codec.ParamSpec(torch.empty(n, dtype=DT[dtype], device=dev)) for n in sizes]
    total = sum(sizes)
    v = _dense_vec(total, seed=13)
    v64 = v.numpy().astype(np.float64)
    delta = torch.zeros(total, dtype=torch.float32, device=dev)
    codec.delta_accumulate(specs, seeds, coefs, delta, stream_mode="torch_cpu")
    proj = _f64(codec.project_mt(specs, seeds, v.to(dev)))
    lhs = math.fsum((delta.cpu().numpy().astype(np.float64) * v64).tolist())  # exact products
    rhs = math.fsum((c32 * proj).tolist())
    z = np.stack([_draw([dtype] * len(sizes), sizes, s) for s in seeds])  # [K, total]
    bound = K * 2.0 ** -24 * float((np.abs(v64) * (np.abs(c32)[:, None] * np.abs(z)).sum(0)).sum())
    bound += float((np.abs(c32) * total * U * np.abs(v64 * z).sum(1)).sum())
    print(f"{dtype}: |lhs - rhs| / bound = {abs(lhs - rhs) / bound:.3e}")
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_vector(dtype):
    from fate_llm.algo.fedkseed import codec
    c = _case(dtype)
    dev = _dev()
    specs = _specs(dtype)
    k = 20
    # a fast element and an irregular one whose reference z is non-zero for every seed
    fast = next(i for i, e in enumerate(c["probes"].tolist()) if e > MT_N and (c["zp"][:k, i] != 0.0).all())
    irr = next(i for i, e in enumerate(c["probes"].tolist()) if e > c["off"][5] and (c["zp"][:k, i] != 0.0).all())
    for pi in (fast, irr):
        e = int(c["probes"][pi])
        dense = c["vec"].to(dev)
        dense[e] = float("nan")
        assert np.isnan(_f64(codec.project_mt(specs, SEEDS[:k], dense))).all()
        for inf in (float("inf"), float("-inf")):
            vec = torch.zeros(c["off"][-1], dtype=torch.float32, device=dev)
            vec[e] = inf
            got = _f64(codec.project_mt(specs, SEEDS[:k], vec))
            assert np.array_equal(got, np.float64(inf) * np.sign(c["zp"][:k, pi]))


def test_libm_flavour():
    """fp32 under codec.set_cpu_fp32_flavour("libm"): the reference z is what codec.normal_ writes
    under that flavour (the existing suite pins that draw to the reference's)."""
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    c = _case("float32")
    specs = _specs("float32")
    tensors = [torch.empty(n, dtype=torch.float32, device=dev) for n in SIZES]

    def draw(dts, sizes, seed):
        codec.normal_(tensors, seed, stream_mode="torch_cpu", leave_generator=False)
        return torch.cat(tensors).cpu().numpy().astype(np.float64)

    dense = c["vec"].to(dev)
    default = _i64(codec.project_mt(specs, SEEDS, dense))
    probes = c["probes"][::3]
    codec.set_cpu_fp32_flavour("libm")
    try:
        assert codec.cpu_fp32_flavour() == "libm"
        ref, sabs, zp = _reference(None, None, c["vec"], SEEDS, probes, c["live"], draw=draw)
        got = codec.project_mt(specs, SEEDS, dense)
        bad = _one_hot(specs, SEEDS, c["off"][-1], probes.tolist(), zp, c["live"], dev)
    finally:
        codec.set_cpu_fp32_flavour(None)
    err, bound = np.abs(_f64(got) - ref), c["n"] * U * sabs
    print(f"libm: max |got - ref| / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all(), (err, bound)
    assert not bad, f"(element, seeds that differ): {bad}"
    if codec.cpu_fp32_flavour() != "libm":  # the two flavours' z differ: so do their projections
        assert (_i64(got) != default).any()


def test_zo_utils_seed_projections_and_fit():
    from fate_llm.algo.fedkseed import zo_utils
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    shapes, dts, rg = [(5000,), (1000, 3), (300,)], ["bfloat16", "float32", "bfloat16"], [True, True, False]
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.02).to(DT[d]).to(dev), requires_grad=r)
              for s, d, r in zip(shapes, dts, rg)]
    for p in params[:2]:
        p.grad = torch.randn(p.shape, generator=g).to(p.dtype).to(dev)
    groups = [{"params": params[:1], "lr": 1e-3, "weight_decay": 0.0}, {"params": params[1:], "lr": 1e-3, "weight_decay": 0.0}]
    seeds = SEEDS[:7]
    # explicit reference: every parameter draws in its own dtype on the CPU, the frozen one is dropped
    ref, sabs = [], []
    for s in seeds:
        torch.manual_seed(s)
        z = [torch.normal(mean=0, std=1, size=p.shape, dtype=p.dtype) for p in params]
        prod = np.concatenate([(p.grad.float().cpu().numpy().astype(np.float64) *
                                t.float().numpy().astype(np.float64)).reshape(-1)
                               for p, t in zip(params[:2], z[:2])])
        ref.append(math.fsum(prod.tolist()))
        sabs.append(float(np.abs(prod).sum()))
    n = sum(p.numel() for p in params[:2])
    bound = n * U * np.array(sabs)
    torch.manual_seed(123)
    torch.rand(3)
    torch.rand(3, device=dev)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    got = zo_utils.seed_projections(groups, seeds, stream_mode="torch_cpu")
    fit = zo_utils.fit_seed_scalars(groups, seeds, [p.grad for p in params[:2]] + [None], stream_mode="torch_cpu")
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)
    assert got.dtype == torch.float64 and got.device.type == "cuda"
    assert (np.abs(_f64(got) - np.array(ref)) <= bound).all()
    assert torch.equal(fit, got / float(n))
    assert (np.abs(_f64(fit) - np.array(ref) / n) <= bound / n * (1 + 2.0 ** -50)).all()
    # the torch_rocm route is untouched and draws another stream
    rocm = zo_utils.seed_projections(groups, seeds, stream_mode="torch_rocm")
    assert not torch.equal(rocm, got)
    # the in-place forms stay torch_rocm only
    with pytest.raises(NotImplementedError, match="torch_cpu"):
        zo_utils.seed_projections_multi(groups, seeds, stream_mode="torch_cpu")
