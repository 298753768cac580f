"""fks_expand_multi (codec.expand_multi, torch_rocm stream) against an exact reference that shares
nothing with the kernels: torch's own draws on the same GPU -- after torch.manual_seed(s),
torch.normal(0, 1, (n,), device, dtype) per tensor in list order, frozen ones drawn and dropped --
widened to f32, folded by tests/exact_f32.py's chain32 (acc = RN_f32(f32(c_s) z_s + acc) from +0,
every fma correctly rounded out of float64 operations), then fma32(f32(beta), widen(old), acc)
where beta != 0, then torch's .to(out dtype).  Every comparison is bitwise on integer views over
every live element of every output; a NaN matches any NaN only in the overflow test.  Outputs lie
inside buffers with guard elements on both sides; guards, frozen and empty tensors' buffers keep
their sentinel.

Lists: A, ten small tensors of three dtypes, the first and last frozen, one empty -- tensors of at
most 256 elements are half a wave's groups, so waves span two or three tensors of different dtype
(the per-lane table lookup, the divergent dtype switch, the Philox offset across element sizes);
B, 600 tensors of 1 .. 41 elements, three dtypes -- more than the 512 entries the kernel copies to
LDS, so the table is read from device memory; C, tests/test_gpu_project.py's list (a capped
stride, a ragged last row, j = 1 items), one dtype per case; SUB, (4096, 65536), bf16 and f32; and
W, (1000, 3 S + 4104) with S the capped stride: the smallest tensor in which groups store whole
16-byte runs (those at idx0 <= 4096) next to groups that store per element -- no tensor of A, B
or SUB is long enough for the former (four runs of a group must lie inside the tensor)."""
import functools

import pytest
import torch

from exact_f32 import chain32, f32, fma32
from test_gpu_expand import SUB, _coefs, _same, _seeds
from test_gpu_parity import _dev
from test_gpu_project import DT, FROZEN, SEEDS, _offsets, _sizes, _stride

pytestmark = pytest.mark.gpu

MODE = "torch_rocm"
CYC = ["bfloat16", "float32", "float16"]
ROWS = ["float32", "bfloat16", "float16"]  # output dtypes over the rows of a call
GUARD = -7.0
K = 33


class _List:
    def __init__(self, sizes, dts, frozen=()):
        self.sizes, self.dts, self.frozen = list(sizes), list(dts), frozenset(frozen)
        self.off = _offsets(self.sizes)
        self.live = [i for i, n in enumerate(self.sizes) if n and i not in self.frozen]

    def specs(self, dev, dts=None):
        from fate_llm.algo.fedkseed import codec
        return [codec.ParamSpec(torch.empty(n, dtype=DT[d], device=dev), frozen=(i in self.frozen))
                for i, (n, d) in enumerate(zip(self.sizes, dts or self.dts))]


@functools.lru_cache(maxsize=None)
def _list(name):
    if name == "A":
        sizes = [5, 256, 1000, 0, 100, 8, 200, 256, 4096, 9]
        return _List(sizes, ["float32"] + [CYC[i % 3] for i in range(8)] + ["float16"], frozen=(0, 9))
    if name == "B":
        return _List([(7 * i) % 41 + 1 for i in range(600)], [CYC[i % 3] for i in range(600)])
    if name == "SUB":
        return _List(SUB, ["bfloat16", "float32"])
    if name == "W":
        return _List([1000, 3 * _stride(10 ** 9) + 4104], ["float16", "bfloat16"])
    return _List(_sizes(), [name[2:]] * len(_sizes()), frozen=(FROZEN,))  # "C:<dtype>"


def _draws(L, dts, seed, dev):
    """torch's draws of one seed over the concatenation (frozen tensors too), widened to f32"""
    torch.manual_seed(seed)
    return torch.cat([torch.normal(mean=0, std=1, size=(n,), device=dev, dtype=DT[d]).float()
                      for n, d in zip(L.sizes, dts)])


@functools.lru_cache(maxsize=None)
def _zs(name):
    """the 33 seeds' draws of a small list, drawn once and shared (never written to)"""
    L = _list(name)
    return [_draws(L, L.dts, s, _dev()) for s in SEEDS[:K]]


def _sums(name, rows, dev, k=K):
    """the exact chains: per coefficient row the f32 sums over the concatenation"""
    L = _list(name)
    if k == 0:
        return [torch.zeros(L.off[-1], dtype=torch.float32, device=dev) for _ in rows]
    if name.startswith("C:"):  # 2.9 M elements: one row, the draws not kept
        assert len(rows) == 1
        return [chain32(rows[0], (_draws(L, L.dts, s, dev) for s in SEEDS[:k]))]
    return [chain32(r, _zs(name)[:k]) for r in rows]


def _old(n, name, seed):
    """old contents: normals of spread 3 with -0.0 and subnormals of the dtype among them"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3
    tiny = {"float32": 1e-40, "bfloat16": 2.0 ** -130, "float16": 2.0 ** -20}[name]
    x[3::11] = tiny
    x[5::13] = -3 * tiny
    x[::7] = -0.0
    return x.to(DT[name])


def _row_names(L, names):
    return [names] * len(L.sizes) if isinstance(names, str) else list(names)


def _buffers(L, names, beta, offset, dev, seed):
    """One output row: per tensor a buffer of GUARD with the output inside it, 16-byte aligned plus
    ``offset`` elements, a guard of at least one element on both sides.  Live outputs hold NaN where
    beta == 0 (never read), else _old; returns (buffers, views, olds)."""
    bufs, views, olds = [], [], []
    for i, (n, d) in enumerate(zip(L.sizes, _row_names(L, names))):
        pad = 16 // DT[d].itemsize + offset
        buf = torch.full((pad + n + 1,), GUARD, dtype=DT[d], device=dev)
        v = buf[pad:pad + n]
        old = None
        if i in L.live:
            assert (v.data_ptr() % 16 == 0) == (offset == 0)
            if beta == 0:
                v.fill_(float("nan"))
            else:
                old = _old(n, d, seed + i).to(dev)
                v.copy_(old)
        bufs.append(buf)
        views.append(v)
        olds.append(old)
    return bufs, views, olds


def _check_row(L, names, beta, acc, bufs, views, olds, what, nan_ok=False):
    names = _row_names(L, names)
    guard = torch.tensor(GUARD)
    for i, n in enumerate(L.sizes):
        pad = bufs[i].numel() - n - 1
        g = guard.to(bufs[i].dtype).to(bufs[i].device)
        if i not in L.live:
            assert _same(bufs[i], g.expand_as(bufs[i])), (what, i, "a frozen or empty tensor's buffer was written")
            continue
        assert _same(bufs[i][:pad], g.expand(pad)) and _same(bufs[i][pad + n:], g.expand(1)), (what, i, "guards")
        a = acc[L.off[i]:L.off[i + 1]]
        want = (a if beta == 0 else fma32(f32(beta), olds[i].float(), a)).to(DT[names[i]])
        if not _same(views[i], want, nan_ok=nan_ok):
            bad = (views[i].float() != want.float()) | (torch.signbit(views[i].float()) != torch.signbit(want.float()))
            e = int(torch.nonzero(bad)[0])
            raise AssertionError(f"{what}: tensor {i} ({n} x {names[i]}, beta {beta}): {int(bad.sum())} elements differ, "
                                 f"first at {e}: got {float(views[i][e])!r}, want {float(want[e])!r}")


def _run(name, rows, row_names, betas=None, offset=0, k=K, spec_dts=None, nan_ok=False, check=True):
    """One expand_multi call on fresh buffers, synchronized, every row checked against the exact
    reference; returns the views per row."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _list(name)
    M = len(rows)
    bs = [0.0] * M if betas is None else list(betas)
    made = [_buffers(L, row_names[m], bs[m], offset, dev, 500 + 100 * m) for m in range(M)]
    codec.expand_multi(L.specs(dev, spec_dts), SEEDS[:k], rows, [v for _, v, _ in made],
                       betas=betas, stream_mode=MODE)
    torch.cuda.synchronize()
    if check:
        accs = _sums(name, rows, dev, k)
        for m in range(M):
            _check_row(L, row_names[m], bs[m], accs[m], *made[m], what=f"list {name}, row {m}", nan_ok=nan_ok)
    return [v for _, v, _ in made]


# ---- 0. the reference's arithmetic on the device is the host's
def test_fma32_on_the_device_equals_the_host():
    """tests/test_exact_f32.py proves fma32 on the host; here the same float64 operations run on
    the GPU: ties with a residual, subnormal results (an f64 -> f32 conversion that flushed would
    show), overflow around the midpoint below 2^128, zeros of either sign."""
    dev = _dev()
    j = torch.arange(512, dtype=torch.float64)
    c = [(1.0 + j * 2.0 ** -23), (1.0 + j * 2.0 ** -23), (2 ** 22 + j) * 2.0 ** -149, (2 ** 22 + j) * 2.0 ** -149]
    a = [torch.full((512,), 2.0 ** -12 * (1 + 2.0 ** -18))] * 2 + [torch.full((512,), 2.0 ** -75 * (1 + 2.0 ** -18))] * 2
    b = [torch.full((512,), s * 2.0 ** e * (1 - 2.0 ** -18)) for s, e in ((1, -12), (-1, -12), (1, -75), (-1, -75))]
    g = torch.Generator().manual_seed(6)
    for scale in (1.0, 2.0 ** -70, 2e19):
        a.append(torch.randn(2000, generator=g) * scale)
        b.append(torch.randn(2000, generator=g) * scale)
        c.append(torch.randn(2000, generator=g) * scale * scale)
    t = 2.0 ** -100
    a.append(torch.tensor([18631.0, 18631.0, 18631.0, -18631.0, 0.0, -0.0, -0.0, 1.5]))
    b.append(torch.tensor([1801.0 * 2.0 ** 103] * 4 + [1.5, 1.5, 1.5, -1.5]))
    c.append(torch.tensor([0.0, t, -t, t, -0.0, -0.0, 0.0, 2.25]))
    a, b, c = (torch.cat([x.double() for x in v]).float() for v in (a, b, c))
    host = fma32(a, b, c)
    assert int(((host != 0) & (host.abs() < 2.0 ** -126)).sum()) > 1000 and bool(torch.isinf(host).any())
    assert _same(fma32(a.to(dev), b.to(dev), c.to(dev)).cpu(), host)


# ---- 1. the chain
@pytest.mark.parametrize("dtype", CYC)
def test_chain_of_33_seeds_is_exact(dtype):
    """K > 1 against something that is not our own kernel: list C, f32 outputs, beta 0."""
    _run("C:" + dtype, [_coefs(K, 50)], ["float32"])


# ---- 2. several dtypes in one wave
def test_mixed_dtypes_in_one_wave():
    L = _list("A")
    names = [[ROWS[(i + m) % 3] for i in range(len(L.sizes))] for m in range(2)]
    rows = [_coefs(K, 51), _coefs(K, 52)]
    got = _run("A", rows, names)
    # teeth: with every spec bf16 the draws, and so the result, differ
    other = _run("A", rows, names, spec_dts=["bfloat16"] * len(L.sizes), check=False)
    assert any(not _same(got[0][i], other[0][i]) for i in L.live if L.dts[i] != "bfloat16")


# ---- 3. a table longer than the LDS copy
@pytest.mark.parametrize("M", [1, 4])
def test_table_of_600_entries(M):
    """M = 1: beta 0; M = 4 (a full batch): beta 1 over random old values.  f32 and bf16 outputs
    alternate over the tensors, the other way round in odd rows."""
    L = _list("B")
    names = [[("float32", "bfloat16")[(i + m) % 2] for i in range(len(L.sizes))] for m in range(M)]
    _run("B", [_coefs(K, 53 + m) for m in range(M)], names, betas=None if M == 1 else [1.0] * M)


# ---- 4. betas across the batches of four outputs
BETAS = [0.3, 0.0, -1.7, -0.0, 1e-3, 1.0]


@pytest.mark.parametrize("name", ["A", "SUB", "W"])
@pytest.mark.parametrize("offset", [0, 1])
def test_betas_across_the_batch(name, offset):
    """Six outputs are a batch of four and one of two: rows 4 and 5 take their beta and their
    read-old bit from betas[4 + m].  Betas that are no powers of two make fma(beta, old, acc) differ
    from a product and a sum in about a quarter of the elements.  Rows 1 and 3 (beta 0.0 and -0.0)
    hold NaN and are never read.  Lists A and SUB store per element; W (beyond the issue's two
    lists) has the groups that store whole 16-byte runs when offset is 0."""
    rows = [_coefs(K, 60 + m) for m in range(6)]
    names = [ROWS[m % 3] for m in range(6)]
    got = _run(name, rows, names, betas=BETAS, offset=offset)
    for m in (1, 3):
        for i in _list(name).live:
            assert bool(torch.isfinite(got[m][i]).all()), (m, i)


# ---- 5. no seeds
def test_no_seeds():
    """k == 0: +0 (all bits zero) where beta == 0, cast(fma(beta, old, +0)) elsewhere: an old -0.0
    becomes +0."""
    L = _list("A")
    got = _run("A", [[], [], []], ROWS, betas=[0.0, 0.5, 0.0], k=0)
    for m in (0, 2):
        for i in L.live:
            assert not bool(got[m][i].view(torch.int32 if m == 0 else torch.int16).any()), (m, i)
    for i in L.live:  # _old puts -0.0 at every seventh element
        assert not bool(torch.signbit(got[1][i][::7].float()).any()), i


# ---- 6. f32 subnormals
def test_subnormal_coefficients_and_sums():
    """Coefficients of about 2^-140 are f32 subnormals, and so is every sum: a kernel that flushed
    either would differ from this reference (not from delta_accumulate, which would flush alike)."""
    dev = _dev()
    rows = [_coefs(K, 70, 2.0 ** -140), _coefs(K, 71, 2.0 ** -140)]
    ref = _sums("SUB", rows, dev)[0]
    sub = (ref != 0) & (ref.abs() < 2.0 ** -126)
    assert int(sub.sum()) > ref.numel() // 2  # the reference holds non-zero subnormal f32 values
    _run("SUB", rows, ["float32", "bfloat16"])


# ---- 7. overflow
def test_overflowing_coefficients():
    """Coefficients of about 3e38: those beyond f32's range are inf as f32, sums overflow to either
    inf, and inf - inf is NaN (whose payload is not part of the contract)."""
    dev = _dev()
    rows = [_coefs(K, 72, 3e38), _coefs(K, 73, 3e38)]
    ref = _sums("SUB", rows, dev)[0]
    assert bool((ref == float("inf")).any()) and bool((ref == float("-inf")).any()) and bool(torch.isnan(ref).any())
    _run("SUB", rows, ["float32", "float16"], nan_ok=True)


# ---- 8. stream order
def test_two_calls_in_flight():
    """Call 1 (4096 seeds, one output) and, with no synchronize in between, call 2 (33 seeds, two
    outputs: another workspace layout) equal the same calls made apart, and call 2 the exact
    reference.  Each call stages its table -- output pieces, seeds, coefficients -- in a host vector
    that the next call overwrites, and hands its workspace back to torch's allocator at once: a
    staging buffer reused while a copy from it is pending, or a workspace handed to call 2 before
    call 1 has read it, would show here as wrong values in X.  That no such race exists is not
    proven: the copy may simply have won."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _list("SUB")
    specs = L.specs(dev)
    a, b = _coefs(4096, 74), [_coefs(K, 75), _coefs(K, 76)]
    names = ["float32", "bfloat16"]

    def fresh():
        return ([torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in L.sizes],
                [[torch.full((n,), float("nan"), dtype=DT[d], device=dev) for n in L.sizes] for d in names])

    X1, Y1 = fresh()
    codec.expand_multi(specs, _seeds(4096), [a], [X1], stream_mode=MODE)
    torch.cuda.synchronize()
    codec.expand_multi(specs, SEEDS[:K], b, Y1, stream_mode=MODE)
    torch.cuda.synchronize()
    X2, Y2 = fresh()
    torch.cuda.synchronize()
    codec.expand_multi(specs, _seeds(4096), [a], [X2], stream_mode=MODE)
    codec.expand_multi(specs, SEEDS[:K], b, Y2, stream_mode=MODE)
    torch.cuda.synchronize()
    accs = _sums("SUB", b, dev)
    for i in L.live:
        assert bool(torch.isfinite(X1[i]).all())
        assert _same(X2[i], X1[i]), i
        for m in range(2):
            assert _same(Y2[m][i], Y1[m][i]), (m, i)
            assert _same(Y2[m][i], accs[m][L.off[i]:L.off[i + 1]].to(DT[names[m]])), (m, i)


# ---- 9. a side stream
def test_the_call_runs_on_the_current_stream():
    """The outputs hold NaN; on a side stream they are filled with 2.0 and expanded with beta 1.0:
    fma(1, 2.0, acc) everywhere only if the call ran on the stream it was given, after the fill."""
    from fate_llm.algo.fedkseed import codec
    dev, L = _dev(), _list("SUB")
    rows = [_coefs(K, 77), _coefs(K, 78)]
    names = ["float32", "bfloat16"]
    outs = [[torch.full((n,), float("nan"), dtype=DT[d], device=dev) for n in L.sizes] for d in names]
    accs = _sums("SUB", rows, dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for o in outs:
            for t in o:
                t.fill_(2.0)
        codec.expand_multi(L.specs(dev), SEEDS[:K], rows, outs, betas=[1.0, 1.0], stream_mode=MODE)
    side.synchronize()
    for m in range(2):
        for i in L.live:
            a = accs[m][L.off[i]:L.off[i + 1]]
            assert _same(outs[m][i], fma32(1.0, torch.full_like(a, 2.0), a).to(DT[names[m]])), (m, i)
