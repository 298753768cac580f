"""An independent reference of the seed-sharded delta operations (fks_delta_accumulate,
fks_delta_apply), and the tensor lists and inputs the delta tests share.  A plain module: the
tests import it (tests/test_delta_ref_host.py ties it to the oracle on the CPU; the
tests/test_gpu_delta_*.py files compare the kernels with it).

The reference shares no arithmetic with the kernels or with oracle/fks_oracle.c's fko_delta_*:
the z values are the oracle generator's draws (O.Generator(seed).normal per tensor in list
order, the part pinned to the reference's golden vectors by tests/test_oracle_golden.py) or
torch's own draws on the device (torch_rocm), and every fma is tests/exact_f32.py's fma32, a
correctly rounded f32 fma made of float64 torch operations.

  accumulate_ref       delta = fma32(f32(c_s), z_s, delta) per seed in order (MT19937 stream)
  accumulate_ref_rocm  the same over torch.normal(0, 1, (n,), device, dtype) after manual_seed(s)
  apply_ref            p = dtype(fma32(f32(decay), f32(p), -delta))

Frozen tensors are drawn and dropped (their range of delta keeps its bits), empty ones draw
nothing."""
import functools

import numpy as np
import torch

from exact_f32 import f32, fma32
from oracle import fks_oracle as O

DTC = {"float32": O.F32, "bfloat16": O.BF16, "float16": O.F16}
TD = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}

GUARD = -7.0  # the sentinel round guarded buffers
NGUARD = 16   # guard elements on each side (at least)


def offsets(sizes):
    return [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]


def bits32(a):
    """uint32 view of an f32 numpy array or torch tensor"""
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _z_f32(bits: np.ndarray, dtype: str) -> torch.Tensor:
    """the oracle generator's stored bits widened to f32 (exact)"""
    if dtype == "float32":
        return torch.from_numpy(bits.copy())
    if dtype == "bfloat16":
        return torch.from_numpy((bits.astype(np.uint32) << 16).view(np.float32))
    return torch.from_numpy(bits.view(np.float16).astype(np.float32))


def draws_mt(sizes, dtypes, seed) -> torch.Tensor:
    """One seed's MT19937-stream draws over the concatenation (frozen tensors included), as f32."""
    gen = O.Generator(seed)
    return torch.cat([_z_f32(gen.normal(n, DTC[d]), d) for n, d in zip(sizes, dtypes) if n] or [torch.zeros(0)])


def draws_rocm(sizes, dtypes, seed, device) -> torch.Tensor:
    """One seed's torch_rocm draws over the concatenation: torch's own, on the device."""
    torch.manual_seed(seed)
    return torch.cat([torch.normal(mean=0, std=1, size=(n,), device=device, dtype=TD[d]).float()
                      for n, d in zip(sizes, dtypes)])


def _fold(draw, sizes, frozen, seeds, coefs, delta0, device):
    acc = torch.as_tensor(delta0, dtype=torch.float32).clone().to(device if device is not None else "cpu")
    off = offsets(sizes)
    assert acc.numel() == off[-1]
    live = torch.zeros(off[-1], dtype=torch.bool, device=acc.device)
    for i, n in enumerate(sizes):
        if n and not (frozen and frozen[i]):
            live[off[i]:off[i + 1]] = True
    for s, c in zip(seeds, coefs):
        z = draw(s).to(acc.device)
        acc = torch.where(live, fma32(torch.tensor(f32(c), device=acc.device), z, acc), acc)
    return acc


def accumulate_ref(sizes, dtypes, frozen, seeds, coefs, delta0, device=None) -> torch.Tensor:
    """The delta buffer after fks_delta_accumulate on the MT19937 stream; ``device``: where the
    float64 operations of fma32 run (the draws are the oracle generator's either way)."""
    return _fold(lambda s: draws_mt(sizes, dtypes, s), sizes, frozen, seeds, coefs, delta0, device)


def accumulate_ref_rocm(sizes, dtypes, frozen, seeds, coefs, delta0, device) -> torch.Tensor:
    """The delta buffer after fks_delta_accumulate on the torch_rocm stream."""
    return _fold(lambda s: draws_rocm(sizes, dtypes, s, device), sizes, frozen, seeds, coefs, delta0, device)


def apply_ref(p: torch.Tensor, dtype: str, delta: torch.Tensor, decay: float) -> torch.Tensor:
    """p after fks_delta_apply: one correctly rounded f32 fma, then torch's rounding to the dtype."""
    assert p.dtype == TD[dtype]
    return fma32(f32(decay), p.float(), -delta.float()).to(TD[dtype])


def oracle_accumulate(sizes, dtypes, frozen, seeds, coefs, delta0) -> np.ndarray:
    """O.delta_accumulate (oracle/fks_oracle.c's fmaf loop) on a copy of delta0."""
    arrays = [np.zeros(n, O.NP_STORAGE[DTC[d]]) for n, d in zip(sizes, dtypes)]
    out = np.ascontiguousarray(torch.as_tensor(delta0).numpy() if torch.is_tensor(delta0) else delta0,
                               dtype=np.float32).copy()
    O.delta_accumulate(arrays, [DTC[d] for d in dtypes], seeds, coefs, out,
                       frozen=[int(bool(f)) for f in frozen] if frozen else None)
    return out


# ---------------------------------------------------------------- lists
class DList:
    def __init__(self, sizes, dtypes, frozen=()):
        self.sizes = list(sizes)
        self.dtypes = [dtypes] * len(self.sizes) if isinstance(dtypes, str) else list(dtypes)
        self.frozen = [i in frozen for i in range(len(self.sizes))]
        self.off = offsets(self.sizes)
        self.total = self.off[-1]

    def specs(self, dev):
        """zero parameters on the device (the delta calls read sizes, dtypes and flags only)"""
        from fate_llm.algo.fedkseed import codec
        return [codec.ParamSpec(torch.zeros(n, dtype=TD[d], device=dev), frozen=f)
                for n, d, f in zip(self.sizes, self.dtypes, self.frozen)]


# the task-path shapes of tests/test_gpu_slice_task_path.py: 104,293 elements (odd); the ragged
# sixth tensor leaves the last one at an odd offset and stream phase 5 (irregular kernel)
_A = [4096 * 3, 16, 48, 2 ** 16, 624 * 16 + 32, 4096 * 3 + 5, 4096]
_M_SIZES = [4096, 1000, 3, 7, 624 * 5, 16, 4097, 2048, 19, 65536, 5, 48, 1]
_M_DTYPES = ["bfloat16", "float32", "float16", "bfloat16", "float32", "bfloat16", "float16", "bfloat16", "float32",
             "bfloat16", "bfloat16", "float32", "float16"]


@functools.lru_cache(maxsize=None)
def dlist(name) -> DList:
    if name == "A":
        return DList(_A, "bfloat16")
    if name == "A3":  # A': three serial draws first put every later tensor at stream phase 8
        return DList([3] + _A, "bfloat16")
    if name == "A7":  # seven serial draws are 16 words: the phase stays 0 and every offset turns odd
        return DList([7] + _A, "bfloat16")
    if name == "PAR":  # 7 and 9 serial draws take 16 words each: the phase stays 0, the parity flips and flips back
        return DList([4096, 7, 2 ** 16, 9, 4096 * 3, 48], "bfloat16")
    if name == "PATH":  # no irregular part: multiples of 16 at even offsets
        return DList([4096 * 3, 2 ** 16, 624 * 16 + 32, 16, 48], "bfloat16")
    if name == "BLOCKS":  # many tasks per wave, a partial last task, a segment that begins inside a task
        return DList([1 << 20, 624 * 48 + 32], "bfloat16")
    if name == "M":  # three kernels in one buffer; tensor 4 frozen, an empty tensor at position 6
        sizes, dts = list(_M_SIZES), list(_M_DTYPES)
        sizes.insert(6, 0)
        dts.insert(6, "float32")
        return DList(sizes, dts, frozen=(4,))
    if name == "MF":  # M behind an f32 fast tensor (M's own f32 tensors are ragged, frozen, tiny or off phase)
        m = dlist("M")
        return DList([4096] + m.sizes, ["float32"] + m.dtypes, frozen=(5,))
    if name == "EDGE":
        return DList([65536, 65536], ["bfloat16", "float32"])
    raise KeyError(name)


def seeds_coefs(k, seed=11, scale=1e-5):
    g = torch.Generator().manual_seed(seed)
    seeds = torch.randint(0, 2 ** 32, (k,), generator=g).tolist()
    vals = (torch.randn(k, generator=g, dtype=torch.float64) * 20).tolist()
    return seeds, [scale * v for v in vals]


def prefill(total, seed=3) -> np.ndarray:
    """live values to accumulate into: N(0, 1) as f32"""
    return torch.randn(total, generator=torch.Generator().manual_seed(seed)).numpy().copy()


def guarded(delta0, dev, shift=0):
    """(buffer, view): delta0 on the device inside a buffer of GUARD, NGUARD + shift elements
    before it and NGUARD behind.  torch's allocations are 256-byte aligned, so the view's address
    is 4 * shift modulo 16."""
    d0 = torch.as_tensor(delta0, dtype=torch.float32)
    buf = torch.full((NGUARD + shift + d0.numel() + NGUARD,), GUARD, dtype=torch.float32, device=dev)
    view = buf[NGUARD + shift:NGUARD + shift + d0.numel()]
    view.copy_(d0)
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return buf, view


def guards_intact(buf, view) -> bool:
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    g = np.float32(GUARD).view(np.uint32)
    b = bits32(buf)
    return bool((b[:lo] == g).all() and (b[lo + view.numel():] == g).all()) and lo >= NGUARD


# ---------------------------------------------------------------- edge values of the accumulate
EDGE_K = 40
PLANTED = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-39, 3e38]
EDGE_CASES = ["edge", "overflow", "subnormal"]


def edge_inputs(case):
    """(seeds, coefs, delta0) for list EDGE, K = 40 (the slice kernel on the bf16 tensor, three
    19-seed passes on the f32 one).  Every case plants PLANTED at the head of each tensor's range
    and runs of -0 and +0 further on, and has the coefficients 0.0, -0.0, 1e-42 (an f32 subnormal)
    and -1e-45 (rounds to the smallest subnormal, -2^-149) among the others.
      edge:       ordinary coefficients over N(0, 1) values;
      overflow:   the same, the last coefficient 1e39 (inf as f32: last, so that the buffer ends
                  +-inf and not NaN);
      subnormal:  coefficients of about 2^-139 over subnormal values and zeros of both signs:
                  every sum stays in the f32 subnormal range."""
    L = dlist("EDGE")
    seeds, coefs = seeds_coefs(EDGE_K, seed=31, scale=1e-4)
    d = prefill(L.total, seed=32)
    if case == "subnormal":
        coefs = [c * 2.0 ** -128 for c in coefs]
        d = (d.astype(np.float64) * 1e-40).astype(np.float32)
        d[::7] = -0.0
        d[3::11] = 0.0
    for pos, c in ((3, 0.0), (11, -0.0), (22, 1e-42), (30, -1e-45)):
        coefs[pos] = c
    if case == "overflow":
        coefs[-1] = 1e39
    for o in L.off[:-1]:
        d[o:o + 8] = np.array(PLANTED, dtype=np.float32)
        d[o + 5000:o + 5016] = -0.0
        d[o + 7000:o + 7016] = 0.0
    return seeds, coefs, d


def edge_expected_nan(case, delta0, z_last) -> np.ndarray:
    """Where the result must be NaN, from the inputs alone: a planted NaN stays; finite terms leave
    a planted infinity as it is; in the overflow case the last term is inf * z: NaN where z is
    exactly 0, and NaN where a planted infinity meets the opposite one."""
    d = np.asarray(delta0, dtype=np.float32)
    nan = np.isnan(d)
    if case == "overflow":
        z = z_last.detach().cpu().numpy()
        nan = nan | (z == 0) | (np.isinf(d) & (np.signbit(d) != np.signbit(z)))
    return nan


def check_edge_reference(case, ref, delta0, z_last):
    """The conditions the reference alone must meet, so that 'NaN matches any NaN' hides nothing
    and the subnormal case says something about flushing."""
    r = ref.detach().cpu().numpy()
    want = edge_expected_nan(case, delta0, z_last)
    assert np.array_equal(np.isnan(r), want), (case, int(np.isnan(r).sum()), int(want.sum()))
    assert 0 < want.sum() < r.size // 100
    if case == "overflow":
        assert np.isinf(r).sum() + want.sum() == r.size  # the buffer ends +-inf (or NaN), both signs
        assert (r == np.inf).any() and (r == -np.inf).any()
    if case == "subnormal":
        sub = (r != 0) & (np.abs(r) < np.float32(2.0 ** -126))
        assert int(sub.sum()) >= 1000, int(sub.sum())
    return int(want.sum())


# ---------------------------------------------------------------- inputs of the apply
APPLY_SIZES = [4099, 4096, 7, 1000]
APPLY_DECAYS = [1.0, 0.999959, 1 - 1e-9, 0.0, -0.0]
BAND = (1000, 3000)  # ties in the tensors that reach it
P_EDGE = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 6e4, -6e4, 1e-7]
D_EDGE = [0.0, 0.0, 1.0, float("-inf"), 0.0, -6e3, 6e3, 1e-7, float("nan"), float("inf"), -0.0, 1e-45]
_MANT = {"float32": 23, "bfloat16": 7, "float16": 10}
_EMIN = {"float32": -126, "bfloat16": -126, "float16": -14}


def half_ulp(p: torch.Tensor, dtype: str) -> torch.Tensor:
    """ulp_dtype(p) / 2 as f32 (p a tensor of the dtype, finite and non-zero)"""
    _, e = torch.frexp(p.float().abs())  # |p| = m 2^e, m in [0.5, 1)
    e = torch.clamp(e - 1, min=_EMIN[dtype])
    return torch.ldexp(torch.ones_like(p, dtype=torch.float32), e - _MANT[dtype] - 1)


@functools.lru_cache(maxsize=None)
def apply_inputs():
    """(dtypes, params, delta): f32, bf16 and f16 tensors of APPLY_SIZES elements each, N(0, 0.02^2);
    delta ~ 1e-3 N(0, 1); in BAND delta = -+ulp_dtype(p) / 2 (p - delta is an exact tie at decay 1:
    for f32 of the fma's own rounding, for bf16 / f16 of the rounding to the dtype); P_EDGE over
    D_EDGE at the head of every tensor (f16 overflow, inf - inf, NaN, a subnormal delta)."""
    g = torch.Generator().manual_seed(41)
    dts, ps, ds = [], [], []
    for d in ("float32", "bfloat16", "float16"):
        for n in APPLY_SIZES:
            p = (torch.randn(n, generator=g) * 0.02).to(TD[d])
            dl = (torch.randn(n, generator=g) * 1e-3).float()
            if n > BAND[1]:
                b = slice(*BAND)
                sign = torch.where(torch.arange(BAND[1] - BAND[0]) % 2 == 0, -1.0, 1.0)
                h = half_ulp(p[b], d) * sign
                dl[b] = torch.where(p[b].float() != 0, h, torch.zeros_like(h))
            m = min(n, len(P_EDGE))
            p[:m] = torch.tensor(P_EDGE[:m]).to(TD[d])
            m = min(n, len(D_EDGE))
            dl[:m] = torch.tensor(D_EDGE[:m], dtype=torch.float32)
            dts.append(d)
            ps.append(p)
            ds.append(dl)
    return dts, ps, torch.cat(ds)


def apply_decay_sets():
    """per tensor: each decay for the whole list, then the five mixed over the tensors of one call"""
    n = 3 * len(APPLY_SIZES)
    return [[c] * n for c in APPLY_DECAYS] + [[APPLY_DECAYS[i % len(APPLY_DECAYS)] for i in range(n)]]


def apply_expected_nan(p: torch.Tensor, delta: torch.Tensor, decay: float) -> torch.Tensor:
    """Where fma(decay, p, -delta) must be NaN, from the inputs alone: a NaN operand, 0 * inf, or
    an infinite product met by the infinity of the same sign in delta."""
    t = float(f32(decay)) * p.double()  # NaN for 0 * inf
    dl = delta.double()
    return torch.isnan(t) | torch.isnan(dl) | (torch.isinf(t) & torch.isinf(dl) & ((t > 0) == (dl > 0)))


def to_bits(t: torch.Tensor) -> np.ndarray:
    """a tensor's elements as unsigned integers of their width"""
    t = t.detach().contiguous().cpu()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.view(torch.int32).numpy().view(np.uint32).copy()


def oracle_apply(dtypes, params, delta, decays, frozen=None):
    """O.delta_apply on copies of ``params`` (torch tensors); returns the new arrays as stored."""
    arrays = []
    for p, d in zip(params, dtypes):
        b = to_bits(p)
        arrays.append(b.view(np.float32) if d == "float32" else b)
    O.delta_apply(arrays, [DTC[d] for d in dtypes], np.ascontiguousarray(delta.detach().cpu().numpy(), dtype=np.float32),
                  decays, frozen=frozen)
    return arrays


def stored(t: torch.Tensor) -> np.ndarray:
    """a tensor's elements as the oracle stores them (float32, or uint16 bits): conftest.assert_bitwise's form"""
    b = to_bits(t)
    return b.view(np.float32) if b.dtype == np.uint32 else b


def as_uint(a: np.ndarray) -> np.ndarray:
    return a.view(np.uint32) if a.dtype == np.float32 else a
