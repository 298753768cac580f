"""FKSD-1 on the device (include/fks.h fks_digest, codec.model_digest) against its numpy
restatement (tests/fksd1.py), exactly: the known answers, every size at which the kernel
takes another path (empty, single elements, one vector more or less than a wave's load,
one tile more or less, several blocks, more tensors than one launch carries), views whose
data are only element-aligned, 64-bit positions, piecewise digests, and the trainers'
use of it.  Every comparison is of integers; nothing here has a tolerance."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import fksd1
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _rand(n, kind, dev, seed):
    """n elements of random bits (NaNs and infinities included: the digest reads bits)."""
    rng = np.random.default_rng(seed)
    if kind == "f32":
        a = rng.integers(0, 1 << 32, n, dtype=np.uint32).view(np.int32)
        return torch.from_numpy(a).view(torch.float32).to(dev)
    a = rng.integers(0, 1 << 16, n, dtype=np.uint16).view(np.int16)
    return torch.from_numpy(a).view(_TORCH[kind]).to(dev)


def _pair(t):
    """(sum, xor) of a codec.model_digest result."""
    from fate_llm.algo.fedkseed import codec
    b = codec.digest_bytes(t)
    return int.from_bytes(b[:8], "little"), int.from_bytes(b[8:], "little")


def _abi(tensors, pos0=0, out=None, codes=None):
    """fks_digest through ctypes: (return code, (sum, xor))."""
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    L = N.load()
    arr = (N.FksTensor * max(1, len(tensors)))()
    for i, t in enumerate(tensors):
        arr[i].data = t.data_ptr() if t.numel() else None
        arr[i].numel = t.numel()
        arr[i].dtype = codes[i] if codes else codec._DTYPES[t.dtype]
        arr[i].flags = 0xFFFF  # ignored, like lr and wd
        arr[i].lr = arr[i].wd = float("nan")
    dev = _dev()
    res = torch.full((2,), -1, dtype=torch.int64, device=dev) if out is None else out
    rc = L.fks_digest(ctypes.addressof(arr), len(tensors), pos0, res.data_ptr() if res is not None else None,
                      torch.cuda.current_stream(dev).cuda_stream)
    return rc, (_pair(res) if rc == 0 else None)


def test_known_answers_through_the_c_abi():
    dev = _dev()
    for arrays, want in fksd1.KNOWN:
        ts = []
        for a in arrays:
            if a.dtype == np.uint16:
                ts.append(torch.from_numpy(a.view(np.int16)).view(torch.bfloat16).to(dev))
            else:
                ts.append(torch.from_numpy(a).to(dev))
        assert _abi(ts) == (0, want)
    # f16 elements are 16 raw bits like bf16 ones
    bits = torch.tensor([0x3F80, 0xBF80 - 0x10000, 0x7FC0], dtype=torch.int16)
    ts = [torch.arange(7, dtype=torch.float32, device=dev), bits.view(torch.float16).to(dev),
          torch.empty(0, dtype=torch.float32, device=dev)]
    assert _abi(ts) == (0, fksd1.KNOWN[1][1])


def test_empty_lists_and_bad_arguments():
    from fate_llm.algo.fedkseed import _native as N
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    assert _abi([]) == (0, (0, 0))
    empties = [torch.empty(0, dtype=d, device=dev) for d in (torch.float32, torch.bfloat16, torch.float16)]
    assert _abi(empties) == (0, (0, 0))
    assert _pair(codec.model_digest([])) == (0, 0)
    assert _pair(codec.model_digest(empties, pos0=77)) == (0, 0)
    t = _rand(17, "bf16", dev, 1)
    assert _abi([t], codes=[7])[0] == -22  # -FKS_EINVAL: a bad dtype
    L = N.load()
    arr = (N.FksTensor * 1)()
    arr[0].data, arr[0].numel, arr[0].dtype = t.data_ptr(), 17, N.BF16
    assert L.fks_digest(ctypes.addressof(arr), 1, 0, None, None) == -22  # dev_out2 == NULL
    assert b"digest output" in L.fks_last_error()
    with pytest.raises(NotImplementedError):
        codec.model_digest([torch.zeros(4, dtype=torch.float64, device=dev)])
    with pytest.raises(ValueError):
        codec.model_digest([torch.zeros(4)])


NUMELS = (0, 1, 15, 16, 17, 255, 256, 257, 4099)


@pytest.fixture(scope="module")
def mixed():
    """The mixed list: every numel in every dtype, views starting at odd element offsets
    (bf16 / f16 data 2-byte aligned, f32 data 4-byte aligned, every residue mod 16 bytes),
    a non-contiguous tensor, and two tensors of several tiles (several blocks)."""
    dev = _dev()
    ts, seed = [], 0
    for n in NUMELS:
        for kind in ("f32", "bf16", "f16"):
            seed += 1
            ts.append(_rand(n, kind, dev, seed))
    for kind, offs in (("bf16", (1, 2, 3, 4, 5, 6, 7)), ("f16", (2, 6)), ("f32", (1, 2, 3))):
        for off in offs:
            for n in (5, 40, 4099):
                seed += 1
                ts.append(_rand(n + off, kind, dev, seed)[off:])
    ts.append(_rand(37 * 24, "bf16", dev, 900).view(37, 24).t())        # non-contiguous: row-major order of the view
    ts.append(_rand(19 * 8, "f32", dev, 901).view(19, 8)[:, 1:6])
    ts.append(_rand(3 * 4096 + 5, "f32", dev, 902))                     # 13 tiles: 4 blocks
    ts.append(_rand(40_000 + 3, "bf16", dev, 903)[3:])                  # 20 tiles behind a 5-element head
    assert any(t.data_ptr() % 16 == 2 for t in ts) and any(t.data_ptr() % 16 == 4 for t in ts)
    assert any(not t.is_contiguous() for t in ts)
    return ts


def test_mixed_list_against_numpy(mixed):
    from fate_llm.algo.fedkseed import codec
    assert len(mixed) > 64  # more tensors than one launch carries
    before = [t.clone() for t in mixed]
    got = codec.model_digest(mixed)
    assert got.dtype == torch.int64 and got.shape == (2,) and got.device == mixed[0].device
    assert _pair(got) == fksd1.digest(mixed)
    for a, b in zip(mixed, before):  # read-only, the staging copy of a view included
        assert torch.equal(a.view(torch.int16) if a.element_size() == 2 else a.view(torch.int32),
                           b.view(torch.int16) if b.element_size() == 2 else b.view(torch.int32))
    # each tensor alone (the contiguous ones through the C ABI as they lie in memory)
    for i, t in enumerate(mixed):
        want = fksd1.digest([t], pos0=i)
        assert _pair(codec.model_digest([t], pos0=i)) == want, (i, tuple(t.shape), t.dtype)
        if t.is_contiguous():
            assert _abi([t], pos0=i) == (0, want)


@pytest.mark.parametrize("pos0", [(1 << 32) - 3, (1 << 40) + 5, (1 << 64) - 9])
def test_64_bit_positions(pos0):
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    ts = [_rand(9, "bf16", dev, 11), _rand(0, "f32", dev, 12), _rand(5, "f32", dev, 13), _rand(3, "f16", dev, 14)]
    assert sum(t.numel() for t in ts) == 17
    assert _pair(codec.model_digest(ts, pos0=pos0)) == fksd1.digest(ts, pos0)
    assert _abi(ts, pos0=pos0) == (0, fksd1.digest(ts, pos0))


def test_slices_combine_into_the_whole(mixed):
    from fate_llm.algo.fedkseed import codec
    ts = [t for t in mixed if t.is_contiguous()]
    pos0 = (1 << 32) - 1000
    whole = codec.digest_bytes(codec.model_digest(ts, pos0=pos0))
    assert whole == fksd1.digest_bytes(ts, pos0)
    total = sum(t.numel() for t in ts)
    # cut the concatenation at tensor boundaries and inside tensors
    bounds = np.cumsum([0] + [t.numel() for t in ts])
    cuts = sorted({0, total, int(bounds[5]), int(bounds[20]), int(bounds[20]) + 1, total // 3, total // 2 + 1,
                   int(bounds[-2]) + 4097, int(bounds[-1]) - 1})
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        piece = []
        for t, b in zip(ts, bounds[:-1]):
            a, e = max(lo, int(b)), min(hi, int(b) + t.numel())
            if a < e:
                piece.append(t.view(-1)[a - int(b):e - int(b)])
        parts.append(codec.digest_bytes(codec.model_digest(piece, pos0=pos0 + lo)))
    assert len(parts) >= 8
    assert codec.combine_digests(parts) == whole


def test_one_bit_or_one_swap_changes_both_words():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    for kind in ("bf16", "f32"):
        t = _rand(4099, kind, dev, 21)
        base = _pair(codec.model_digest([t]))
        iv = t.view(torch.int16 if kind == "bf16" else torch.int32)
        for e in (0, 7, 2048, 4098):
            u = t.clone()
            u.view(iv.dtype)[e] ^= 1
            got = _pair(codec.model_digest([u]))
            assert got[0] != base[0] and got[1] != base[1], (kind, e)
            assert got == fksd1.digest([u])
        for e in (0, 1000, 4097):
            assert int(iv[e]) != int(iv[e + 1])
            u = t.clone()
            u[e], u[e + 1] = t[e + 1].clone(), t[e].clone()
            got = _pair(codec.model_digest([u]))
            assert got[0] != base[0] and got[1] != base[1], (kind, e)


def test_side_stream_sees_the_write_before_it_and_calls_repeat():
    from fate_llm.algo.fedkseed import codec
    dev = _dev()
    t = _rand(3 * 4096 + 5, "f32", dev, 31)
    u = _rand(3 * 4096 + 5, "f32", dev, 32)
    want_t, want_u = fksd1.digest([t]), fksd1.digest([u])
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        t.copy_(u)  # in place, on the side stream
        d1 = codec.model_digest([t])
        d2 = codec.model_digest([t])
    side.synchronize()
    assert want_t != want_u
    assert _pair(d1) == want_u and _pair(d2) == want_u
    # the output is zeroed by each call: a used buffer gives the same result
    out = torch.full((2,), 0x5A5A, dtype=torch.int64, device=dev)
    assert _abi([t], out=out) == (0, want_u)
    assert _abi([t], out=out) == (0, want_u)


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.emb = nn.Embedding(30, 16)
        self.proj = nn.Linear(16, 30, bias=True)
        self.proj.weight = self.emb.weight  # tied: hashed once
        self.norm = nn.LayerNorm(16)
        self.odd = nn.Parameter(torch.randn(4099, generator=g) * 0.02)
        self.frozen = nn.Parameter(torch.randn(33, generator=g), requires_grad=False)
        self.register_buffer("steps", torch.arange(7))  # buffers are not part of the digest


class _Args:
    learning_rate = 1e-3
    weight_decay = 0.01

    def __init__(self, dev):
        self.device = dev


def _sums(k=40):
    g = torch.Generator().manual_seed(5)
    seeds = torch.randint(0, 2**32, (k,), generator=g).tolist()
    return {s: float(v) for s, v in zip(seeds, torch.randn(k, generator=g, dtype=torch.float64) * 20)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reconstruct_leaves_the_digest_of_the_model(dtype):
    from fate_llm.algo.fedkseed.fedkseed import ClientTrainer
    dev = _dev()
    model_0 = _Tiny().to(dtype)
    ct = ClientTrainer(None, model_0, None, _Args(dev), None, None, None, None)
    off = ClientTrainer(None, copy.deepcopy(model_0), None, _Args(dev), None, None, None, None, verify_model=False)
    for sums in (None, _sums()):  # round 0 included
        model = ct.reconstruct(sums)
        params = [p for _, p in model.named_parameters()]
        assert len(params) == 6  # tied weight once, the frozen parameter included
        assert _pair(ct.model_digest) == fksd1.digest([p.data for p in params])
        plain = off.reconstruct(sums)
        assert off.model_digest is None
        for (k, a), (_, b) in zip(model.state_dict().items(), plain.state_dict().items()):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) if a.is_floating_point() else torch.equal(a, b), k
    # another model_0 is another digest: one last bit of the frozen parameter, which no step
    # rounds away
    first = _pair(ct.model_digest)
    with torch.no_grad():
        other_0 = copy.deepcopy(model_0)
        other_0.frozen.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)[3] ^= 1
    other = ClientTrainer(None, other_0, None, _Args(dev), None, None, None, None)
    other.reconstruct(_sums())
    assert _pair(other.model_digest) != first


class _OneRound:
    """A federation context of one client and one round that keeps what the client puts."""

    def __init__(self, message):
        self.message, self.put_values = message, []
        self.arbiter = self

    def ctxs_range(self, n):
        for i in range(n):
            yield i, self

    def get(self, key):
        assert key == "train_once"
        return self.message

    def put(self, key, value):
        assert key == "direction_derivative_history"
        self.put_values.append(value)


def test_history_over_a_wire_context_carries_the_digest():
    from fate_llm.algo.fedkseed import fedkseed as F
    from fate_llm.algo.fedkseed import payload as W
    dev = _dev()
    sums = _sums(8)
    cands = torch.tensor(list(sums))

    class Client(F.ClientTrainer):
        """train_once without transformers: the reconstruct, then local steps that move the
        model on (the digest is of the reconstructed model, not of what training leaves)."""

        def train_once(self, seed_candidates, seed_probabilities, direction_derivative_sum):
            model = self.reconstruct(direction_derivative_sum)
            self.want = fksd1.digest_bytes([p.data for _, p in model.named_parameters()])
            with torch.no_grad():
                for p in model.parameters():
                    p.add_(1.0)
            return {int(s): ([0.25] if i == 1 else []) for i, s in enumerate(seed_candidates)}

    msg = (False, {"seed_candidates": cands, "seed_probabilities": torch.ones(8) / 8,
                   "direction_derivative_sum": sums})
    for wire in (True, False):
        inner = _OneRound(W.encode_train_once(msg) if wire else msg)
        ctx = W.WireContext(inner) if wire else inner
        cl = Client(ctx, _Tiny().to(torch.bfloat16), F.FedKSeedTrainingArguments(num_aggregations=1), _Args(dev),
                    None, None, None, None)
        cl.train()
        (put,) = inner.put_values
        if not wire:  # a plain context's arbiter unpickles the dict, as before
            assert type(put) is dict
            continue
        assert put[4] == 2  # a version-2 record
        back = W.decode_history(put, cands.tolist())
        assert back.model_digest == cl.want
        assert back == {int(s): ([0.25] if i == 1 else []) for i, s in enumerate(cands)}
        assert back.stream_mode == "torch_cpu"
