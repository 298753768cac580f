"""Tensor lists for the MT19937 (torch_cpu) stream's kernels, and a Python mirror of the layout the
library gives them.  A plain module: the tests import it; nothing of the library goes into it.

mirror(sizes, dts, frozen) restates make_layout's classification (csrc/fks_layout.cpp) for the
geometry-only plan of fks_project_mt_multi / fks_expand_mt_multi, where a tensor's pointer is
base + 4 x (its first element's index in the concatenation):

  a tensor of n >= 16 elements draws n stream words, plus 16 fresh ones if n % 16 != 0;
  one of 0 < n < 16 draws serially: 4 words per NEW Box-Muller pair, the second value of a pair is
  cached and taken by the next serial draw, whichever tensor makes it (frozen ones too);
  a tensor is a FAST SEGMENT iff it is live, n % 16 == 0, its first word is a multiple of 16, it
  is not f16 and its first element's index is even; any other live tensor of n >= 16 is a RUN of
  16 floor(n / 16) words under the limit n (n - 16 if ragged) plus, if ragged, a run of the 16 fresh
  words over its last 16 elements; every live element of a smaller tensor is a TINY element with
  its pair's first word and a flag for the cached (sin) half.

The lists (sizes exact; `frozen` are tensor indices):

  G  21 tensors, 15,088 elements, 25 MT blocks (of 624 words), tensor 5 frozen.  It exists for the
     fast kernel's segment lookup: three fast segments inside block 0 (the lookup advances several
     segments in one step), block 1 wholly inside the frozen gap (a chunk whose first word lies in
     a gap; lanes before the next segment), fast segments after tiny groups, after a ragged pair
     (1000 + 24 returns the stream to phase 0) and after the frozen stretch, four runs, 32 tiny
     elements.  "G:<dtype>" has one dtype, "G:mixed" cycles bf16, f32, f16 over the tensors: the
     f32 and the bf16 launch each see the other's segments, and the f16 tensors' runs, as gaps.
  R  800 tensors: the period [9984, 16, 16, 16, 5, 3, 1248, 32] a hundred times, positions 1 and 6
     of every period frozen; period r is f16 where r % 10 == 9, else bf16 for even r and f32 for
     odd r.  1,816 MT blocks -- more than the plan has chunks on a device of up to 600 CUs, so a
     workgroup walks several blocks and its lookahead crosses segment ends, gaps and the other
     dtype's stretches --, segment starts at many phases of the 624-word block, and a table of
     1,200 entries (360 fast segments, 40 runs, 800 tiny elements).
  sweep(case), case in range(SWEEP): seeded lists out of motifs that each return the stream to
     phase 0 and an even element index, so that fast segments keep appearing after irregular work
     (sizes drawn freely almost never give one after the first irregular tensor)."""
import collections
import functools

import numpy as np
import torch

MT_N = 624
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
CYC = ["bfloat16", "float32", "float16"]
SWEEP = 32

Seg = collections.namedtuple("Seg", "tensor dtype start numel elem")  # elem: first element in the concatenation
Run = collections.namedtuple("Run", "tensor dtype start numel limit elem")
Tiny = collections.namedtuple("Tiny", "tensor dtype word sin elem")
Mirror = collections.namedtuple("Mirror", "segs runs tiny stream_len")
MtList = collections.namedtuple("MtList", "name sizes dts frozen")


def mirror(sizes, dts, frozen=()):
    segs, runs, tiny = [], [], []
    cum = pos = pair = 0
    cached = False
    for i, (n, d) in enumerate(zip(sizes, dts)):
        live = i not in frozen
        first = cum
        cum += n
        if n >= 16:
            fast = n % 16 == 0 and pos % 16 == 0 and d != "float16" and first % 2 == 0
            if live and fast:
                segs.append(Seg(i, d, pos, n, first))
            elif live:
                runs.append(Run(i, d, pos, 16 * (n // 16), n - 16 if n % 16 else n, first))
                if n % 16:
                    runs.append(Run(i, d, pos + n, 16, 16, first + n - 16))
            pos += n + (16 if n % 16 else 0)
        else:
            for e in range(n):
                if cached:
                    cached, word, sin = False, pair, True
                else:
                    cached, pair, word, sin = True, pos, pos, False
                    pos += 4
                if live:
                    tiny.append(Tiny(i, d, word, sin, first + e))
    return Mirror(segs, runs, tiny, pos)


def mirror_of(lst):
    return mirror(lst.sizes, lst.dts, lst.frozen)


def nblocks(m):
    return max(1, -(-m.stream_len // MT_N))


def segs_of(m, dtype):
    return [s for s in m.segs if s.dtype == dtype]


def facts(m):
    """What a layout offers the fast kernel's lookup, per non-f16 dtype and overall."""
    out = {"fast": len(m.segs), "runs": len(m.runs), "tiny": len(m.tiny), "gap": False, "three_in_a_block": False,
           "empty_block_between": False, "odd_phase_run": any(r.start % 16 for r in m.runs),
           "both": all(segs_of(m, d) for d in ("bfloat16", "float32"))}
    for d in ("bfloat16", "float32"):
        ss = segs_of(m, d)
        out["gap"] |= any(a.start + a.numel < b.start for a, b in zip(ss, ss[1:]))
        per_block = collections.Counter(b for s in ss
                                        for b in range(s.start // MT_N, (s.start + s.numel - 1) // MT_N + 1))
        out["three_in_a_block"] |= any(c >= 3 for c in per_block.values())
        if ss:
            lo, hi = ss[0].start // MT_N, (ss[-1].start + ss[-1].numel - 1) // MT_N
            out["empty_block_between"] |= any(b not in per_block for b in range(lo, hi + 1))
    return out


G_SIZES = [16, 5, 3, 16, 32, 1248, 16, 8, 9984, 4, 4, 16, 1000, 24, 48, 0, 640, 7, 1, 2000, 16]
G_FROZEN = (5,)
G_NAMES = ["G:bfloat16", "G:float32", "G:float16", "G:mixed"]
R_PERIOD = [9984, 16, 16, 16, 5, 3, 1248, 32]
R_FROZEN_AT = (1, 6)


@functools.lru_cache(maxsize=None)
def named(name):
    if name == "R":
        sizes, dts, frozen = [], [], []
        for r in range(100):
            d = "float16" if r % 10 == 9 else ("bfloat16", "float32")[r % 2]
            frozen += [len(sizes) + j for j in R_FROZEN_AT]
            sizes += R_PERIOD
            dts += [d] * len(R_PERIOD)
        return MtList(name, tuple(sizes), tuple(dts), tuple(frozen))
    kind = name[2:]  # "G:<dtype>" or "G:mixed"
    dts = [CYC[i % 3] for i in range(len(G_SIZES))] if kind == "mixed" else [kind] * len(G_SIZES)
    return MtList(name, tuple(G_SIZES), tuple(dts), G_FROZEN)


_SERIAL = [(8,), (5, 3), (1, 7), (2, 2, 4), (3, 1, 4), (15, 1)]


@functools.lru_cache(maxsize=None)
def sweep(case):
    """Sweep case `case`: 4 to 13 motifs, each a list of (size, frozen) that leaves the stream at
    phase 0 and the element index even."""
    g = np.random.default_rng(9000 + case)
    pieces = []  # (size, frozen)

    def m16(lo, hi):
        return 16 * int(g.integers(lo, hi + 1))

    for _ in range(int(g.integers(4, 14))):
        kind = int(g.integers(0, 9))
        if kind == 0:  # a fast piece, short or long
            pieces.append((m16(1, 3) if g.random() < 0.5 else m16(4, 299), False))
        elif kind in (1, 2):  # three 16-element-scale pieces in a row
            pieces += [(m16(1, 2), False), (16, False), (16, False)]
        elif kind in (3, 4):  # a serial group: whole Box-Muller pairs
            pieces += [(n, bool(g.random() < 0.2)) for n in _SERIAL[int(g.integers(0, len(_SERIAL)))]]
        elif kind == 5:  # a ragged pair, half the time around a run at a non-zero phase
            n = int(g.integers(17, 700))
            n += 1 if n % 16 == 0 else 0
            n2 = 16 * int(g.integers(2, 40)) - n % 16
            pieces.append((n, False))
            if g.random() < 0.5:
                pieces.append((m16(1, 80), False))
            pieces.append((n2, False))
        elif kind == 6:  # a frozen stretch
            pieces.append((m16(1, 60), True))
        elif kind == 7:  # whole MT blocks, frozen half the time
            pieces.append((MT_N * int(g.integers(1, 4)), bool(g.random() < 0.5)))
        else:
            pieces.append((0, False))
    u = g.random()
    if u < 0.35:
        dts = [("bfloat16", "float32")[int(g.integers(0, 2))]] * len(pieces)
    elif u < 0.45:
        dts = ["float16"] * len(pieces)
    else:
        dts = [CYC[int(g.choice(3, p=[0.4, 0.4, 0.2]))] for _ in pieces]
    return MtList(f"sweep{case}", tuple(n for n, _ in pieces), tuple(dts),
                  tuple(i for i, (_, f) in enumerate(pieces) if f))


def offsets(sizes):
    return [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]


def live_mask(lst):
    off = offsets(lst.sizes)
    live = np.ones(off[-1], bool)
    for i in lst.frozen:
        live[off[i]:off[i + 1]] = False
    return live


def draw(lst, seed):
    """The reference z of one seed over the concatenation, as the reference draws it on the CPU:
    torch.manual_seed, then torch.normal per tensor in the tensor's dtype (frozen tensors too),
    widened to f32; a CPU tensor."""
    torch.manual_seed(seed)
    z = [torch.normal(mean=0, std=1, size=(n,), dtype=DT[d]).float() for n, d in zip(lst.sizes, lst.dts)]
    return torch.cat(z) if z else torch.zeros(0)


def get(name):
    """a list by name: "G:<dtype>", "G:mixed", "R" or "sweep<case>" """
    return sweep(int(name[5:])) if name.startswith("sweep") else named(name)


_ZS = {}


def zs(name, seeds):
    """draw() of list `name` for the seeds given, which must extend or be a prefix of the seeds of
    earlier calls for that list: drawn once per list and seed, shared by the test files, never
    written to"""
    have = _ZS.setdefault(name, ([], []))
    assert have[0][:len(seeds)] == list(seeds)[:len(have[0])], "one seed list per list"
    while len(have[1]) < len(seeds):
        s = seeds[len(have[1])]
        have[0].append(s)
        have[1].append(draw(get(name), s))
    return have[1][:len(seeds)]
