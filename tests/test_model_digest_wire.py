"""The model fingerprint on the wire and at the arbiter (CPU, no device).

Every client of a round rebuilds its model from the same model_0 and the same sums, so the
16-byte FKSD-1 digest of the reconstructed model (include/fks.h fks_digest; restated in
numpy by tests/fksd1.py) must be the same at every client.  What these tests pin:

* the numpy restatement gives the contract's two known answers, and digests of a partition
  of the elements combine (add, xor) into the digest of the whole;
* a history record with a digest is version 2, 16 bytes longer, flag bit 12; one without is
  byte for byte the version-1 record; malformed combinations are ``WireFormatError``;
* the arbiter compares the declared digests before it folds a round's histories:
  ``ModelMismatchError`` names the clients, the sums stay as they were.
"""
import logging
import queue
import struct
import threading

import numpy as np
import pytest
import torch

import fksd1
from fate_llm.algo.fedkseed import codec
from fate_llm.algo.fedkseed import fedkseed as F
from fate_llm.algo.fedkseed import payload as W

CANDS = [3, 1 << 31, 7]
HIST = {3: [0.25, -1.5], 1 << 31: [], 7: [2.0]}
DIGEST = fksd1.to_bytes(fksd1.KNOWN[1][1])


def test_known_answers():
    for arrays, want in fksd1.KNOWN:
        assert fksd1.digest(arrays) == want
    assert fksd1.to_bytes((1, 2 << 56)) == b"\x01" + bytes(7) + bytes(7) + b"\x02"  # two little-endian u64


def test_combine_digests_over_a_partition():
    rng = np.random.default_rng(5)
    arrays = [rng.integers(0, 1 << 16, 37, dtype=np.uint16), rng.standard_normal(11).astype(np.float32),
              np.zeros(0, np.uint16), rng.integers(0, 1 << 16, 300, dtype=np.uint16)]
    for pos0 in (0, (1 << 32) - 5, (1 << 64) - 9):
        whole = fksd1.digest_bytes(arrays, pos0)
        # cut inside tensors and at their boundaries; each piece with its own pos0
        parts, q = [], pos0
        for a in arrays:
            cuts = [0, a.size // 3, a.size // 3, a.size] if a.size else [0, 0]
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                parts.append(fksd1.digest_bytes([a[lo:hi]], q + lo))
            q += a.size
        assert codec.combine_digests(parts) == whole
        assert codec.combine_digests(list(reversed(parts))) == whole
    assert codec.combine_digests([]) == bytes(16)
    assert codec.combine_digests([DIGEST]) == DIGEST
    with pytest.raises(ValueError):
        codec.combine_digests([b"short"])


def test_round_trip_with_and_without_a_digest():
    for c in (CANDS, None):  # sparse and explicit-key forms
        for stream, grid in ((None, None), ("torch_cpu", None), ("torch_rocm", 2048)):
            rec = W.encode_history(HIST, c, stream, grid, model_digest=DIGEST)
            back = W.decode_history(rec, c)
            assert isinstance(back, W.History) and back == HIST and list(back) == list(HIST)
            assert (back.stream_mode, back.stream_grid, back.model_digest) == (stream, grid, DIGEST)
            plain = W.decode_history(W.encode_history(HIST, c, stream, grid), c)
            assert plain == HIST and getattr(plain, "model_digest", None) is None
    assert type(W.decode_history(W.encode_history(HIST, CANDS), CANDS)) is dict
    with pytest.raises(W.WireFormatError):
        W.encode_history(HIST, CANDS, model_digest=b"\0" * 15)


def test_record_without_a_digest_is_the_version_1_record():
    # the version-1 layout, written out by hand: header (magic, version, kind, flags, count),
    # [grid cap], then sparse (index, count) pairs and f32 values
    body = np.array([0, 2], "<u4").tobytes() + np.array([2, 1], "<u4").tobytes() + \
        np.array([0.25, -1.5, 2.0], "<f4").tobytes()
    sparse = 1 << 3
    assert W.encode_history(HIST, CANDS) == struct.pack("<4sBBHQ", b"FKSW", 1, 2, sparse, 2) + body
    tagged = sparse | (1 << 8) | (1 << 9) | (1 << 10)
    assert (W.encode_history(HIST, CANDS, "torch_rocm", 2048)
            == struct.pack("<4sBBHQ", b"FKSW", 1, 2, tagged, 2) + struct.pack("<I", 2048) + body)
    # ... and the digest record: version 2, bit 12, the 16 bytes after the grid cap
    assert (W.encode_history(HIST, CANDS, "torch_rocm", 2048, DIGEST)
            == struct.pack("<4sBBHQ", b"FKSW", 2, 2, tagged | (1 << 12), 2) + struct.pack("<I", 2048) + DIGEST + body)
    for c in (CANDS, None):
        for stream, grid in ((None, None), ("torch_rocm", 256)):
            plain = W.encode_history(HIST, c, stream, grid)
            with_d = W.encode_history(HIST, c, stream, grid, DIGEST)
            assert plain[4] == 1 and with_d[4] == 2
            assert len(with_d) == len(plain) + 16
    # train_once records are unchanged: version 1
    msg = (False, {"seed_candidates": torch.tensor(CANDS), "seed_probabilities": torch.ones(3) / 3,
                   "direction_derivative_sum": {3: 1.0, 1 << 31: 0.0, 7: -2.0}})
    assert W.encode_train_once(msg, "torch_rocm", 2048)[4] == 1


def _reheader(rec, version=None, flags=None):
    magic, v, kind, f, count = W._HEADER.unpack_from(rec, 0)
    return W._HEADER.pack(magic, v if version is None else version, kind, f if flags is None else flags,
                          count) + rec[W._HEADER.size:]


def test_malformed_digest_records():
    rec = W.encode_history(HIST, CANDS, "torch_rocm", 2048, DIGEST)
    plain = W.encode_history(HIST, CANDS, "torch_rocm", 2048)
    flags = W._HEADER.unpack_from(rec, 0)[3]
    assert flags & (1 << 12) and W.decode_history(rec, CANDS).model_digest == DIGEST
    with pytest.raises(W.WireFormatError, match="version"):
        W.decode_history(_reheader(rec, version=1), CANDS)        # version 1 with bit 12
    with pytest.raises(W.WireFormatError, match="version"):
        W.decode_history(_reheader(plain, version=2), CANDS)      # version 2 without it
    with pytest.raises(W.WireFormatError, match="version"):
        W.decode_history(_reheader(rec, version=3), CANDS)
    with pytest.raises(W.WireFormatError):
        W.decode_history(rec[:W._HEADER.size + 4 + 9], CANDS)     # the digest cut off
    with pytest.raises(W.WireFormatError):                        # 16 digest bytes, nothing after them
        W.decode_history(rec[:W._HEADER.size + 4 + 16], CANDS)
    for bit in (1 << 0, 1 << 4, 1 << 5, 1 << 13, 1 << 15):        # outside the history's known mask
        with pytest.raises(W.WireFormatError, match="unknown flag"):
            W.decode_history(_reheader(plain, flags=W._HEADER.unpack_from(plain, 0)[3] | bit), CANDS)
    msg = (False, {"seed_candidates": torch.tensor(CANDS), "seed_probabilities": None,
                   "direction_derivative_sum": None})
    once = W.encode_train_once(msg)
    for bit in (1 << 5, 1 << 12, 1 << 14):                        # train_once knows no digest
        with pytest.raises(W.WireFormatError, match="unknown flag"):
            W.decode_train_once(_reheader(once, flags=W._HEADER.unpack_from(once, 0)[3] | bit))
    with pytest.raises(W.WireFormatError, match="version"):
        W.decode_train_once(_reheader(once, version=2))


def test_check_model_digests():
    a, b = DIGEST, fksd1.to_bytes(fksd1.KNOWN[0][1])
    assert W.check_model_digests([None, None]) is None
    assert W.check_model_digests([None, a, a]) == a
    with pytest.raises(W.ModelMismatchError) as e:
        W.check_model_digests([a, None, b, a])
    msg = str(e.value)
    assert "client 0, client 3" in msg and "client 2" in msg and "client 1" not in msg
    assert f"{fksd1.KNOWN[1][1][0]:016x}:{fksd1.KNOWN[1][1][1]:016x}" in msg
    for cause in ("model_0", "stream", "glibc", "build"):
        assert cause in msg
    assert issubclass(W.ModelMismatchError, RuntimeError)


# --------------------------------------------------------------- a loopback federation
class _Party:
    def __init__(self, out_q, in_q):
        self.out_q, self.in_q = out_q, in_q
        self.got = []

    def put(self, key, value):
        self.out_q.put((key, value))

    def get(self, key):
        k, v = self.in_q.get(timeout=5)
        assert k == key, (k, key)
        self.got.append(v)
        return v


class _ArbiterCtx:
    def __init__(self, links):
        self.guest = _Party(links[0][0], links[0][1])
        self.hosts = [_Party(a, b) for a, b in links[1:]]

    def ctxs_range(self, n):
        for i in range(n):
            yield i, self


class _ClientCtx:
    def __init__(self, link):
        self.arbiter = _Party(link[1], link[0])

    def ctxs_range(self, n):
        for i in range(n):
            yield i, self


class _Args:
    learning_rate, weight_decay = 1e-5, 0.0
    device = "cpu"


class _DigestClient(F.ClientTrainer):
    """The drop-in ClientTrainer's round loop with a host-only local phase that leaves the
    digest a reconstruct would have launched: ``digests[r]`` in round r, a (sum, xor) pair,
    or None for a round in which the client declares none."""

    digests = ()
    rounds_done = 0

    def train_once(self, seed_candidates, seed_probabilities, direction_derivative_sum):
        d = self.digests[self.rounds_done]
        self.rounds_done += 1
        if d is not None:
            self.model_digest = torch.from_numpy(np.array(d, dtype=np.uint64).view(np.int64))
        first = int(seed_candidates[0])
        return {int(s): ([0.5] if int(s) == first else []) for s in seed_candidates}


class _SpyTrainer(F.Trainer):
    """Keeps the sums dict it hands to its puts: one object for the whole run, updated in
    place when a round's histories are folded."""

    sums = None

    def get_clients(self, ctx):
        owner = self

        class _Spy:
            def __init__(self, party):
                self.party = party

            def put(self, key, value):
                owner.sums = value[1]["direction_derivative_sum"]
                return self.party.put(key, value)

            def get(self, key):
                return self.party.get(key)

        return [_Spy(c) for c in F.Trainer.get_clients(ctx)]


def _federation(digests, rounds, wire=True):
    """One client per entry of ``digests`` (its per-round digests); returns the arbiter, the
    errors by party, and the arbiter side's raw parties."""
    links = [(queue.Queue(), queue.Queue()) for _ in digests]
    errors, threads = {}, []

    def run(name, fn):
        try:
            fn()
        except Exception as e:  # noqa: BLE001 -- reported to the test
            errors[name] = e

    wrap = W.WireContext if wire else (lambda c: c)
    actx = _ArbiterCtx(links)
    arb = _SpyTrainer(wrap(actx), torch.tensor([11, 22, 33]), None,
                      F.FedKSeedTrainingArguments(num_aggregations=rounds, k=3))
    threads.append(threading.Thread(target=run, args=("arbiter", arb.train), daemon=True))
    for i, (d, link) in enumerate(zip(digests, links)):
        cl = _DigestClient(wrap(_ClientCtx(link)), torch.nn.Linear(2, 2),
                           F.FedKSeedTrainingArguments(num_aggregations=rounds), _Args(), None, None, None, None)
        cl.digests = d
        threads.append(threading.Thread(target=run, args=(f"client{i}", cl.train), daemon=True))
    for t in threads:
        t.start()
    threads[0].join(timeout=30)
    assert not threads[0].is_alive()
    if "arbiter" not in errors:  # after an arbiter failure the clients wait for a record that never comes
        for t in threads[1:]:
            t.join(timeout=5)
    return arb, errors, [actx.guest] + actx.hosts


A, B = fksd1.KNOWN[1][1], fksd1.KNOWN[0][1]


@pytest.fixture(autouse=True)
def _cpu_stream(monkeypatch):
    monkeypatch.setattr(codec, "_stream_mode", "torch_cpu")


def test_equal_digests_run():
    arb, errors, parties = _federation([[A, A]] * 3, rounds=2)
    assert not errors
    assert arb.model_digest == fksd1.to_bytes(A)
    assert arb.sums == {11: 3.0, 22: 0.0, 33: 0.0}
    assert all(rec[4] == 2 for p in parties for rec in p.got)  # version-2 records on the wire


def test_one_differing_client_fails_loudly_before_the_fold():
    # round 1 agrees; in round 2 client 2 (the second host) holds another model
    arb, errors, _ = _federation([[A, A], [A, A], [A, B]], rounds=2)
    err = errors.get("arbiter")
    assert isinstance(err, W.ModelMismatchError), errors
    assert "client 2" in str(err) and "client 0, client 1" in str(err)
    assert arb.sums == {11: 1.5, 22: 0.0, 33: 0.0}  # round 1's fold (3 x 0.5); round 2 added nothing
    assert arb.model_digest == fksd1.to_bytes(A)     # of the last round that agreed


def test_declared_and_undeclared_digests_mix_with_a_warning(caplog):
    with caplog.at_level(logging.INFO, logger=F.logger.name):
        arb, errors, _ = _federation([[A, A], [None, None], [A, A]], rounds=2)
    assert not errors
    assert arb.model_digest == fksd1.to_bytes(A) and arb.sums == {11: 3.0, 22: 0.0, 33: 0.0}
    assert any(r.levelno == logging.WARNING and "model digest" in r.getMessage() for r in caplog.records)
    # the client that declares none says so in one line, not one per round
    assert len([r for r in caplog.records if "no model digest sent" in r.getMessage()]) == 1


def test_plain_context_sends_the_dict_as_before():
    arb, errors, parties = _federation([[A], [A]], rounds=1, wire=False)
    assert not errors and arb.model_digest is None
    assert all(type(h) is dict for p in parties for h in p.got)
