"""FKSD-1, the model fingerprint, restated in numpy (test helper; include/fks.h fks_digest
has the definition, INTEGRATION.md the same snippet for reference parties).

The digest of a list of arrays laid end to end, the list starting at element ``pos0`` of a
larger concatenation.  Element e of array i has position q = pos0 + (sizes before i) + e and
raw bits b (16 bits of a bf16 / f16 element, 32 of an f32 one, zero-extended); mod 2^64:

    x = ((q + 1) * 0x9E3779B97F4A7C15) ^ b
    z = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z =  z ^ (z >> 31)
    digest = (sum of z mod 2^64, xor of z)

Pinned by the two known answers of the contract (tests/test_model_digest_wire.py).
"""
import numpy as np

MASK = (1 << 64) - 1
_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def bits_of(a) -> np.ndarray:
    """The raw element bits, row-major, as uint64: of a numpy array (uint16 = bf16 / f16
    bits, uint32 / float32, float16) or a torch tensor (bfloat16, float16, float32)."""
    if not isinstance(a, np.ndarray):
        import torch
        t = a.detach().cpu().contiguous().reshape(-1)
        a = t.view(torch.int16).numpy() if t.element_size() == 2 else t.view(torch.int32).numpy()
    a = np.ascontiguousarray(a).reshape(-1)
    if a.dtype.itemsize == 2:
        return a.view(np.uint16).astype(np.uint64)
    if a.dtype.itemsize == 4:
        return a.view(np.uint32).astype(np.uint64)
    raise TypeError(f"FKSD-1 covers 16- and 32-bit elements, not {a.dtype}")


def digest(arrays, pos0: int = 0):
    """(sum, xor) as python ints."""
    s = x = 0
    q = int(pos0)
    for a in arrays:
        b = bits_of(a)
        if b.size:
            with np.errstate(over="ignore"):
                pos = np.arange(b.size, dtype=np.uint64) + np.uint64((q + 1) & MASK)
                z = (pos * _G) ^ b
                z = (z ^ (z >> np.uint64(30))) * _M1
                z = (z ^ (z >> np.uint64(27))) * _M2
                z = z ^ (z >> np.uint64(31))
                s = (s + int(z.sum(dtype=np.uint64))) & MASK
            x ^= int(np.bitwise_xor.reduce(z))
        q += b.size
    return s, x


def to_bytes(d) -> bytes:
    """The 16 wire bytes of a (sum, xor) pair: two little-endian u64."""
    return int(d[0]).to_bytes(8, "little") + int(d[1]).to_bytes(8, "little")


def digest_bytes(arrays, pos0: int = 0) -> bytes:
    return to_bytes(digest(arrays, pos0))


# the contract's known answers (pos0 = 0)
KNOWN = (
    ([np.zeros(5, np.uint16)], (0x6B22E5CF60D56F79, 0x692E5A8979491863)),
    ([np.arange(7, dtype=np.float32), np.array([0x3F80, 0xBF80, 0x7FC0], np.uint16), np.zeros(0, np.float32)],
     (0x137A41D7F2732521, 0x9EB2728B3CD11F4D)),
)
