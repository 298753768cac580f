"""An exact single-rounded f32 fma out of float64 torch operations, for references that must not
share code with the kernels they check.  A plain module: the tests import it.

fma32(a, b, c) returns RN_f32(a b + c) for f32-valued tensors on any device, every step a
separate torch op (nothing can be contracted):

  p = a b in f64 is exact (24 x 24 significand bits, exponents far inside f64's range);
  s = RN_f64(p + c) with its TwoSum error e (Knuth): bb = s - p, e = (p - (s - bb)) + (c - bb), so
  that p + c = s + e exactly and |e| <= ulp64(s) / 2;
  r = RN_f32(s) is RN_f32(s + e) unless s lies exactly midway between r and its f32 neighbour r2
  on s's side while e != 0: every f32 midpoint is an f64 number, so when s is none the exact sum
  lies on s's side of each of them and rounds as s does; when s is one, the exact sum lies on e's
  side of it: r2 if e points away from r, else r.  (s - r and r2 - s are exact in f64 whenever
  they can be equal.)

The one midpoint without two finite neighbours is M = 2^128 - 2^103, which RN_f32 sends to inf:
with |s| = M and e pointing to zero the exact sum is below M in magnitude and rounds to the
largest finite f32.  Where s is not finite the result is s.float(): the widened finite inputs
cannot overflow f64, and inf / NaN propagate as in an f32 fma.  f32 subnormals and signed zeros
need no case of their own: f64's addition signs a zero sum as f32's fma does, and the f64 -> f32
conversion rounds into the subnormal range to nearest even.

chain32(coefs, zs) folds acc = fma32(f32(c_s), z_s, acc) from +0.0f in the order given."""
import numpy as np
import torch

_M = float(2.0 ** 128 - 2.0 ** 103)  # the midpoint between the largest finite f32 and 2^128
_MAX = float(np.finfo(np.float32).max)


def f32(x):
    """the C cast (float)x of a Python number: round to nearest even, overflow to inf"""
    with np.errstate(over="ignore"):
        return np.float32(x)


def _f64(x, like=None):
    if not torch.is_tensor(x):
        x = torch.tensor(f32(x), device=None if like is None else like.device)
    if x.dtype != torch.float32:
        raise TypeError(f"fma32 takes float32 tensors (or numbers, taken as float32), got {x.dtype}")
    return x.double()


def fma32(a, b, c):
    """RN_f32(a * b + c), exactly, elementwise with broadcasting; float32 in, float32 out."""
    like = next((x for x in (a, b, c) if torch.is_tensor(x)), None)
    a, b, c = _f64(a, like), _f64(b, like), _f64(c, like)
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.float()
    d = s - r.double()  # > 0: s above r
    inf = torch.full_like(r, float("inf"))
    r2 = torch.nextafter(r, torch.where(d > 0, inf, -inf))
    tie = (d != 0) & (e != 0) & ((r2.double() - s) == d)
    out = torch.where(tie & ((e > 0) == (d > 0)), r2, r)
    top = (s.abs() == _M) & (e != 0) & ((e > 0) != (s > 0))
    out = torch.where(top, torch.copysign(torch.full_like(r, _MAX), r), out)
    return torch.where(torch.isfinite(s), out, r)


def chain32(coefs, zs):
    """acc = +0.0f; for (c, z) in zip(coefs, zs): acc = fma32(f32(c), z, acc).  ``zs`` may be a
    generator of float32 tensors of one shape; returns None for an empty chain."""
    acc = None
    for c, z in zip(coefs, zs):
        if acc is None:
            acc = torch.zeros_like(z)
        acc = fma32(torch.tensor(f32(c), device=z.device), z, acc)
    return acc
