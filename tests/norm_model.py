"""Exact model of the normalised float output formats (OUT_RGB_PLANAR_F16 /
_F32): out = fma(float(u8), a[c], b[c]) rounded once to fp32
(nearest-even), for F16 then rounded to half (nearest-even, overflow to inf,
subnormals kept).  Each channel has 256 possible inputs, so the model is a
(3, 256) table of bit patterns; v * a + b is formed exactly with
fractions.Fraction on the float32 constants, never through a float64 sum."""
from fractions import Fraction

import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _round_to_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the non-zero rational x, ties to even; subnormals
    kept, overflow to +-inf."""
    sign, x = (-1.0, -x) if x < 0 else (1.0, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()   # 2^(e-1) < x < 2^(e+1)
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)                      # the quantum of x's binade
    m = x / q
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    r = n * q
    if r >= Fraction(2) ** 128:
        return np.float32(sign * np.inf)
    f = float(r)                       # exact: 24 significant bits in float64's range
    assert Fraction(f) == r
    return np.float32(sign * f)


def _fma_f32(v: int, a: np.float32, b: np.float32) -> np.float32:
    exact = v * Fraction(float(a)) + Fraction(float(b))
    if exact != 0:
        return _round_to_f32(exact)
    # an exact zero: -0 only when the product and the addend are both -0
    # (v >= 0, so a zero product has a's sign); cancelling terms give +0
    prod_is_zero = v == 0 or a == 0
    if prod_is_zero and b == 0 and np.signbit(a) and np.signbit(b):
        return np.float32(-0.0)
    return np.float32(0.0)


def table(a, b, dtype) -> np.ndarray:
    """(3, 256) bit patterns (uint16 for float16, uint32 for float32) of every
    input byte, per channel, for the float32 constants a[3], b[3]."""
    a = np.broadcast_to(np.asarray(a, dtype=np.float32), (3,))
    b = np.broadcast_to(np.asarray(b, dtype=np.float32), (3,))
    assert np.isfinite(a).all() and np.isfinite(b).all()
    f32 = np.array([[_fma_f32(v, a[c], b[c]) for v in range(256)] for c in range(3)], dtype=np.float32)
    if np.dtype(dtype) == np.float32:
        return f32.view(np.uint32)
    assert np.dtype(dtype) == np.float16
    with np.errstate(over="ignore"):
        return f32.astype(np.float16).view(np.uint16)   # nearest-even, subnormals, inf


def apply(u8_planar, a, b, dtype) -> np.ndarray:
    """Bit patterns of the float frame of a (3, H, W) uint8 planar frame."""
    u8 = np.asarray(u8_planar)
    assert u8.dtype == np.uint8 and u8.shape[0] == 3
    t = table(a, b, dtype)
    return np.stack([t[c][u8[c]] for c in range(3)])
