"""numpy model of the resize (include/hjd.h, hjd_resize_*): bilinear with
half-pixel centres, 11-bit integer weights, one rounding, optional horizontal
flip.  Everything is int64, and the bounds that let the kernel work in 32
bits are asserted on the values actually formed.  Float outputs are
norm_model.apply of the bytes."""
import numpy as np

import norm_model

MAX_DIM = 16384
WEIGHT = 2048   # 11-bit weights


def taps(size: int, out_size: int):
    """(p0, p1, f) per output index of one axis: the two source positions and
    the weight f (0..2047) of the second."""
    assert 1 <= size <= MAX_DIM and 1 <= out_size <= MAX_DIM
    j = np.arange(out_size, dtype=np.int64)
    n = np.maximum((2 * j + 1) * size - out_size, 0)
    den = 2 * out_size
    assert n.max() < 2 ** 31
    p0 = n // den
    rem = n % den
    assert (rem * WEIGHT).max() < 2 ** 31
    f = (rem * WEIGHT) // den
    assert 0 <= f.min() and f.max() < WEIGHT and p0.max() <= size - 1
    return p0, np.minimum(p0 + 1, size - 1), f


def resize_u8(src, out_w: int, out_h: int, flip: bool = False) -> np.ndarray:
    """(3, h, w) uint8 -> (3, out_h, out_w) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[0] == 3
    h, w = src.shape[1:]
    x0, x1, fx = taps(w, out_w)
    y0, y1, fy = taps(h, out_h)
    s = src.astype(np.int64)
    fx = fx[None, None, :]
    fy = fy[None, :, None]
    a = s[:, y0][:, :, x0]
    b = s[:, y0][:, :, x1]
    c = s[:, y1][:, :, x0]
    d = s[:, y1][:, :, x1]
    acc = (a * (WEIGHT - fx) * (WEIGHT - fy) + b * fx * (WEIGHT - fy) + c * (WEIGHT - fx) * fy + d * fx * fy +
           (1 << 21))
    assert acc.max() < 2 ** 31 and acc.min() >= 0
    out = (acc >> 22).astype(np.uint8)
    assert ((acc >> 22) <= 255).all()
    return np.ascontiguousarray(out[:, :, ::-1]) if flip else out


def resize(src, out_w: int, out_h: int, flip: bool = False, dtype=np.uint8, a=1.0, b=0.0) -> np.ndarray:
    """The output's bit patterns: uint8 bytes, or the uint16 / uint32 patterns
    of the float16 / float32 planes fma(float(u8), a[c], b[c])."""
    u8 = resize_u8(src, out_w, out_h, flip)
    return u8 if np.dtype(dtype) == np.uint8 else norm_model.apply(u8, a, b, dtype)
