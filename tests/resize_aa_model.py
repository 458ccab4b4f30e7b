"""numpy model of the antialiased resize (include/hjd.h, HJD_RESIZE_TRIANGLE_AA):
the exact triangle filter, separable, the horizontal pass rounded to uint8
before the vertical one, optional horizontal flip.  Everything is int64, and
the bounds that let the kernels work in 32 bits are asserted on the values
actually formed.  Float outputs are norm_model.apply of the bytes."""
import numpy as np

import norm_model

MAX_DIM = 16384
RATIO = 1 << 21   # legal: size * size <= RATIO * out_size, per axis


def legal(size: int, out_size: int) -> bool:
    return 1 <= size <= MAX_DIM and 1 <= out_size <= MAX_DIM and size * size <= RATIO * out_size


def axis_weights(size: int, out_size: int):
    """Per output index j of one axis: (k0, t) -- the first tap and the integer
    weights t_k of the taps k0 .. k0 + len(t) - 1."""
    assert legal(size, out_size), (size, out_size)
    s = max(size, out_size)
    k = np.arange(size, dtype=np.int64)
    out = []
    for j in range(out_size):
        c = (2 * j + 1) * size
        assert c + 2 * s < 2 ** 31
        d = (2 * k + 1) * out_size - c
        assert np.abs(d).max() < 2 ** 31
        t = 2 * s - np.abs(d)
        taps = np.flatnonzero(t > 0)
        assert taps.size and (np.diff(taps) == 1).all()   # the centre tap exists; the taps are one run
        t = t[taps]
        total = int(t.sum())
        assert 0 < total <= 2 * s * s // out_size + 2 * s
        assert 255 * total + total // 2 < 2 ** 31            # the kernels' accumulator
        out.append((int(taps[0]), t))
    return out


def axis_pass(src: np.ndarray, out_size: int) -> np.ndarray:
    """Resample the last axis of an int64 array of bytes; one rounding."""
    out = np.empty(src.shape[:-1] + (out_size,), np.int64)
    for j, (k0, t) in enumerate(axis_weights(src.shape[-1], out_size)):
        total = int(t.sum())
        acc = (src[..., k0:k0 + t.size] * t).sum(-1) + total // 2
        assert acc.min() >= 0 and acc.max() < 2 ** 31
        out[..., j] = acc // total
    assert out.min() >= 0 and out.max() <= 255
    return out


def resize_u8(src, out_w: int, out_h: int, flip: bool = False) -> np.ndarray:
    """(3, h, w) uint8 -> (3, out_h, out_w) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[0] == 3
    mid = axis_pass(src.astype(np.int64), out_w)                      # (3, h, out_w), bytes
    if flip:
        mid = mid[:, :, ::-1]
    out = axis_pass(mid.swapaxes(1, 2), out_h).swapaxes(1, 2)         # (3, out_h, out_w)
    return np.ascontiguousarray(out.astype(np.uint8))


def resize(src, out_w: int, out_h: int, flip: bool = False, dtype=np.uint8, a=1.0, b=0.0) -> np.ndarray:
    """The output's bit patterns: uint8 bytes, or the uint16 / uint32 patterns
    of the float16 / float32 planes fma(float(u8), a[c], b[c])."""
    u8 = resize_u8(src, out_w, out_h, flip)
    return u8 if np.dtype(dtype) == np.uint8 else norm_model.apply(u8, a, b, dtype)
