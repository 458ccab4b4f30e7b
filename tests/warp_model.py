"""numpy model of the affine warp (include/hjd.h, hjd_warp_item): the inverse
map in Q16 integers, floor by arithmetic shift, the resize's 11-bit weights and
one rounding, fill or replicate outside the image.  Everything is int64 (>> on
signed values is floor), and the bounds that let the kernel keep X >> 16 and
the blend in 32 bits are asserted on the values actually formed.  Float
outputs are norm_model.apply of the bytes."""
import numpy as np

import norm_model

MAX_DIM = 16384
WEIGHT = 2048   # 11-bit weights
REPLICATE = 1   # flags bit 0

IDENTITY = (65536, 0, 0, 0, 65536, 0)


def positions(m, out_w: int, out_h: int):
    """(X, Y): the Q16 source positions of every output pixel, (out_h, out_w) int64 each."""
    assert len(m) == 6 and all(-2 ** 31 <= int(v) < 2 ** 31 for v in m)
    assert 1 <= out_w <= MAX_DIM and 1 <= out_h <= MAX_DIM
    m = [int(v) for v in m]
    i, j = np.meshgrid(np.arange(out_h, dtype=np.int64), np.arange(out_w, dtype=np.int64), indexing="ij")
    return m[0] * j + m[1] * i + m[2], m[3] * j + m[4] * i + m[5]


def taps(m, out_w: int, out_h: int):
    """(x0, y0, fx, fy) per output pixel: the first tap and the weights of the second."""
    X, Y = positions(m, out_w, out_h)
    x0, y0 = X >> 16, Y >> 16
    assert max(abs(x0).max(), abs(y0).max()) < 2 ** 31 - 1
    return x0, y0, (X & 0xffff) >> 5, (Y & 0xffff) >> 5


def warp_u8(src, m, out_w: int, out_h: int, fill: int = 0, flags: int = 0) -> np.ndarray:
    """(3, h, w) uint8 -> (3, out_h, out_w) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[0] == 3
    assert 0 <= fill <= 0xFFFFFF and flags in (0, REPLICATE)
    h, w = src.shape[1:]
    assert 1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM
    x0, y0, fx, fy = taps(m, out_w, out_h)
    s = src.astype(np.int64)
    fillc = np.array([(fill >> 16) & 255, (fill >> 8) & 255, fill & 255], np.int64)[:, None, None]

    def tap(x, y):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        v = s[:, np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]   # never an index outside the image
        return v if flags & REPLICATE else np.where(inside[None], v, fillc)

    a, b, c, d = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    acc = (a * (WEIGHT - fx) * (WEIGHT - fy) + b * fx * (WEIGHT - fy) + c * (WEIGHT - fx) * fy + d * fx * fy + (1 << 21))
    assert acc.max() < 2 ** 31 and acc.min() >= 0
    assert ((acc >> 22) <= 255).all()
    return (acc >> 22).astype(np.uint8)


def warp(src, m, out_w: int, out_h: int, fill: int = 0, flags: int = 0, dtype=np.uint8, a=1.0, b=0.0) -> np.ndarray:
    """The output's bit patterns: uint8 bytes, or the uint16 / uint32 patterns
    of the float16 / float32 planes fma(float(u8), a[c], b[c])."""
    u8 = warp_u8(src, m, out_w, out_h, fill, flags)
    return u8 if np.dtype(dtype) == np.uint8 else norm_model.apply(u8, a, b, dtype)


def clamped_tap_box(width: int, height: int, m, out_w: int, out_h: int):
    """Brute force: the bounding box (x, y, w, h) of every tap the output
    reads, each tap's coordinates clamped into the width x height frame."""
    x0, y0, _, _ = taps(m, out_w, out_h)
    xs = np.clip(np.concatenate([x0.ravel(), x0.ravel() + 1]), 0, width - 1)
    ys = np.clip(np.concatenate([y0.ravel(), y0.ravel() + 1]), 0, height - 1)
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


def shifted(m, x: int, y: int):
    """m addressing the crop whose origin is (x, y) of what m addresses."""
    return [m[0], m[1], m[2] - (x << 16), m[3], m[4], m[5] - (y << 16)]


def orient_matrix(o: int, w: int, h: int):
    """The integer matrix of orientation o on a stored w x h image, by hand
    from the table of include/hjd.h: D[i][j] = S[row][col], X = col, Y = row."""
    one, W, H = 65536, (w - 1) << 16, (h - 1) << 16
    return {1: [one, 0, 0, 0, one, 0],        # S[i][j]
            2: [-one, 0, W, 0, one, 0],       # S[i][w-1-j]
            3: [-one, 0, W, 0, -one, H],      # S[h-1-i][w-1-j]
            4: [one, 0, 0, 0, -one, H],       # S[h-1-i][j]
            5: [0, one, 0, one, 0, 0],        # S[j][i]
            6: [0, one, 0, -one, 0, H],       # S[h-1-j][i]
            7: [0, -one, W, -one, 0, H],      # S[h-1-j][w-1-i]
            8: [0, -one, W, one, 0, 0]}[o]    # S[j][w-1-i]


def compose_orient(m, w: int, h: int, o: int):
    """m on the displayed image -> the matrix on the stored w x h image:
    (X, Y) of m substituted for (j, i) in orient_matrix, in exact integers."""
    k = orient_matrix(o, w, h)
    rows = []
    for r in (k[0:3], k[3:6]):   # r[0] * X + r[1] * Y + r[2], X and Y in Q16: r[0], r[1] are +-65536 or 0
        sx, sy = r[0] // 65536, r[1] // 65536
        rows += [sx * m[0] + sy * m[3], sx * m[1] + sy * m[4], sx * m[2] + sy * m[5] + r[2]]
    return rows
