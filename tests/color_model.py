"""numpy model of the colour stage (include/hjd.h, hjd_color_item): a record of
21 Q12 integers m[9], p[9], t[3] applied to a planar uint8 RGB image, with the
image's channel means in Q8.  Everything is int64 (>> on signed values is
floor), and the widths the kernel relies on -- 24-bit multiplies, an int32
accumulator, 64 bits for T only -- are asserted on the values actually formed.
Float outputs are norm_model.apply of the bytes.

The error bound (derived, not measured).  The real-valued map of the integer
record is y_c = (m[c] . x + p[c] . xbar) / 4096 + t[c] / 4096 with xbar = S / N.

  1  mq_k = floor((256 S_k + (N >> 1)) / N) is 256 xbar_k rounded to nearest:
     z = 256 S_k / N is a multiple of 1 / N and d = (N >> 1) / N lies in
     [(N - 1) / 2N, 1 / 2], so floor(z + d) - z lies in [d - (N - 1) / N, d],
     inside [-1/2, 1/2].  mq_k / 256 is within 2^-9 of xbar_k, and p[c] . mq / 256
     within sum_k |p[c][k]| * 2^-9 Q12 units of p[c] . xbar -- in grey levels
     (sum_k |p[c][k]| / 4096) * 2^-9.
  2  (v + 128) >> 8 is v / 256 rounded to nearest: at most half a Q12 unit,
     2^-13 grey level.
  3  (a + 2048) >> 12 is a / 4096 rounded to nearest (ties up): at most 0.5.
     clamp(round(v), 0, 255) == round(clamp(v, 0, 255)) for integer limits, and
     the clamp is 1-Lipschitz, so the errors of 1 and 2 pass through it unamplified.

Together |u8_c - clamp(y_c, 0, 255)| <= 0.5 + 2^-13 + (sum_k |p[c][k]| / 4096) * 2^-9
(bound()).  Where the integers are real coefficients rounded to nearest in
Q12, each of the 3 entries of m[c] and of p[c] is off by at most 2^-13 on a
factor of at most 255, and t[c] by 2^-13: (3 * 255 + 3 * 255 + 1) * 2^-13 more
(ROUNDED_COEFS)."""
import numpy as np

import norm_model

MAX_COEF = 32767          # HJD_COLOR_MAX_COEF
MAX_OFFSET = 1 << 23      # HJD_COLOR_MAX_OFFSET
ONE = 4096                # Q12
IDENTITY = (ONE, 0, 0, 0, ONE, 0, 0, 0, ONE) + (0,) * 12
INVERSE = (-ONE, 0, 0, 0, -ONE, 0, 0, 0, -ONE) + (0,) * 9 + (255 * ONE,) * 3
ROUNDED_COEFS = (3 * 255 + 3 * 255 + 1) * 2.0 ** -13


def split(rec):
    """(m, p, t): (3, 3), (3, 3) and (3,) int64 of a record, its ranges asserted."""
    rec = [int(v) for v in rec]
    assert len(rec) == 21
    m, p, t = (np.array(rec[:9], np.int64).reshape(3, 3), np.array(rec[9:18], np.int64).reshape(3, 3),
               np.array(rec[18:], np.int64))
    assert np.abs(m).max() <= MAX_COEF and np.abs(p).max() <= MAX_COEF and np.abs(t).max() <= MAX_OFFSET
    return m, p, t


def means_q8(src):
    """mq: the channel means of a (3, h, w) uint8 image in Q8, (3,) int64."""
    src = np.asarray(src)
    n = src.shape[1] * src.shape[2]
    s = src.reshape(3, -1).astype(np.int64).sum(axis=1)
    assert s.max() < 2 ** 36
    return (s * 256 + (n >> 1)) // n


def offsets(rec, src, sums_read=None):
    """T: (3,) int64.  A record with p = 0 never reads the sums (sums_read, a list, says whether)."""
    m, p, t = split(rec)
    if not p.any():
        return t
    if sums_read is not None:
        sums_read.append(True)
    mq = means_q8(src)
    assert 0 <= mq.min() and mq.max() <= 255 * 256
    prod = p * mq[None, :]
    assert np.abs(prod).max() < 2 ** 31            # one product fits 32 bits; their sum takes 64
    T = t + ((prod.sum(axis=1) + 128) >> 8)
    assert np.abs(T).max() < 2 ** 23 + 2 ** 25
    return T


def color_u8(src, rec) -> np.ndarray:
    """(3, h, w) uint8 -> (3, h, w) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[0] == 3
    m, _, _ = split(rec)
    T = offsets(rec, src)
    x = src.astype(np.int64)
    assert np.abs(m).max() < 2 ** 23 and x.max() < 2 ** 23              # 24-bit signed multiplies
    acc = np.einsum("ck,khw->chw", m, x) + (T + 2048)[:, None, None]
    assert np.abs(acc).max() < 2 ** 31                                  # the accumulator fits int32
    return np.clip(acc >> 12, 0, 255).astype(np.uint8)


def color(src, rec, dtype=np.uint8, a=None, b=None) -> np.ndarray:
    """color_u8, then for float16 / float32 the normalisation: bit patterns (uint16 / uint32)."""
    u8 = color_u8(src, rec)
    return u8 if np.dtype(dtype) == np.uint8 else norm_model.apply(u8, a, b, np.dtype(dtype))


def real_map(src, M, P, t):
    """The real-valued map x -> M x + P xbar + t on a (3, h, w) image, float64, not clamped."""
    x = np.asarray(src, np.float64)
    xbar = x.reshape(3, -1).mean(axis=1)
    M, P, t = np.asarray(M, np.float64), np.asarray(P, np.float64), np.asarray(t, np.float64)
    return np.einsum("ck,khw->chw", M, x) + (P @ xbar + t)[:, None, None]


def real_of_record(src, rec):
    """real_map of the integer record itself: m / 4096, p / 4096, t / 4096."""
    m, p, t = split(rec)
    return real_map(src, m / 4096.0, p / 4096.0, t / 4096.0)


def bound(rec):
    """(3,): the derived bound per output channel against clamp(real_of_record)."""
    _, p, _ = split(rec)
    return 0.5 + 2.0 ** -13 + np.abs(p).sum(axis=1) / 4096.0 * 2.0 ** -9
