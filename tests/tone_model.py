"""numpy model of the tone stage (include/hjd.h, hjd_tone_curve): a mode and a
3 x 256 table applied to a planar uint8 RGB image, u8_c = lut[c][D_c[x_c]].
Histograms are taken over the image's own pixels (the array handed in has no
padding), everything is int64 with floor division, and the widths the kernel
relies on -- uint32 counts and sums -- are asserted on the values actually
formed.  Float outputs are norm_model.apply of the bytes."""
import numpy as np

import norm_model

TABLE, AUTOCONTRAST, EQUALIZE = 0, 1, 2
IDENTITY = np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def histogram(src) -> np.ndarray:
    """h: (3, 256) int64, h[c][v] the number of pixels of plane c whose byte is v."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[0] == 3
    assert src.shape[1] * src.shape[2] <= 2 ** 28
    return np.stack([np.bincount(src[c].ravel(), minlength=256) for c in range(3)]).astype(np.int64)


def data_curve(mode, hist) -> np.ndarray:
    """D: (3, 256) int64, the data curve of each channel from its histogram (256 int64 counts)."""
    hist = np.asarray(hist, np.int64)
    assert hist.shape == (3, 256) and hist.min() >= 0 and mode in (TABLE, AUTOCONTRAST, EQUALIZE)
    v = np.arange(256, dtype=np.int64)
    out = np.empty((3, 256), np.int64)
    for c in range(3):
        h = hist[c]
        n = int(h.sum())
        assert n <= 2 ** 28
        full = np.flatnonzero(h)
        out[c] = v
        if mode == TABLE or len(full) < 2:
            continue
        lo, hi = int(full[0]), int(full[-1])
        if mode == AUTOCONTRAST:
            out[c] = np.where(v <= lo, 0, np.where(v >= hi, 255, 255 * (v - lo) // (hi - lo)))
        else:
            step = (n - int(h[hi])) // 255
            if step == 0:
                continue
            below = np.concatenate(([0], np.cumsum(h)[:-1]))   # the sum over k < v
            acc = step // 2 + below
            assert acc.max() < 2 ** 28 + 2 ** 27                # fits uint32
            out[c] = np.minimum(255, acc // step)
    assert out.min() >= 0 and out.max() <= 255
    return out


def composed(mode, hist, lut=IDENTITY) -> np.ndarray:
    """(3, 256) uint8: v -> lut[c][D_c[v]], what hjd_tone_curve_from_histogram and tone_lut_kernel write."""
    lut = np.asarray(lut)
    assert lut.shape == (3, 256) and lut.dtype == np.uint8
    return np.take_along_axis(lut, data_curve(mode, hist), axis=1)


def tone_u8(src, mode=TABLE, lut=IDENTITY, hist_read=None) -> np.ndarray:
    """(3, h, w) uint8 -> (3, h, w) uint8.  A mode-0 record never reads a histogram (hist_read, a list, says whether)."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[0] == 3
    lut = np.asarray(lut)
    assert lut.shape == (3, 256) and lut.dtype == np.uint8
    if mode == TABLE:
        table = lut
    else:
        if hist_read is not None:
            hist_read.append(True)
        table = composed(mode, histogram(src), lut)
    return np.stack([table[c][src[c]] for c in range(3)])


def tone(src, mode=TABLE, lut=IDENTITY, dtype=np.uint8, a=None, b=None) -> np.ndarray:
    """tone_u8, then for float16 / float32 the normalisation: bit patterns (uint16 / uint32)."""
    u8 = tone_u8(src, mode, lut)
    return u8 if np.dtype(dtype) == np.uint8 else norm_model.apply(u8, a, b, np.dtype(dtype))
