"""numpy model of the filter stage (include/hjd.h, hjd_conv_filter): a small
separable filter with a blend against the centre pixel on a planar uint8 RGB
image, u8 = clamp((a (x << 24) + b S + 2^35) >> 36, 0, 255).  Everything is
int64 with a flooring shift, and the widths the kernel relies on -- S in uint32,
|T| < 2^53 -- are asserted on the values actually formed.  Float outputs are
norm_model.apply of the bytes."""
import numpy as np

import norm_model

KEEP, REFLECT, REPLICATE = 0, 1, 2
MAX_RADIUS, MAX_GAIN = 11, 1 << 20


def record(kh, kv, a, b, border):
    """A filter as the model takes it: a dict of Python ints and two tap lists of odd length."""
    kh, kv = [int(v) for v in kh], [int(v) for v in kv]
    assert len(kh) % 2 == 1 and len(kv) % 2 == 1
    return {"rx": len(kh) // 2, "ry": len(kv) // 2, "border": int(border), "a": int(a), "b": int(b), "kh": kh, "kv": kv}


IDENTITY = record([4096], [4096], 4096, 0, KEEP)


def from_numpy(f):
    """The model's dict of a hjd_conv_filter numpy record (backend.conv_filter and its kin)."""
    rx, ry = int(f["rx"]), int(f["ry"])
    assert not f["kh"][2 * rx + 1:].any() and not f["kv"][2 * ry + 1:].any()
    return record(f["kh"][:2 * rx + 1], f["kv"][:2 * ry + 1], f["a"], f["b"], f["border"])


def legal(f, w, h):
    """What hjd_conv_check demands of a filter for an image of w x h."""
    return (0 <= f["rx"] <= MAX_RADIUS and 0 <= f["ry"] <= MAX_RADIUS and f["border"] in (KEEP, REFLECT, REPLICATE) and
            (f["border"] != REFLECT or (f["rx"] < w and f["ry"] < h)) and
            all(1 <= sum(k) <= 4096 and min(k) >= 0 for k in (f["kh"], f["kv"])) and abs(f["a"]) <= MAX_GAIN and abs(f["b"]) <= MAX_GAIN)


def _index(n, r, border):
    """(n + 2 r) source indices of the positions -r .. n - 1 + r of an axis."""
    i = np.arange(-r, n + r, dtype=np.int64)
    if border == REFLECT:
        assert r < n
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)   # REPLICATE; KEEP never uses what it reads outside


def conv_u8(src, f) -> np.ndarray:
    """(3, h, w) uint8 -> (3, h, w) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[0] == 3
    _, h, w = src.shape
    assert legal(f, w, h), (f, w, h)
    rx, ry, border = f["rx"], f["ry"], f["border"]
    x = src.astype(np.int64)
    padded = x[:, _index(h, ry, border)][:, :, _index(w, rx, border)]   # (3, h + 2 ry, w + 2 rx)
    rows = sum(k * padded[:, :, p:p + w] for p, k in enumerate(f["kh"]))   # the row sums: <= 255 * 4096
    assert rows.max() <= 255 * 4096
    S = sum(k * rows[:, q:q + h, :] for q, k in enumerate(f["kv"]))
    assert 0 <= S.min() and S.max() <= 255 << 24 and S.max() < 2 ** 32   # uint32 (and, at 255 << 24, not int32)
    T = f["a"] * (x << 24) + f["b"] * S
    assert np.abs(T).max() < 2 ** 53
    u8 = np.clip((T + (1 << 35)) >> 36, 0, 255)   # numpy's >> on int64 is arithmetic: a floor
    if border == KEEP:
        j, i = np.arange(w), np.arange(h)
        band = ((i < ry) | (i >= h - ry))[:, None] | ((j < rx) | (j >= w - rx))[None, :]
        u8 = np.where(band[None], x, u8)
    return u8.astype(np.uint8)


def conv(src, f, dtype=np.uint8, a=None, b=None) -> np.ndarray:
    """conv_u8, then for float16 / float32 the normalisation: bit patterns (uint16 / uint32)."""
    u8 = conv_u8(src, f)
    return u8 if np.dtype(dtype) == np.uint8 else norm_model.apply(u8, a, b, np.dtype(dtype))
