"""numpy model of the scaled decode (include/hjd.h, hjd_plan_create_scaled),
built from the oracle's primitives.  TEST INFRASTRUCTURE ONLY.

For scale s in {1, 2, 4, 8}: the oracle's IDCT samples of every block (after
its [-256,255] clamp, before the luma level shift) are reduced to (8/s)x(8/s)
box means m = (sum + s*s/2) >> (2 log2 s) (floor); the scaled blocks form the
component planes in MCU order, chroma is replicated nearest by the sampling's
factors on the scaled grids, the oracle's colour conversion is applied and the
result is cropped to ceil(W/s) x ceil(H/s).
"""
import numpy as np

import oracle_py as O


def scaled_size(width, height, scale):
    return -(-width // scale), -(-height // scale)


def box_means(samples, scale):
    """(N, 64) int32 IDCT samples -> (N, 8/s, 8/s) box means."""
    n = 8 // scale
    lg = {1: 0, 2: 1, 4: 2, 8: 3}[scale]
    b = np.asarray(samples, dtype=np.int64).reshape(-1, n, scale, n, scale)
    return ((b.sum(axis=(2, 4)) + scale * scale // 2) >> (2 * lg)).astype(np.int32)


def scaled_planes(coefs, qt, width, height, sampling, scale):
    """The scaled component planes (Y, U, V) over the whole MCU grid, chroma
    already replicated to the luma grid (gray: U = V = 0)."""
    pw, ph, bpm, nluma = O.GEOM[sampling]
    mw, mh = (width - 1) // pw + 1, (height - 1) // ph + 1
    n = 8 // scale
    hb, vb = pw // 8, ph // 8                       # luma blocks per MCU, across and down
    assert hb * vb == nluma
    nat = O.dequant_natural(coefs, qt, sampling)
    m = box_means(O.idct_blocks(nat), scale).reshape(mh, mw, bpm, n, n)
    comp = O.block_components(sampling, bpm)
    assert list(comp[:nluma]) == [0] * nluma
    # luma: the MCU's blocks in raster order (vb rows of hb blocks)
    luma = m[:, :, :nluma].reshape(mh, mw, vb, hb, n, n).transpose(0, 2, 4, 1, 3, 5).reshape(mh * vb * n, mw * hb * n)
    if bpm == nluma:
        zero = np.zeros_like(luma)
        return luma, zero, zero
    planes = [luma]
    for c in (1, 2):
        k = nluma + c - 1
        assert comp[k] == c
        p = m[:, :, k].transpose(0, 2, 1, 3).reshape(mh * n, mw * n)
        planes.append(np.repeat(np.repeat(p, vb, axis=0), hb, axis=1))   # nearest, by the sampling's factors
    return tuple(planes)


def decode_scaled(coefs, qt, width, height, sampling, scale):
    """(H', W') uint32 BGRX words of the scaled decode."""
    y, u, v = scaled_planes(coefs, qt, width, height, sampling, scale)
    sw, sh = scaled_size(width, height, scale)
    return np.ascontiguousarray(O.yuv_to_bgrx(y, u, v)[:sh, :sw])
