"""The affine warp without a GPU: the numpy model (warp_model.py) against
torch's grid_sample within a derived bound, the laws of the definition (crop,
flips, the eight orientations, all-fill, a 1 x 1 source), hjd_warp_roi against
the brute-force box of the clamped taps, hjd_warp_orient against composing by
hand, warp_xform against affine_grid, hjd_warp_check's refusals and the
interfaces."""
import ctypes
import functools
import glob
import inspect
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import orient_model as OM
import warp_model as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 65536
# Derived, not measured: truncating fx, fy to 11 bits moves the sampled
# position by less than 1/2048 pixel per axis, bilinear interpolation of bytes
# is 255-Lipschitz per axis, and the one rounding adds 0.5.
BOUND = 0.5 + 2 * 255 / 2048 + 1e-6
# src (w, h), out (w, h), angle, zoom
CASES = [((37, 29), (24, 16), 30.0, 1.3), ((64, 48), (40, 40), -75.0, 0.8), ((9, 200), (17, 13), 10.0, 2.0),
         ((80, 40), (33, 50), 180.0, 1.0), ((5, 3), (16, 8), 45.0, 0.3), ((300, 257), (224, 224), 15.0, 1.2)]


@functools.lru_cache(maxsize=None)
def _src(w, h, kind="random"):
    if kind == "random":
        a = np.random.default_rng(1000 * w + h).integers(0, 256, (3, h, w), dtype=np.uint8)
    else:   # a checkerboard of single pixels: the steepest bilinear surface there is
        i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        a = np.ascontiguousarray(np.broadcast_to((((i + j) & 1) * 255).astype(np.uint8), (3, h, w)))
    a.setflags(write=False)
    return a


# ---- the model against torch ----------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "checker"])
@pytest.mark.parametrize("replicate", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}")
def test_model_vs_grid_sample(hjd, case, replicate, kind):
    import torch
    (w, h), (wo, ho), angle, zoom = case
    m = hjd.warp_xform(w, h, wo, ho, angle=angle, zoom=zoom)
    src = _src(w, h, kind)
    got = W.warp_u8(src, m, wo, ho, 0, W.REPLICATE if replicate else 0)
    # the model's own positions, so that the matrix's quantisation is not in the comparison
    X, Y = W.positions(m, wo, ho)
    gx = (2 * (X / 65536.0 + 0.5) / w) - 1
    gy = (2 * (Y / 65536.0 + 0.5) / h) - 1
    grid = torch.from_numpy(np.stack([gx, gy], -1)[None])
    ref = torch.nn.functional.grid_sample(torch.from_numpy(src.astype(np.float64))[None], grid, mode="bilinear",
                                          padding_mode="border" if replicate else "zeros", align_corners=False)[0].numpy()
    worst = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{w}x{h} -> {wo}x{ho} angle {angle} zoom {zoom} {kind} replicate {replicate}: max |model - grid_sample| = "
          f"{worst:.4f} (bound {BOUND:.4f})")
    assert worst <= BOUND


# ---- the laws ---------------------------------------------------------------------
def test_crop_and_flips_byte_for_byte():
    w, h = 37, 29
    src = _src(w, h)
    for tx, ty, cw, ch in ((0, 0, w, h), (5, 3, 24, 16), (36, 28, 1, 1)):
        m = [ONE, 0, tx << 16, 0, ONE, ty << 16]
        for flags in (0, W.REPLICATE):
            np.testing.assert_array_equal(W.warp_u8(src, m, cw, ch, 0x123456, flags), src[:, ty:ty + ch, tx:tx + cw])
    np.testing.assert_array_equal(W.warp_u8(src, [-ONE, 0, (w - 1) << 16, 0, ONE, 0], w, h), src[:, :, ::-1])
    np.testing.assert_array_equal(W.warp_u8(src, [ONE, 0, 0, 0, -ONE, (h - 1) << 16], w, h), src[:, ::-1, :])
    np.testing.assert_array_equal(W.warp_u8(src, [0, ONE, 0, -ONE, 0, (h - 1) << 16], h, w), OM.orient(src, 6))


@pytest.mark.parametrize("o", range(1, 9))
def test_every_orientation_is_an_integer_matrix(hjd, o):
    w, h = 9, 6
    src = _src(w, h)
    dw, dh = OM.oriented_size(w, h, o)
    m = W.orient_matrix(o, w, h)
    np.testing.assert_array_equal(W.warp_u8(src, m, dw, dh, 0xFF00FF), OM.orient(src, o))
    # hjd_warp_orient of the identity is that matrix, and of any matrix the composition by hand
    assert hjd.warp_orient(W.IDENTITY, w, h, o) == m
    rng = np.random.default_rng(o)
    for _ in range(20):
        k = [int(v) for v in rng.integers(-(1 << 24), 1 << 24, 6)]
        assert hjd.warp_orient(k, w, h, o) == W.compose_orient(k, w, h, o)
    # integer translations: the oriented warp is the warp of the oriented image, exactly
    k = [ONE, 0, 2 << 16, 0, ONE, -(1 << 16)]
    np.testing.assert_array_equal(W.warp_u8(src, hjd.warp_orient(k, w, h, o), 7, 8, 0x0A0B0C),
                                  W.warp_u8(OM.orient(src, o), k, 7, 8, 0x0A0B0C))


def test_outside_one_pixel_and_fill():
    src = _src(5, 3)
    fill = 0x11C0FE
    planes = np.array([0x11, 0xC0, 0xFE], np.uint8)[:, None, None]
    for m in ([ONE, 0, 7 << 16, 0, ONE, 0], [ONE, 0, 0, 0, ONE, -(40 << 16)], [3 * ONE, ONE // 3, -(900 << 16), 7, ONE, 5]):
        out = W.warp_u8(src, m, 16, 8, fill)
        np.testing.assert_array_equal(out, np.broadcast_to(planes, out.shape))   # wholly outside: all fill
    # replicate, wholly to the right of the image: every pixel is the last column's
    out = W.warp_u8(src, [ONE, 0, 7 << 16, 0, ONE, 0], 4, 3, fill, W.REPLICATE)
    np.testing.assert_array_equal(out, np.broadcast_to(src[:, :, 4:5], out.shape))
    # a 1 x 1 source: replicate gives its colour everywhere, fill blends towards the fill colour around it
    one = np.array([[[200]], [[100]], [[0]]], np.uint8)
    m = [ONE // 2, 0, -(1 << 16), 0, ONE // 2, -(1 << 16)]   # output (2, 2) is the pixel, half a pixel per step
    np.testing.assert_array_equal(W.warp_u8(one, m, 6, 6, fill, W.REPLICATE), np.broadcast_to(one, (3, 6, 6)))
    out = W.warp_u8(one, m, 6, 6, fill)
    assert (out[:, 2, 2] == one[:, 0, 0]).all() and (out[:, 0, 0] == planes[:, 0, 0]).all()
    # half-way between the pixel and the fill: (200 + 0x11) / 2 rounded once, per channel
    assert out[0, 2, 3] == (200 * 1024 * 2048 + 0x11 * 1024 * 2048 + (1 << 21)) >> 22
    assert out[2, 2, 3] == (0xFE * 1024 * 2048 + (1 << 21)) >> 22


# ---- hjd_warp_roi --------------------------------------------------------------------
ROI_MAPS = [  # (frame w, h), (out w, h), matrix
    ((64, 48), (24, 16), None),                                                 # filled in: rotated 30 degrees
    ((64, 48), (24, 16), [ONE, 0, 5 << 16, 0, ONE, 3 << 16]),                   # a crop: X whole, the second tap included
    ((64, 48), (24, 16), [2 * ONE, 0, -(9 << 16) + 77, 0, 2 * ONE, 40 << 16]),  # past the left and the bottom edge
    ((64, 48), (10, 7), [ONE, 0, 100 << 16, 0, ONE, 3 << 16]),                  # wholly to the right
    ((64, 48), (10, 7), [ONE, 0, -(100 << 16), 0, ONE, -(100 << 16)]),          # wholly above and to the left
    ((5, 3), (16, 8), [ONE // 3, -ONE // 5, 1 << 16, ONE // 7, ONE // 3, 0]),
    ((1, 1), (4, 4), [ONE, 0, 0, 0, ONE, 0]),
]


@pytest.mark.parametrize("k", range(len(ROI_MAPS)))
def test_warp_roi_vs_brute_force_and_crop_equals_frame(hjd, k):
    (w, h), (wo, ho), m = ROI_MAPS[k]
    if m is None:
        m = hjd.warp_xform(w, h, wo, ho, angle=30.0, zoom=1.7)
    roi = hjd.warp_roi(w, h, m, wo, ho)
    x, y, rw, rh = roi
    assert rw >= 1 and rh >= 1 and x >= 0 and y >= 0 and x + rw <= w and y + rh <= h
    # the smallest rectangle: the box of all taps (a second tap of weight 0 is a tap)
    assert roi == W.clamped_tap_box(w, h, m, wo, ho)
    src = _src(w, h)
    crop = np.ascontiguousarray(src[:, y:y + rh, x:x + rw])
    for flags in (0, W.REPLICATE):
        np.testing.assert_array_equal(W.warp_u8(crop, W.shifted(m, x, y), wo, ho, 0x804020, flags),
                                      W.warp_u8(src, m, wo, ho, 0x804020, flags))


def test_warp_roi_refusals(hjd):
    from ocljpegdecoder_amd._lib import HjdError
    lib = hjd._lib.load()
    m = (ctypes.c_int32 * 6)(*W.IDENTITY)
    assert lib.hjd_warp_roi(8, 8, None, 4, 4, None) == -1 and "NULL" in hjd._lib.error_string()
    for args, match in (((0, 8, W.IDENTITY, 4, 4), "frame size"), ((8, -1, W.IDENTITY, 4, 4), "frame size"),
                        ((8, 8, W.IDENTITY, 0, 4), "output size"), ((8, 8, W.IDENTITY, 4, 16385), "output size")):
        with pytest.raises(HjdError, match=match) as e:
            hjd.warp_roi(*args)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        hjd.warp_roi(8, 8, [1, 2, 3], 4, 4)
    with pytest.raises(ValueError):
        hjd.warp_roi(8, 8, [1 << 31, 0, 0, 0, 1, 0], 4, 4)
    r = hjd._lib.HjdRect()
    # a frame larger than a warp's source may be: the rectangle is what counts (here with the weight-0 second taps)
    assert lib.hjd_warp_roi(70000, 70000, m, 16384, 16384, ctypes.byref(r)) == 0 and (r.w, r.h) == (16385, 16385)


# ---- hjd_warp_orient ------------------------------------------------------------------
def test_warp_orient_overflow_and_refusals(hjd):
    from ocljpegdecoder_amd._lib import HjdError
    big = [-(1 << 31), 0, 0, 0, ONE, 0]
    assert hjd.warp_orient(big, 8, 8, 1) == big
    with pytest.raises(HjdError, match=r"m\[0\].*leaves int32") as e:
        hjd.warp_orient(big, 8, 8, 2)            # -(-2^31)
    assert e.value.code == -1
    with pytest.raises(HjdError, match=r"m\[2\].*leaves int32"):
        hjd.warp_orient([ONE, 0, -(1 << 30) - (1 << 17), 0, ONE, 0], 16384, 8, 2)   # ((w - 1) << 16) + 2^30 + 2^17
    assert hjd.warp_orient([ONE, 0, -(1 << 30), 0, ONE, 0], 16384, 8, 2)[2] == (16383 << 16) + (1 << 30)
    with pytest.raises(HjdError, match=r"m\[5\].*leaves int32"):
        hjd.warp_orient([ONE, 0, -(1 << 30) - (1 << 17), 0, ONE, 0], 8, 16384, 6)   # row Y of 6 is h - 1 - X
    for o in (0, 9, -1):
        with pytest.raises(HjdError, match="orientation"):
            hjd.warp_orient(W.IDENTITY, 8, 8, o)
    with pytest.raises(HjdError, match="stored size"):
        hjd.warp_orient(W.IDENTITY, 0, 8, 1)
    lib = hjd._lib.load()
    assert lib.hjd_warp_orient(None, 8, 8, 1, None) == -1


# ---- warp_xform -------------------------------------------------------------------------
def test_warp_xform_exact_cases(hjd):
    assert hjd.warp_xform(37, 29, 37, 29) == [ONE, 0, 0, 0, ONE, 0]
    assert hjd.warp_xform(37, 29, 37, 29, hflip=True) == [-ONE, 0, 36 << 16, 0, ONE, 0]
    n = 16
    assert hjd.warp_xform(n, n, n, n, angle=90.0) == W.orient_matrix(8, n, n)     # counter-clockwise
    assert hjd.warp_xform(n, n, n, n, angle=-90.0) == W.orient_matrix(6, n, n)
    assert hjd.warp_xform(n, n, n, n, angle=180.0) == W.orient_matrix(3, n, n)
    assert hjd.warp_xform(64, 48, 32, 24, zoom=2.0) == [2 * ONE, 0, ONE // 2, 0, 2 * ONE, ONE // 2]   # the resize's taps
    assert hjd.warp_xform(64, 48, 8, 8, center=(10.5, 20.5)) == [ONE, 0, (10 - 4) * ONE + ONE // 2, 0, ONE,
                                                                 (20 - 4) * ONE + ONE // 2]
    assert all(isinstance(v, int) for v in hjd.warp_xform(37, 29, 24, 16, angle=12.5, zoom=1.1, shear=(5.0, -3.0)))
    with pytest.raises(ValueError, match="int32"):
        hjd.warp_xform(16384, 16384, 8, 8, zoom=40000.0)
    with pytest.raises(ValueError, match="int32"):
        hjd.warp_xform(8, 8, 8, 8, center=(40000.0, 0.0))


@pytest.mark.parametrize("angle,zoom,shear,hflip", [(30.0, 1.3, (0.0, 0.0), False), (-75.0, 0.8, (0.0, 0.0), True),
                                                    (10.0, 2.0, (12.0, 0.0), False), (200.0, 0.5, (-8.0, 15.0), False)])
def test_warp_xform_vs_affine_grid(hjd, angle, zoom, shear, hflip):
    """The positions of the integer matrix against affine_grid's of the real
    one.  theta is built here from the parts -- a rotation by the angle
    (counter-clockwise on the screen, y down), the shears as an image
    library's affine composes them (rotation . shear_y . shear_x, inverted),
    the zoom and the flip -- in normalised coordinates."""
    import torch
    w, h, wo, ho = 300, 257, 224, 200
    m = hjd.warp_xform(w, h, wo, ho, angle=angle, zoom=zoom, shear=shear, hflip=hflip)
    t, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    rot = np.array([[math.cos(t), math.sin(t)], [-math.sin(t), math.cos(t)]])      # the picture's forward turn (y down)
    shy = np.array([[1.0, 0.0], [-math.tan(sy), 1.0]])
    shx = np.array([[1.0, -math.tan(sx)], [0.0, 1.0]])
    A = zoom * np.linalg.inv(rot @ shy @ shx)
    if hflip:
        A = A @ np.diag([-1.0, 1.0])
    theta = np.array([[A[0, 0] * wo / w, A[0, 1] * ho / w, 0.0], [A[1, 0] * wo / h, A[1, 1] * ho / h, 0.0]])
    g = torch.nn.functional.affine_grid(torch.from_numpy(theta)[None], (1, 1, ho, wo), align_corners=False)[0].numpy()
    rx = ((g[..., 0] + 1) * w - 1) / 2     # source pixel indices, as grid_sample unnormalises them
    ry = ((g[..., 1] + 1) * h - 1) / 2
    X, Y = W.positions(m, wo, ho)
    i, j = np.meshgrid(np.arange(ho), np.arange(wo), indexing="ij")
    tol = (j + i + 1) * 2.0 ** -16
    assert (np.abs(X / 65536.0 - rx) <= tol).all() and (np.abs(Y / 65536.0 - ry) <= tol).all()


# ---- hjd_warp_check -----------------------------------------------------------------------
PLANAR, F16, F32 = 3, 5, 6


def _item(hjd, src=0x10000, dst=0x20000, w=37, h=29, pitch=37, flags=0, m=W.IDENTITY, fill=0, reserved=0):
    return hjd._lib.HjdWarpItem(src, dst, w, h, pitch, flags, (ctypes.c_int32 * 6)(*m), fill, reserved)


def _check(hjd, items, n, wo, ho, pitch, fmt):
    lib = hjd._lib.load()
    arr = (hjd._lib.HjdWarpItem * len(items))(*items)
    return lib.hjd_warp_check(arr, n, wo, ho, pitch, fmt), hjd._lib.error_string()


def _refused(hjd, match, items, n=None, wo=24, ho=16, pitch=24, fmt=PLANAR):
    rc, msg = _check(hjd, items, len(items) if n is None else n, wo, ho, pitch, fmt)
    assert rc == -1, (rc, msg)   # HJD_E_INVALID
    assert re.search(match, msg), msg


def test_warp_check(hjd):
    lib = hjd._lib.load()
    ok = _item(hjd)
    wild = _item(hjd, src=0x10001, dst=0x30001, w=5, h=3, pitch=7, flags=1, m=[-(1 << 31), (1 << 31) - 1, 5, -7, 0, 1 << 30],
                 fill=0xFFFFFF)
    assert _check(hjd, [ok, wild], 2, 24, 16, 24, PLANAR)[0] == 0
    assert _check(hjd, [ok], 1, 24, 16, 48, F16)[0] == 0 and _check(hjd, [ok], 1, 23, 7, 92, F32)[0] == 0
    assert _check(hjd, [_item(hjd, w=16384, h=16384, pitch=16384)], 1, 16384, 16384, 16384, PLANAR)[0] == 0
    assert _check(hjd, [_item(hjd, w=1, h=1, pitch=1)], 1, 1, 1, 1, PLANAR)[0] == 0
    assert lib.hjd_warp_check(None, 1, 24, 16, 24, PLANAR) == -1 and "NULL" in hjd._lib.error_string()
    for n in (0, -1, (1 << 20) + 1):
        _refused(hjd, "n = ", [ok], n=n)
    _refused(hjd, "item 0: src or dst is NULL", [_item(hjd, src=0)])
    _refused(hjd, "item 1: src or dst is NULL", [ok, _item(hjd, dst=0)])
    for bad in (0, -3, 16385):
        _refused(hjd, "item 0: source size", [_item(hjd, w=bad, pitch=1 << 20)])
        _refused(hjd, "item 1: source size", [ok, _item(hjd, h=bad)])
        _refused(hjd, "output size", [ok], wo=bad, pitch=1 << 20)
        _refused(hjd, "output size", [ok], ho=bad)
    _refused(hjd, "src_pitch", [_item(hjd, pitch=36)])
    for flags in (2, 3, 0x100, -1):
        _refused(hjd, "item 0: unknown flag bits", [_item(hjd, flags=flags)])
    _refused(hjd, "item 1: fill", [ok, _item(hjd, fill=0x1000000)])
    _refused(hjd, "fill", [_item(hjd, fill=0xFFFFFFFF)])
    _refused(hjd, "item 0: reserved", [_item(hjd, reserved=1)])
    _refused(hjd, "out_pitch", [ok], pitch=23)
    _refused(hjd, "out_pitch", [ok], pitch=46, fmt=F16)      # < 2 * 24
    _refused(hjd, "out_pitch", [ok], pitch=49, fmt=F16)      # not a multiple of 2
    _refused(hjd, "out_pitch", [ok], pitch=98, fmt=F32)      # not a multiple of 4
    _refused(hjd, "dst must be a multiple", [_item(hjd, dst=0x20001)], pitch=48, fmt=F16)
    _refused(hjd, "dst must be a multiple", [_item(hjd, dst=0x20002)], pitch=96, fmt=F32)
    assert _check(hjd, [_item(hjd, dst=0x20001)], 1, 24, 16, 24, PLANAR)[0] == 0   # bytes: any dst
    for fmt in (0, 1, 2, 4, 7, -1):
        _refused(hjd, "output format", [ok], fmt=fmt)


# ---- interfaces ------------------------------------------------------------------------------
def test_warp_entry_points_are_bound(hjd):
    """Declared in the headers, exported, bound in _lib.py; NULL objects are refused without a device."""
    lib = hjd._lib.load()
    for name in ("hjd_warp_check", "hjd_warp_create", "hjd_warp_set_normalize", "hjd_warp_launch", "hjd_warp_destroy",
                 "hjd_warp_roi", "hjd_warp_orient", "hjd_debug_warp_launch_form", "hjd_gdec_decode_warped"):
        assert name in hjd._lib.SIGNATURES and getattr(lib, name).argtypes == hjd._lib.SIGNATURES[name][1]
        for header in ("hjd.h", "hjd_host.h"):
            if re.search(rf"\b{name}\(", open(os.path.join(REPO, "include", header)).read()):
                break
        else:
            raise AssertionError(f"{name} is in no header")
    header = open(os.path.join(REPO, "include", "hjd.h")).read()
    assert re.search(r"typedef struct hjd_warp_item \{[^}]*int32_t m\[6\];[^}]*uint32_t fill;[^}]*\} hjd_warp_item;", header)
    assert "HJD_WARP_REPLICATE = 1" in header and "#define HJD_ABI_VERSION 1" in header
    assert ctypes.sizeof(hjd._lib.HjdWarpItem) == 64 and hjd._lib.HjdWarpItem.m.offset == 32
    assert hjd._lib.HjdWarpItem.fill.offset == 56
    assert lib.hjd_warp_launch(None, None) == -1
    assert lib.hjd_debug_warp_launch_form(None, 1, None) == -1
    one = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.hjd_warp_set_normalize(None, one, one) == -1
    assert lib.hjd_warp_destroy(None) == 0
    assert lib.hjd_warp_create(None, None, 1, 8, 8, 8, PLANAR, None) == -1
    assert lib.hjd_gdec_decode_warped(None, None, None, 1, None, None, None, None, None, 8, 8, 8, None) == -1
    # Python
    assert hjd.WARP_REPLICATE == 1
    for name in ("Warp", "WARP_REPLICATE", "warp_roi", "warp_orient", "warp_xform"):
        assert name in hjd.__all__ and hasattr(hjd, name)
    assert list(inspect.signature(hjd.Warp.__init__).parameters) == ["self", "ctx", "srcs", "out", "xforms", "fills",
                                                                     "replicate", "normalize"]
    for method in ("launch", "set_normalize", "close"):
        assert callable(getattr(hjd.Warp, method))
    assert list(inspect.signature(hjd.warp_roi).parameters) == ["width", "height", "xform", "out_w", "out_h"]
    assert list(inspect.signature(hjd.warp_orient).parameters) == ["xform", "stored_w", "stored_h", "orientation"]
    p = inspect.signature(hjd.warp_xform).parameters
    assert list(p) == ["src_w", "src_h", "out_w", "out_h", "angle", "zoom", "shear", "center", "hflip"]
    assert (p["angle"].default, p["zoom"].default, p["shear"].default, p["center"].default, p["hflip"].default) == \
        (0.0, 1.0, (0.0, 0.0), None, False)
    assert "cos(r - sy)" in hjd.warp_xform.__doc__            # the formula is written down
    p = inspect.signature(hjd.GpuDecoder.decode_warped).parameters
    assert list(p) == ["self", "datas", "out", "xforms", "stream", "fills", "replicate", "apply_exif_orientation",
                       "orientations"]
    p = inspect.signature(hjd.GpuDecoder.decode_rgb_warped).parameters
    assert list(p) == ["self", "datas", "size", "xforms", "fill", "replicate", "out", "stream", "scale", "dtype", "mean",
                       "std", "apply_exif_orientation", "orientations"]
    assert p["fill"].default == 0 and p["replicate"].default is False and p["scale"].default == 1
    assert p["apply_exif_orientation"].default is False and p["orientations"].default is None


def test_warp_kernels_in_the_built_library(hjd):
    sys.path.insert(0, os.path.join(REPO, "tools", "check"))
    import d16_order
    if not os.path.exists(d16_order.LLVM_OBJDUMP):
        pytest.skip("llvm-objdump is not installed")
    lib_path = os.path.join(REPO, "ocljpegdecoder_amd", "lib", "libhjd.so")
    tmp = tempfile.mkdtemp(prefix="hjd_warp_")
    try:
        dst = os.path.join(tmp, os.path.basename(lib_path))
        shutil.copy(lib_path, dst)
        subprocess.run([d16_order.LLVM_OBJDUMP, "--offloading", dst], cwd=tmp, check=True, capture_output=True)
        objs = sorted(glob.glob(os.path.join(tmp, f"*{d16_order.ARCH}*")))
        assert objs
        syms = "\n".join(subprocess.run([d16_order.LLVM_OBJDUMP, "-t", "-C", co], check=True, capture_output=True,
                                        text=True).stdout for co in objs)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert set(re.findall(r"hjd::warp_kernel<(\d+)>\(", syms)) == {"0", "1", "2"}
