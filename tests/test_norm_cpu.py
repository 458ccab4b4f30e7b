"""Normalised float output formats, host side: norm_constants, the exact model
(tests/norm_model.py) against the float64 expression, the declarations, the
Python names and the refusals that need no device.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import norm_model as N
import oracle_py as O

MEAN, STD = N.IMAGENET_MEAN, N.IMAGENET_STD
W, H = 769, 40


def _invalid(match):
    from ocljpegdecoder_amd._lib import HjdError
    return pytest.raises(HjdError, match=match)


# ---- constants ----------------------------------------------------------------------
def test_norm_constants(hjd):
    a, b = hjd.norm_constants()
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (3,)
    assert (a == np.float32(1.0 / 255.0)).all()
    assert (b.view(np.uint32) == 0).all()            # +0
    a, b = hjd.norm_constants(MEAN, STD)
    for c in range(3):   # float64, rounded once
        assert a[c] == np.float32(1.0 / (255.0 * STD[c]))
        assert b[c] == np.float32(-MEAN[c] / STD[c])
    a, b = hjd.norm_constants(0.5, 0.25)             # scalars broadcast
    assert (a == np.float32(4.0 / 255.0)).all() and (b == np.float32(-2.0)).all()
    a, b = hjd.norm_constants(std=(1, 2, 4))
    assert (a == np.float32(1 / 255.0) / np.array([1, 2, 4], np.float32)).all() and (b.view(np.uint32) == 0).all()
    for kw in (dict(std=0.0), dict(std=(1, 0, 1)), dict(mean=float("inf")), dict(mean=float("nan")),
               dict(std=float("nan")), dict(mean=1e30, std=1e-30)):
        with pytest.raises(ValueError, match="finite"):
            hjd.norm_constants(**kw)


# ---- the model ----------------------------------------------------------------------
def test_model_vs_float64_expression(hjd):
    """Three roundings of relative 2^-24 each (a, b, the fma) bound the F32
    model's distance from (v/255 - mean)/std by 2^-22 (|v a| + |b|); F16 adds
    half an ulp of the half result."""
    a, b = hjd.norm_constants(MEAN, STD)
    t32 = N.table(a, b, np.float32).view(np.float32).astype(np.float64)
    t16 = N.table(a, b, np.float16).view(np.float16).astype(np.float64)
    v = np.arange(256, dtype=np.float64)
    for c in range(3):
        ref = (v / 255.0 - MEAN[c]) / STD[c]
        bound = 2.0 ** -22 * (np.abs(v * float(a[c])) + abs(float(b[c])))
        assert (np.abs(t32[c] - ref) <= bound).all(), c
        binade = np.floor(np.log2(np.maximum(np.abs(t32[c]), 2.0 ** -14)))
        half_ulp = 2.0 ** (binade - 11)
        assert (np.abs(t16[c] - ref) <= bound + half_ulp).all(), c
    # ToTensor: v / 255 within the same bound, 0 and 1 exact
    a, b = hjd.norm_constants()
    t = N.table(a, b, np.float32).view(np.float32).astype(np.float64)
    assert (np.abs(t[0] - v / 255.0) <= 2.0 ** -22 * v / 255.0).all() and t[0][0] == 0.0
    # the identity is exact
    assert (N.table(1, 0, np.float32).view(np.float32)[1] == v).all()
    assert (N.table(1, 0, np.float16).view(np.float16)[2] == v).all()


def test_model_is_one_fused_rounding():
    """fl(v a + b) differs from fl(fl(v a) + b) somewhere on the ImageNet
    constants' scale: the model gives the fused value, checked against exact
    integer arithmetic on a hand-made case."""
    # a = 1 + 2^-23, v = 255: v a = 255 + 255 * 2^-23 needs 32 bits; b = -255 leaves 255 * 2^-23 exactly,
    # where a rounded product (255 + 2^-15 after rounding to 24 bits) would leave 2^-15
    a, b = np.float32(1 + 2.0 ** -23), np.float32(-255)
    t = N.table(a, b, np.float32).view(np.float32)
    assert float(t[0][255]) == 255 * 2.0 ** -23
    assert float(np.float32(np.float32(255) * a) + b) == 2.0 ** -15 != float(t[0][255])


def test_model_zero_and_overflow_entries():
    t16 = N.table((2.0 ** -20, 1, 300), (0, -128, 0), np.float16)
    t32 = N.table((2.0 ** -20, 1, 300), (0, -128, 0), np.float32)
    assert t16[1][128] == 0x0000 and t32[1][128] == 0x00000000          # an exact +0, not -0
    assert t16[1][127] == 0xBC00 and t16[1][129] == 0x3C00              # -1, +1
    assert (t16[2][219:] == 0x7C00).all() and (t16[2][:219] < 0x7C00).all()   # 300 v overflows half above v = 218
    assert t16[2][218] == np.float16(65400).view(np.uint16)
    assert np.isfinite(t32[2].view(np.float32)).all()
    # half subnormals are kept: below 2^-14 the half grid is 2^-24, so v 2^-20 is exactly 16 v quanta
    sub = t16[0].view(np.float16).astype(np.float64) / 2.0 ** -24
    assert (sub == 16 * np.arange(256)).all() and (t16[0][1:64] < 0x0400).all() and t16[0][64] == 0x0400
    # and rounded nearest-even on that grid: v 2^-26 is v / 4 quanta
    q = N.table(2.0 ** -26, 0, np.float16)[0]
    assert list(q[:12]) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 3]   # the ties 0.5, 1.5, 2.5 go to 0, 2, 2
    # signs of exact zeros: -0 only from (-0) + (-0)
    z = N.table((-1.0, 1.0, -0.0), (-0.0, -0.0, 0.0), np.float32)
    assert z[0][0] == 0x80000000 and z[1][0] == 0x00000000 and z[2][7] == 0x00000000
    assert N.table(-0.0, -0.0, np.float16)[0][9] == 0x8000
    # apply() indexes the table per channel
    u8 = np.arange(3 * 2 * 5, dtype=np.uint8).reshape(3, 2, 5)
    got = N.apply(u8, (1, 2, 4), (0, 0, 1), np.float32).view(np.float32)
    assert (got[0] == u8[0]).all() and (got[1] == 2.0 * u8[1]).all() and (got[2] == 4.0 * u8[2] + 1).all()


# ---- declarations -------------------------------------------------------------------
def test_declarations_and_abi(hjd):
    inc = os.path.join(O.REPO, "include")
    hjd_h = open(os.path.join(inc, "hjd.h")).read()
    host_h = open(os.path.join(inc, "hjd_host.h")).read()
    assert re.search(r"HJD_OUT_RGB_PLANAR_F16\s*=\s*5\b", hjd_h) and re.search(r"HJD_OUT_RGB_PLANAR_F32\s*=\s*6\b", hjd_h)
    assert re.search(r"int\s+hjd_plan_set_normalize\(hjd_plan\* plan, const float a\[3\], const float b\[3\]\);", hjd_h)
    assert re.search(r"int\s+hjd_frame_check\(const hjd_frame\* frame, int input_format, int scale, "
                     r"const hjd_rect\* roi\);", hjd_h)
    assert re.search(r"int\s+hjd_gdec_set_normalize\(hjd_gdec\* g, const float a\[3\], const float b\[3\]\);", host_h)
    assert re.search(r"#define\s+HJD_ABI_VERSION\s+1\b", hjd_h)
    from ocljpegdecoder_amd import _lib
    lib = _lib.load()
    for name in ("hjd_plan_set_normalize", "hjd_gdec_set_normalize", "hjd_frame_check"):
        assert getattr(lib, name) and name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.HjdFrame) == 48      # hjd_frame keeps its layout
    assert (hjd.OUT_RGB_PLANAR_F16, hjd.OUT_RGB_PLANAR_F32) == (5, 6)


def test_python_names(hjd):
    import torch
    for name in ("OUT_RGB_PLANAR_F16", "OUT_RGB_PLANAR_F32", "norm_constants", "frame_check"):
        assert name in hjd.__all__, name
    assert hjd.OUT_BYTES[hjd.OUT_RGB_PLANAR_F16] == 6 and hjd.OUT_BYTES[hjd.OUT_RGB_PLANAR_F32] == 12
    assert hjd.OUT_BYTES[hjd.OUT_RGB_PLANAR] == 3 and hjd.OUT_BYTES[hjd.OUT_BGRX] == 4
    assert hjd.default_pitch(W, hjd.OUT_RGB_PLANAR_F16) == 2 * W and hjd.default_pitch(W, hjd.OUT_RGB_PLANAR_F32) == 4 * W
    assert hjd.default_pitch(W, hjd.OUT_RGB_PLANAR) == W and hjd.default_pitch(W, hjd.OUT_BGR24) == (3 * W + 3) & ~3
    from ocljpegdecoder_amd.backend import out_rows
    assert out_rows(H, hjd.OUT_RGB_PLANAR_F16) == out_rows(H, hjd.OUT_RGB_PLANAR_F32) == 3 * H
    assert out_rows(H, hjd.OUT_RGB24) == H
    from ocljpegdecoder_amd.jpeg import _out_pitch
    assert _out_pitch(torch.empty((3, 4, 10), dtype=torch.float16), hjd.OUT_RGB_PLANAR_F16) == 20
    assert _out_pitch(torch.empty((2, 3, 4, 10), dtype=torch.float32)[1], hjd.OUT_RGB_PLANAR_F32) == 40
    assert list(inspect.signature(hjd.norm_constants).parameters) == ["mean", "std"]
    assert inspect.signature(hjd.Plan).parameters["normalize"].default is None
    assert inspect.signature(hjd.decode_frame).parameters["normalize"].default is None
    assert list(inspect.signature(hjd.GpuDecoder.set_normalize).parameters) == ["self", "a", "b"]
    assert list(inspect.signature(hjd.Plan.set_normalize).parameters) == ["self", "a", "b"]
    p = inspect.signature(hjd.GpuDecoder.decode_rgb).parameters
    assert list(p) == ["self", "datas", "layout", "out", "stream", "scale", "rois", "dtype", "mean", "std"]
    assert p["dtype"].default is torch.uint8 and p["mean"].default is None and p["std"].default is None
    assert p["layout"].default == "chw" and p["scale"].default == 1       # the uint8 defaults are unchanged
    spec = hjd.FrameSpec(W, H, hjd.YUV420, out_format=hjd.OUT_RGB_PLANAR_F32, roi=(133, 5, 131, 30))
    assert spec.pitch == 4 * 131 and spec.to_c(2).out_pitch == 4 * 131


# ---- refusals that need no device ----------------------------------------------------
@pytest.mark.parametrize("fmt,elem", [("OUT_RGB_PLANAR_F16", 2), ("OUT_RGB_PLANAR_F32", 4)])
def test_layout_refusals(hjd, fmt, elem):
    f = getattr(hjd, fmt)

    def spec(**kw):
        return hjd.FrameSpec(W, H, hjd.YUV420, out_format=f, **kw)

    hjd.frame_check(spec())
    hjd.frame_check(spec(out_offset=elem * 33, out_pitch=elem * (W + 1)))      # guarded path, legal
    for kw in (dict(out_offset=1), dict(out_offset=elem + 1), dict(out_pitch=elem * W + 1),
               dict(out_offset=elem * 8 + 1)):
        with _invalid("pitch/offset") as e:
            hjd.frame_check(spec(**kw))
        assert e.value.code == -1
    if elem == 4:
        with _invalid("pitch/offset"):
            hjd.frame_check(spec(out_offset=66))          # a multiple of 2, not of 4
        with _invalid("pitch/offset"):
            hjd.frame_check(spec(out_pitch=4 * W + 2))
    with _invalid("pitch/offset"):
        hjd.frame_check(spec(out_pitch=elem * (W - 1)))   # below elem * w
    # scaled and ROI plans measure the pitch against their own width
    hjd.frame_check(spec(out_pitch=elem * 385), scale=2)
    with _invalid("pitch/offset"):
        hjd.frame_check(spec(out_pitch=elem * 384), scale=2)
    hjd.frame_check(spec(roi=(133, 5, 131, 30), out_pitch=elem * 131))
    with _invalid("pitch/offset"):
        hjd.frame_check(spec(roi=(133, 5, 131, 30), out_pitch=elem * 130))
    with _invalid("roi"):
        hjd.frame_check(spec(roi=(700, 5, 131, 30)))
    # the int32 compat input format
    with _invalid("HJD_IN_I32_NATURAL") as e:
        hjd.frame_check(spec(), input_format=hjd.IN_I32_NATURAL)
    assert e.value.code == -1
    hjd.frame_check(hjd.FrameSpec(W, H, hjd.YUV420, out_format=hjd.OUT_RGB_PLANAR), input_format=hjd.IN_I32_NATURAL)
    for unknown in (4, 7, -1):   # 4 was refused before the float formats and still is
        with _invalid("unknown output format"):
            hjd.frame_check(hjd.FrameSpec(W, H, hjd.YUV420, out_format=unknown, out_pitch=4 * W))


def test_non_finite_constants_are_refused(hjd):
    """The setters check the constants before they look at the handle."""
    from ocljpegdecoder_amd import _lib
    lib = _lib.load()
    one, zero = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(0, 0, 0)
    for bad in (float("inf"), float("-inf"), float("nan")):
        for k in range(3):
            arr = (ctypes.c_float * 3)(1, 1, 1)
            arr[k] = bad
            for fn in (lib.hjd_plan_set_normalize, lib.hjd_gdec_set_normalize):
                for a, b in ((arr, zero), (one, arr)):
                    assert fn(None, a, b) == -1
                    assert "finite" in _lib.error_string()
    assert lib.hjd_plan_set_normalize(None, one, zero) == -1 and "NULL" in _lib.error_string()
    assert lib.hjd_gdec_set_normalize(None, one, zero) == -1 and "NULL" in _lib.error_string()
    assert lib.hjd_plan_set_normalize(None, None, zero) == -1 and "NULL" in _lib.error_string()


def test_decode_rgb_argument_refusals(hjd):
    """decode_rgb refuses these before it touches the decoder or the data."""
    import torch
    gd = object.__new__(hjd.GpuDecoder)   # no device behind it: the refusals come first
    gd.handle = None
    for dt in (torch.float16, torch.float32):
        with pytest.raises(ValueError, match="chw"):
            gd.decode_rgb([b""], layout="hwc", dtype=dt)
    for kw in (dict(mean=MEAN), dict(std=STD), dict(mean=0.5, std=0.5)):
        with pytest.raises(ValueError, match="float"):
            gd.decode_rgb([b""], dtype=torch.uint8, **kw)
        with pytest.raises(ValueError, match="float"):
            gd.decode_rgb([b""], layout="hwc", **kw)
    with pytest.raises(ValueError, match="dtype"):
        gd.decode_rgb([b""], dtype=torch.int32)
    with pytest.raises(ValueError, match="finite"):
        gd.decode_rgb([b""], dtype=torch.float16, std=0.0)
