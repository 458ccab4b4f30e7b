"""The resize without a GPU: the numpy model of the definition (resize_model.py)
against torch's bilinear interpolation on the CPU, hjd_resize_check's
refusals, resize_scale's table, and the resize kernel's place in the built
library (its own three instantiations; the pixel-kernel table is checked,
unchanged, by test_kernel_table_cpu.py)."""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import resize_model as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (w, h, Wo, Ho)
SHAPES = [(5, 3, 16, 8), (16, 8, 16, 8), (37, 29, 8, 8), (1, 1, 7, 5), (400, 40, 3, 3), (1, 9, 10, 7),
          (223, 225, 224, 224), (16384, 3, 16384, 2), (2, 2, 16384, 3)]
# Derived, not measured: flooring the two 11-bit weights moves the value by
# less than 255 * 2^-10 ~ 0.249, the final rounding by at most 0.5; 1e-3 covers
# the float64 reference's own arithmetic.
BOUND = 0.75 + 1e-3


def _src(w, h):
    return np.random.default_rng(1000 * w + h).integers(0, 256, (3, h, w), dtype=np.uint8)


@pytest.mark.parametrize("w,h,wo,ho", SHAPES)
def test_model_vs_torch_bilinear(w, h, wo, ho):
    import torch
    import torch.nn.functional as F
    src = _src(w, h)
    got = R.resize_u8(src, wo, ho)
    assert got.shape == (3, ho, wo) and got.dtype == np.uint8
    ref = F.interpolate(torch.from_numpy(src)[None].double(), size=(ho, wo), mode="bilinear", align_corners=False,
                        antialias=False)[0].numpy()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{w}x{h} -> {wo}x{ho}: max |model - torch| = {err:.4f}")
    assert err <= BOUND
    if (w, h) == (wo, ho):
        np.testing.assert_array_equal(got, src)   # identity: byte for byte


def test_model_flip_and_floats():
    import norm_model
    src = _src(37, 29)
    plain, flipped = R.resize_u8(src, 10, 7), R.resize_u8(src, 10, 7, flip=True)
    np.testing.assert_array_equal(flipped, plain[:, :, ::-1])
    assert not np.array_equal(flipped, plain)
    a, b = (1 / 255.0,) * 3, (0.0,) * 3
    for dt in (np.float16, np.float32):
        np.testing.assert_array_equal(R.resize(src, 10, 7, dtype=dt, a=a, b=b), norm_model.apply(plain, a, b, dt))


# ---- hjd_resize_check ---------------------------------------------------------
PLANAR, F16, F32 = 3, 5, 6


def _check(hjd, items, n, wo, ho, pitch, fmt):
    lib = hjd._lib.load()
    arr = (hjd._lib.HjdResizeItem * len(items))(*[hjd._lib.HjdResizeItem(*it) for it in items])
    rc = lib.hjd_resize_check(arr, n, wo, ho, pitch, fmt)
    return rc, hjd._lib.error_string()


def _refused(hjd, match, items, n, wo, ho, pitch, fmt):
    rc, msg = _check(hjd, items, n, wo, ho, pitch, fmt)
    assert rc == -1, (rc, msg)   # HJD_E_INVALID
    assert re.search(match, msg), msg


def test_resize_check(hjd):
    lib = hjd._lib.load()
    ok = (0x1000, 0x2000, 37, 29, 37, 0)   # src, dst, w, h, pitch, flags
    flipped = (0x1001, 0x3000, 5, 3, 7, 1)
    assert _check(hjd, [ok, flipped], 2, 24, 16, 24, PLANAR)[0] == 0
    assert _check(hjd, [ok, flipped], 2, 24, 16, 50, F16)[0] == 0
    assert _check(hjd, [ok, flipped], 2, 24, 16, 96, F32)[0] == 0
    assert _check(hjd, [(0x1000, 0x2000, 16384, 16384, 16384, 1)], 1, 16384, 16384, 16384, PLANAR)[0] == 0
    assert _check(hjd, [(0x1000, 0x2000, 1, 1, 1, 0)], 1, 1, 1, 1, PLANAR)[0] == 0
    # n and items
    assert lib.hjd_resize_check(None, 1, 24, 16, 24, PLANAR) == -1 and "NULL" in hjd._lib.error_string()
    for n in (0, -1):
        _refused(hjd, "n = ", [ok], n, 24, 16, 24, PLANAR)
    # dimensions outside 1..16384, each of the four
    for bad in (0, -3, 16385):
        _refused(hjd, "output size", [ok], 1, bad, 16, 1 << 20, PLANAR)
        _refused(hjd, "output size", [ok], 1, 24, bad, 24, PLANAR)
        _refused(hjd, "item 0: source size", [(0x1000, 0x2000, bad, 29, 1 << 20, 0)], 1, 24, 16, 24, PLANAR)
        _refused(hjd, "item 1: source size", [ok, (0x1000, 0x2000, 37, bad, 37, 0)], 2, 24, 16, 24, PLANAR)
    # null pointers
    _refused(hjd, "item 0: src or dst is NULL", [(0, 0x2000, 37, 29, 37, 0)], 1, 24, 16, 24, PLANAR)
    _refused(hjd, "item 1: src or dst is NULL", [ok, (0x1000, 0, 37, 29, 37, 0)], 2, 24, 16, 24, PLANAR)
    # pitches
    _refused(hjd, "src_pitch", [(0x1000, 0x2000, 37, 29, 36, 0)], 1, 24, 16, 24, PLANAR)
    _refused(hjd, "out_pitch", [ok], 1, 24, 16, 23, PLANAR)
    _refused(hjd, "out_pitch", [ok], 1, 24, 16, 46, F16)    # < 2 * 24
    _refused(hjd, "out_pitch", [ok], 1, 24, 16, 49, F16)    # not a multiple of 2
    _refused(hjd, "out_pitch", [ok], 1, 24, 16, 98, F32)    # not a multiple of 4
    _refused(hjd, "dst must be a multiple", [(0x1000, 0x2001, 37, 29, 37, 0)], 1, 24, 16, 48, F16)
    _refused(hjd, "dst must be a multiple", [(0x1000, 0x2002, 37, 29, 37, 0)], 1, 24, 16, 96, F32)
    assert _check(hjd, [(0x1000, 0x2001, 37, 29, 37, 0)], 1, 24, 16, 24, PLANAR)[0] == 0   # bytes: any dst
    # formats: the interleaved ones, the hole at 4, unknown values
    for fmt in (0, 1, 2, 4, 7, -1):
        _refused(hjd, "output format", [ok], 1, 24, 16, 4 * 24, fmt)
    # flag bits
    for flags in (2, 3, 4, -2, 1 << 30):
        _refused(hjd, "flag bits", [(0x1000, 0x2000, 37, 29, 37, flags)], 1, 24, 16, 24, PLANAR)


def test_resize_entry_points_are_bound(hjd):
    """Declared in the headers, exported, bound in _lib.py; NULL objects are refused without a device."""
    lib = hjd._lib.load()
    for name in ("hjd_resize_check", "hjd_resize_create", "hjd_resize_set_normalize", "hjd_resize_launch",
                 "hjd_resize_destroy", "hjd_gdec_decode_resized"):
        assert name in hjd._lib.SIGNATURES and getattr(lib, name).argtypes == hjd._lib.SIGNATURES[name][1]
    assert lib.hjd_resize_launch(None, None) == -1
    one = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.hjd_resize_set_normalize(None, one, one) == -1
    assert lib.hjd_resize_destroy(None) == 0
    assert lib.hjd_gdec_decode_resized(None, None, None, 1, None, None, None, 8, 8, 8, None) == -1
    assert callable(hjd.Resize) and callable(hjd.GpuDecoder.decode_resized) and hjd.RESIZE_FLIP_H == 1


# ---- resize_scale ---------------------------------------------------------------
@pytest.mark.parametrize("src_w,src_h,wo,ho,expect", [
    (1920, 1080, 224, 224, 4),      # 1080 / 4 = 270 >= 224, 1080 / 8 = 135 < 224
    (3840, 2160, 224, 224, 8),      # 2160 / 8 = 270
    (1792, 1792, 224, 224, 8),      # exactly 8x
    (1791, 1792, 224, 224, 8),      # ceil(1791 / 8) = 224
    (1784, 1792, 224, 224, 4),      # ceil(1784 / 8) = 223
    (448, 448, 224, 224, 2),
    (447, 448, 224, 224, 2),        # ceil(447 / 2) = 224
    (446, 448, 224, 224, 1),
    (224, 224, 224, 224, 1),
    (100, 80, 224, 224, 1),         # an upscale
    (4000, 230, 224, 224, 1),       # the short side decides
    (1, 1, 1, 1, 8),
    (16384, 16384, 1, 1, 8),
])
def test_resize_scale(hjd, src_w, src_h, wo, ho, expect):
    s = hjd.resize_scale(src_w, src_h, wo, ho)
    assert s == expect
    if s > 1:   # what it promises, through the library's own scaled size
        sw, sh = hjd.scaled_size(src_w, src_h, s)
        assert sw >= wo and sh >= ho


# ---- the built library ------------------------------------------------------------
def test_resize_kernel_has_three_instantiations_of_its_own(hjd):
    sys.path.insert(0, os.path.join(REPO, "tools", "check"))
    import d16_order
    if not os.path.exists(d16_order.LLVM_OBJDUMP):
        pytest.skip("llvm-objdump is not installed")
    lib_path = os.path.join(REPO, "ocljpegdecoder_amd", "lib", "libhjd.so")
    tmp = tempfile.mkdtemp(prefix="hjd_resize_")
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
    assert set(re.findall(r"hjd::resize_kernel<(\d+)>\(", syms)) == {"0", "1", "2"}
