"""The antialiased resize without a GPU: the numpy model of the definition
(resize_aa_model.py) against torch's antialiased bilinear interpolation on the
CPU and against its own laws, hjd_resize_check_filter's refusals, the names of
the C and Python interfaces, and the two kernels' place in the built library."""
import ctypes
import glob
import inspect
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import resize_aa_model as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (w, h, Wo, Ho), every dimension >= 2 (torch's antialiased kernel repeats one
# value along a size-1 dimension, which is not the definition); each case is
# also run transposed.
TORCH_SHAPES = [(37, 29, 24, 16), (100, 80, 7, 5), (9, 200, 9, 3), (33, 17, 40, 50), (300, 257, 224, 224),
                (540, 960, 224, 224)]
# Derived, not measured: with exact weights the horizontal rounding moves an
# intermediate byte by at most 0.5, which the vertical weights (non-negative,
# summing to 1) carry to at most 0.5 in the result; the final rounding adds at
# most 0.5.  1e-6 covers the float64 reference's own arithmetic.
BOUND = 1.0 + 1e-6


def _src(w, h, kind="rand"):
    if kind == "checker":
        plane = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
        return np.ascontiguousarray(np.broadcast_to(plane, (3, h, w)))
    return np.random.default_rng(1000 * w + h).integers(0, 256, (3, h, w), dtype=np.uint8)


@pytest.mark.parametrize("kind", ["rand", "checker"])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("w,h,wo,ho", TORCH_SHAPES)
def test_model_vs_torch_antialias(w, h, wo, ho, transposed, kind):
    import torch
    import torch.nn.functional as F
    if transposed:
        w, h, wo, ho = h, w, ho, wo
    src = _src(w, h, kind)
    got = A.resize_u8(src, wo, ho)
    assert got.shape == (3, ho, wo) and got.dtype == np.uint8
    ref = F.interpolate(torch.from_numpy(src)[None].double(), size=(ho, wo), mode="bilinear", align_corners=False,
                        antialias=True)[0].numpy()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{w}x{h} -> {wo}x{ho} {kind}: max |model - torch| = {err:.4f}")
    assert err <= BOUND


# ---- the model's own laws -------------------------------------------------------
@pytest.mark.parametrize("w,h", [(16, 8), (37, 29), (1, 1), (1, 9), (7, 1)])
def test_same_size_is_the_source(w, h):
    src = _src(w, h)
    np.testing.assert_array_equal(A.resize_u8(src, w, h), src)
    np.testing.assert_array_equal(A.resize_u8(src, w, h, flip=True), src[:, :, ::-1])


@pytest.mark.parametrize("w,h,wo,ho", [(37, 29, 10, 7), (5, 3, 16, 8), (64, 9, 3, 9), (9, 200, 9, 3)])
def test_flip_law_and_floats(w, h, wo, ho):
    import norm_model
    src = _src(w, h)
    plain, flipped = A.resize_u8(src, wo, ho), A.resize_u8(src, wo, ho, flip=True)
    np.testing.assert_array_equal(flipped, plain[:, :, ::-1])
    assert not np.array_equal(flipped, plain)
    a, b = (1 / 255.0, 2.0, 0.5), (0.0, -1.0, 0.25)
    for dt in (np.float16, np.float32):
        np.testing.assert_array_equal(A.resize(src, wo, ho, dtype=dt, a=a, b=b), norm_model.apply(plain, a, b, dt))


@pytest.mark.parametrize("size,out_size", [(1, 1), (1, 3), (5, 5), (5, 6), (5, 16), (17, 50), (33, 40), (2, 16384)])
def test_enlargement_is_two_tap_bilinear(size, out_size):
    """Wo >= w: at most two taps, 2 Wo apart in d, and T = 2 Wo unless the second tap fell outside the image."""
    for j, (k0, t) in enumerate(A.axis_weights(size, out_size)):
        assert 1 <= t.size <= 2
        if t.size == 2:
            assert int(t.sum()) == 2 * out_size
        else:
            d = (2 * k0 + 1) * out_size - (2 * j + 1) * size
            # one tap: exactly on a sample (the other weighs 0), or the neighbour lies outside the image
            assert d == 0 or (k0 == 0 and d > 0) or (k0 == size - 1 and d < 0)
            assert int(t.sum()) == 2 * out_size - abs(d)


def test_one_pixel_sources_and_outputs():
    one = np.array([[[7]], [[130]], [[255]]], np.uint8)
    for wo, ho in ((3, 3), (1, 1), (5, 2)):
        np.testing.assert_array_equal(A.resize_u8(one, wo, ho), np.broadcast_to(one, (3, ho, wo)))
    src = _src(5, 7)
    got = A.resize_u8(src, 1, 1)
    assert got.shape == (3, 1, 1)
    # every pixel weighs in: a constant image stays constant, and the mean bounds the result's distance
    np.testing.assert_array_equal(A.resize_u8(np.full((3, 7, 5), 93, np.uint8), 1, 1), np.full((3, 1, 1), 93, np.uint8))
    assert (np.abs(got[:, 0, 0].astype(np.float64) - src.reshape(3, -1).mean(1)) < 64).all()
    assert A.resize_u8(_src(300, 7), 1, 1).shape == (3, 1, 1)


@pytest.mark.parametrize("w,h,wo,ho", [(1448, 2, 1, 2), (2, 1448, 2, 1), (16384, 2, 128, 1), (2, 16384, 2, 128)])
def test_bounds_hold_at_the_legality_edge(w, h, wo, ho):
    """The model's 2^31 asserts at src^2 == 2^21 * out (or just below), on all-255 and random sources."""
    assert A.legal(w, wo) and A.legal(h, ho)
    white = np.full((3, h, w), 255, np.uint8)
    np.testing.assert_array_equal(A.resize_u8(white, wo, ho), np.full((3, ho, wo), 255, np.uint8))
    assert A.resize_u8(_src(w, h), wo, ho).shape == (3, ho, wo)
    assert not A.legal(1449, 1) and not A.legal(16384, 127)


# ---- hjd_resize_check_filter ---------------------------------------------------------
PLANAR, F16, F32 = 3, 5, 6
BILINEAR, AA = 0, 1


def _check(hjd, items, n, wo, ho, pitch, fmt, filt):
    lib = hjd._lib.load()
    arr = (hjd._lib.HjdResizeItem * len(items))(*[hjd._lib.HjdResizeItem(*it) for it in items])
    rc = lib.hjd_resize_check_filter(arr, n, wo, ho, pitch, fmt, filt)
    return rc, hjd._lib.error_string()


def _refused(hjd, match, items, n, wo, ho, pitch, fmt, filt=AA):
    rc, msg = _check(hjd, items, n, wo, ho, pitch, fmt, filt)
    assert rc == -1, (rc, msg)   # HJD_E_INVALID
    assert re.search(match, msg), msg


def test_check_filter(hjd):
    lib = hjd._lib.load()
    ok = (0x1000, 0x2000, 37, 29, 37, 0)   # src, dst, w, h, pitch, flags
    flipped = (0x1001, 0x3000, 5, 3, 7, 1)
    big = (0x1000, 0x2000, 16384, 16384, 16384, 1)
    # filter 0 accepts what hjd_resize_check accepts -- also what filter 1's ratio rule refuses
    for args in (([ok, flipped], 2, 24, 16, 24, PLANAR), ([ok, flipped], 2, 24, 16, 50, F16),
                 ([ok, flipped], 2, 24, 16, 96, F32), ([big], 1, 16384, 16384, 16384, PLANAR),
                 ([(0x1000, 0x2000, 1, 1, 1, 0)], 1, 1, 1, 1, PLANAR), ([big], 1, 1, 1, 1, PLANAR)):
        arr = (hjd._lib.HjdResizeItem * len(args[0]))(*[hjd._lib.HjdResizeItem(*it) for it in args[0]])
        assert lib.hjd_resize_check(arr, *args[1:]) == 0
        assert _check(hjd, *args, BILINEAR)[0] == 0
    for args in (([ok, flipped], 2, 24, 16, 24, PLANAR), ([ok, flipped], 2, 24, 16, 50, F16),
                 ([ok, flipped], 2, 24, 16, 96, F32), ([big], 1, 16384, 16384, 16384, PLANAR)):
        assert _check(hjd, *args, AA)[0] == 0
    # the filter itself
    for filt in (2, -1, 1 << 20):
        _refused(hjd, "filter", [ok], 1, 24, 16, 24, PLANAR, filt)
    # the ratio rule, per axis, naming it
    wide = lambda w: (0x1000, 0x2000, w, 2, w, 0)
    tall = lambda h: (0x1000, 0x2000, 2, h, 2, 0)
    assert _check(hjd, [wide(1448)], 1, 1, 2, 1, PLANAR, AA)[0] == 0
    assert _check(hjd, [tall(1448)], 1, 2, 1, 2, PLANAR, AA)[0] == 0
    assert _check(hjd, [wide(16384)], 1, 128, 2, 128, PLANAR, AA)[0] == 0
    assert _check(hjd, [tall(16384)], 1, 2, 128, 2, PLANAR, AA)[0] == 0
    _refused(hjd, r"item 0: src_w 1449 -> out_w 1\b", [wide(1449)], 1, 1, 2, 1, PLANAR)
    _refused(hjd, r"item 1: src_h 1449 -> out_h 1\b", [ok, tall(1449)], 2, 2, 1, 2, PLANAR)
    _refused(hjd, r"src_w 16384 -> out_w 127\b", [wide(16384)], 1, 127, 2, 127, PLANAR)
    _refused(hjd, r"src_h 16384 -> out_h 127\b", [tall(16384)], 1, 2, 127, 2, PLANAR)
    assert _check(hjd, [wide(1449)], 1, 1, 2, 1, PLANAR, BILINEAR)[0] == 0
    # every refusal of hjd_resize_check stays at filter 1
    assert lib.hjd_resize_check_filter(None, 1, 24, 16, 24, PLANAR, AA) == -1 and "NULL" in hjd._lib.error_string()
    for n in (0, -1):
        _refused(hjd, "n = ", [ok], n, 24, 16, 24, PLANAR)
    for bad in (0, -3, 16385):
        _refused(hjd, "output size", [ok], 1, bad, 16, 1 << 20, PLANAR)
        _refused(hjd, "output size", [ok], 1, 24, bad, 24, PLANAR)
        _refused(hjd, "item 0: source size", [(0x1000, 0x2000, bad, 29, 1 << 20, 0)], 1, 24, 16, 24, PLANAR)
        _refused(hjd, "item 1: source size", [ok, (0x1000, 0x2000, 37, bad, 37, 0)], 2, 24, 16, 24, PLANAR)
    _refused(hjd, "item 0: src or dst is NULL", [(0, 0x2000, 37, 29, 37, 0)], 1, 24, 16, 24, PLANAR)
    _refused(hjd, "item 1: src or dst is NULL", [ok, (0x1000, 0, 37, 29, 37, 0)], 2, 24, 16, 24, PLANAR)
    _refused(hjd, "src_pitch", [(0x1000, 0x2000, 37, 29, 36, 0)], 1, 24, 16, 24, PLANAR)
    _refused(hjd, "out_pitch", [ok], 1, 24, 16, 23, PLANAR)
    _refused(hjd, "out_pitch", [ok], 1, 24, 16, 46, F16)
    _refused(hjd, "out_pitch", [ok], 1, 24, 16, 49, F16)
    _refused(hjd, "out_pitch", [ok], 1, 24, 16, 98, F32)
    _refused(hjd, "dst must be a multiple", [(0x1000, 0x2001, 37, 29, 37, 0)], 1, 24, 16, 48, F16)
    _refused(hjd, "dst must be a multiple", [(0x1000, 0x2002, 37, 29, 37, 0)], 1, 24, 16, 96, F32)
    assert _check(hjd, [(0x1000, 0x2001, 37, 29, 37, 0)], 1, 24, 16, 24, PLANAR, AA)[0] == 0
    for fmt in (0, 1, 2, 4, 7, -1):
        _refused(hjd, "output format", [ok], 1, 24, 16, 4 * 24, fmt)
    for flags in (2, 3, 4, -2, 1 << 30):
        _refused(hjd, "flag bits", [(0x1000, 0x2000, 37, 29, 37, flags)], 1, 24, 16, 24, PLANAR)


# ---- names ------------------------------------------------------------------------
def test_entry_points_and_python_names(hjd):
    lib = hjd._lib.load()
    c_int, vp = ctypes.c_int, ctypes.c_void_p
    items = ctypes.POINTER(hjd._lib.HjdResizeItem)
    u8pp = ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))
    declared = {
        "hjd_resize_check_filter": [items] + [c_int] * 6,
        "hjd_resize_create_filter": [vp, items] + [c_int] * 6 + [ctypes.POINTER(vp)],
        "hjd_gdec_decode_resized_filter": [vp, u8pp, ctypes.POINTER(ctypes.c_size_t), c_int,
                                           ctypes.POINTER(hjd._lib.HjdRect), ctypes.POINTER(ctypes.c_int32), vp, c_int,
                                           c_int, ctypes.c_int32, c_int, vp],
    }
    for name, argtypes in declared.items():
        assert name in hjd._lib.SIGNATURES
        restype, bound = hjd._lib.SIGNATURES[name]
        assert restype is c_int and list(bound) == argtypes, name
        assert getattr(lib, name).argtypes == bound
    # NULL objects are refused without a device
    assert lib.hjd_resize_check_filter(None, 1, 8, 8, 8, PLANAR, AA) == -1
    assert lib.hjd_resize_create_filter(None, None, 1, 8, 8, 8, PLANAR, AA, None) == -1
    assert lib.hjd_gdec_decode_resized_filter(None, None, None, 1, None, None, None, 8, 8, 8, AA, None) == -1
    assert hjd.RESIZE_BILINEAR == 0 and hjd.RESIZE_TRIANGLE_AA == 1
    for fn in (hjd.Resize.__init__, hjd.GpuDecoder.decode_resized, hjd.GpuDecoder.decode_rgb_resized):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "antialias" and last.default is False, fn


# ---- the built library ------------------------------------------------------------
def test_antialias_kernels_in_the_built_library(hjd):
    sys.path.insert(0, os.path.join(REPO, "tools", "check"))
    import d16_order
    if not os.path.exists(d16_order.LLVM_OBJDUMP):
        pytest.skip("llvm-objdump is not installed")
    lib_path = os.path.join(REPO, "ocljpegdecoder_amd", "lib", "libhjd.so")
    tmp = tempfile.mkdtemp(prefix="hjd_resize_aa_")
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
    assert re.search(r"hjd::resize_aa_h_kernel\(", syms)
    assert set(re.findall(r"hjd::resize_aa_v_kernel<(\d+)>\(", syms)) == {"0", "1", "2"}
    assert set(re.findall(r"hjd::resize_kernel<(\d+)>\(", syms)) == {"0", "1", "2"}
