"""The colour stage without a device: the numpy model of include/hjd.h's
definition (tests/color_model.py) against the real-valued map and its derived
bound, color_matrix() against the blend formulas it rounds, hjd_color_check's
refusals, and the interfaces."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import color_model as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANAR, F16, F32 = 3, 5, 6
LUMA = np.array([0.299, 0.587, 0.114])
EPS = 1e-9   # the float64 evaluation of the real map: |y| < 2^17, 2^-52 relative per operation


def _images(rng):
    """Random and all-0 / all-255 images of 1x1 .. 8x8."""
    for h in range(1, 9):
        for w in range(1, 9):
            yield rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    for v in (0, 255):
        for h, w in ((1, 1), (3, 5), (8, 8)):
            yield np.full((3, h, w), v, np.uint8)


def _limit_records(rng, count):
    """Random records, most entries at or next to the range limits."""
    for k in range(count):
        coef = rng.integers(-C.MAX_COEF, C.MAX_COEF + 1, 18)
        lim = rng.choice([-C.MAX_COEF, C.MAX_COEF, 0, 1, -1], 18)
        coef = np.where(rng.random(18) < 0.5, lim, coef)
        t = rng.integers(-C.MAX_OFFSET, C.MAX_OFFSET + 1, 3)
        t = np.where(rng.random(3) < 0.5, rng.choice([-C.MAX_OFFSET, C.MAX_OFFSET, 0], 3), t)
        if k % 4 == 0:
            coef[9:] = 0          # p = 0
        yield [int(v) for v in coef] + [int(v) for v in t]
    for s in (1, -1):             # everything at one limit
        yield [s * C.MAX_COEF] * 18 + [s * C.MAX_OFFSET] * 3
        yield [s * C.MAX_COEF] * 18 + [-s * C.MAX_OFFSET] * 3


# ---- the model --------------------------------------------------------------------------------
def test_model_stays_within_the_derived_bound():
    """u8 against clamp(real map of the integer record): 0.5 + 2^-13 + sum|p| / 4096 * 2^-9.
    The model asserts the widths (24-bit products, int32 accumulator) on every value it forms."""
    rng = np.random.default_rng(2024)
    worst, worst_bound = 0.0, 0.0
    records = list(_limit_records(rng, 60))
    for src in _images(rng):
        for rec in records:
            got = C.color_u8(src, rec).astype(np.float64)
            want = np.clip(C.real_of_record(src, rec), 0.0, 255.0)
            err = np.abs(got - want).reshape(3, -1).max(axis=1)
            assert (err <= C.bound(rec) + EPS).all(), (src.shape, rec, err, C.bound(rec))
            k = int(np.argmax(err))
            if err[k] > worst:
                worst, worst_bound = float(err[k]), float(C.bound(rec)[k])
    print(f"largest error {worst:.4f} (its bound {worst_bound:.4f}; the largest bound {0.5 + 2.0 ** -13 + 24 * 2.0 ** -9:.4f})")
    assert worst >= 0.5 - 1e-3                    # the rounding's half is reached: the bound is not slack by design
    assert C.bound([C.MAX_COEF] * 18 + [0] * 3).max() < 0.5 + 2.0 ** -13 + 24 * 2.0 ** -9


def test_laws():
    rng = np.random.default_rng(5)
    for src in _images(rng):
        np.testing.assert_array_equal(C.color_u8(src, C.IDENTITY), src)
        np.testing.assert_array_equal(C.color_u8(src, C.INVERSE), 255 - src)
        read = []
        C.offsets(C.INVERSE, src, read)
        assert read == []                         # p = 0: the sums are not read
        C.offsets([0] * 9 + [1] + [0] * 11, src, read)
        assert read == [True]


def test_mean_rounding_boundary():
    """N = 2 with an odd sum: 256 S / N ends in .0, N = 3: thirds; mq rounds to nearest, ties up."""
    assert C.means_q8(np.array([[[0, 1]]] * 3, np.uint8)).tolist() == [128] * 3
    assert C.means_q8(np.array([[[254, 255]]] * 3, np.uint8)).tolist() == [65152] * 3
    assert C.means_q8(np.array([[[0, 0, 1]], [[0, 1, 1]], [[1, 1, 1]]], np.uint8)).tolist() == [85, 171, 256]
    # (S 256 + (N >> 1)) / N at N = 4: S = 1 -> 64.5 -> floor(66 / 4 ...) = 64 + (2 / 4) -> 64
    assert C.means_q8(np.array([[[0, 0, 0, 1]]] * 3, np.uint8)).tolist() == [64] * 3
    # a tie in Q8 needs 256 S / N = k + 1/2: N = 512 -> S odd
    src = np.zeros((3, 16, 32), np.uint8)
    src[:, 0, 0] = 3
    assert C.means_q8(src).tolist() == [2] * 3    # 1.5 rounds up


def test_the_limit_records_reach_both_clamps_and_negative_accumulators():
    """What the limit records are there for, asserted on the model's own values (no device)."""
    from test_gpu_color import _records     # the GPU tests' records: no device is touched
    src = np.random.default_rng(257005).integers(0, 256, (3, 5, 257), dtype=np.uint8)
    lo = hi = neg = False
    for name, rec in _records().items():
        if not name.startswith("limits"):
            continue
        m, _, _ = C.split(rec)
        acc = np.einsum("ck,khw->chw", m, src.astype(np.int64)) + (C.offsets(rec, src) + 2048)[:, None, None]
        neg = neg or bool((acc < -4096).any())
        lo, hi = lo or bool(((acc >> 12) < 0).any()), hi or bool(((acc >> 12) > 255).any())
        u8 = C.color_u8(src, rec)
        assert u8.min() == 0 or u8.max() == 255
    assert lo and hi and neg
    mixed = C.color_u8(src, _records()["limits+1-1+1"])      # m against the means: both clamps in one image
    assert mixed.min() == 0 and mixed.max() == 255


# ---- color_matrix ---------------------------------------------------------------------------
def _safe_images(rng, lo=64, hi=192):
    """Images in the middle of the range: a mild operation saturates nothing."""
    for h, w in ((1, 1), (2, 3), (5, 4), (8, 8)):
        yield rng.integers(lo, hi, (3, h, w), dtype=np.uint8)


def _luma(x):
    return np.einsum("k,khw->hw", LUMA, x)


def _blend(name, f, x):
    """The float64 blend formula of one operation on x (3, h, w) float64."""
    if name == "brightness":
        return f * x
    if name == "contrast":
        return f * x + (1 - f) * float(LUMA @ x.reshape(3, -1).mean(axis=1))
    if name == "saturation":
        return f * x + (1 - f) * _luma(x)[None]
    if name == "gray":
        return np.broadcast_to(_luma(x)[None], x.shape)
    if name == "invert":
        return 255.0 - x
    raise AssertionError(name)


def _rec_bound(rec):
    return C.bound(rec).max() + C.ROUNDED_COEFS


def test_color_matrix_defaults_are_the_identity(hjd):
    assert hjd.color_matrix() == list(C.IDENTITY) == list(hjd.COLOR_IDENTITY)
    assert hjd.color_matrix(invert=True) == list(C.INVERSE)
    assert all(isinstance(v, int) for v in hjd.color_matrix(contrast=0.3, hue=0.1))


@pytest.mark.parametrize("name,f", [("brightness", 0.7), ("brightness", 1.25), ("contrast", 0.5), ("contrast", 1.3),
                                    ("saturation", 0.0), ("saturation", 1.4), ("gray", True), ("invert", True)])
def test_single_operations_follow_their_blend_formulas(hjd, name, f):
    rng = np.random.default_rng(11)
    rec = hjd.color_matrix(**{name: f})
    for src in _safe_images(rng):
        want = _blend(name, f, src.astype(np.float64))
        assert want.min() >= 0.0 and want.max() <= 255.0          # nothing saturates
        err = np.abs(C.color_u8(src, rec).astype(np.float64) - want).max()
        assert err <= 1.0 and err <= _rec_bound(rec) + EPS, (name, f, err, _rec_bound(rec))


def test_contrast_pivot_and_hue(hjd):
    rng = np.random.default_rng(12)
    rec = hjd.color_matrix(contrast=0.5, pivot=128)
    assert not any(rec[9:18]) and rec[18:] == [64 * 4096] * 3
    # hue: a rotation about the grey axis in YIQ -- greys stay, luma stays, half a turn twice is the identity
    for h in (0.25, -0.1, 0.5):
        M = np.array(hjd.backend._color_ops(hue=h)[0])
        np.testing.assert_allclose(M @ np.ones(3), np.ones(3), atol=1e-12)
        np.testing.assert_allclose(LUMA @ M, LUMA, atol=1e-12)
        back = np.array(hjd.backend._color_ops(hue=-h)[0])
        np.testing.assert_allclose(back @ M, np.eye(3), atol=1e-12)
        yiq = np.array(hjd.backend._RGB_TO_YIQ)
        a = 2 * math.pi * h
        rot = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
        np.testing.assert_allclose(yiq @ M @ np.linalg.inv(yiq), rot, atol=1e-12)
        rec = hjd.color_matrix(hue=h)
        for src in _safe_images(rng, 100, 156):
            want = np.einsum("ck,khw->chw", M, src.astype(np.float64))
            assert want.min() >= 0 and want.max() <= 255
            assert np.abs(C.color_u8(src, rec) - want).max() <= min(1.0, _rec_bound(rec) + EPS)


def test_composition_law(hjd):
    """color_matrix of two operations is the second single-operation map after the first on the
    real-valued model, means included: (M2, P2, t2) o (M1, P1, t1)."""
    rng = np.random.default_rng(13)
    ops = hjd.backend._color_ops
    cases = [({"brightness": 1.2}, {"contrast": 0.6}, ("brightness", "contrast", "saturation", "hue")),
             ({"contrast": 1.4}, {"brightness": 0.8}, ("contrast", "brightness", "saturation", "hue")),
             ({"contrast": 0.5}, {"saturation": 1.5}, ("brightness", "contrast", "saturation", "hue")),
             ({"saturation": 0.3}, {"contrast": 1.2}, ("saturation", "contrast", "brightness", "hue")),
             ({"contrast": 0.7}, {"hue": 0.2}, ("brightness", "contrast", "saturation", "hue")),
             ({"contrast": 0.7}, {"invert": True}, ("brightness", "contrast", "saturation", "hue")),
             ({"hue": -0.3}, {"gray": True}, ("brightness", "contrast", "saturation", "hue"))]
    for first, second, order in cases:
        both = ops(order=order, **first, **second)
        rec = hjd.color_matrix(order=order, **first, **second)
        for src in _images(rng):
            step1 = C.real_map(src, *ops(**first))
            # the second map on the real-valued intermediate: its means are the intermediate's
            M2, P2, t2 = (np.array(v) for v in ops(**second))
            xbar = step1.reshape(3, -1).mean(axis=1)
            seq = np.einsum("ck,khw->chw", M2, step1) + (P2 @ xbar + t2)[:, None, None]
            np.testing.assert_allclose(C.real_map(src, *both), seq, atol=1e-9)
            err = np.abs(C.color_u8(src, rec) - np.clip(seq, 0, 255)).max()
            assert err <= _rec_bound(rec) + EPS, (first, second, err)


def test_gray_rows_are_equal_and_arguments_are_checked(hjd):
    rec = hjd.color_matrix(brightness=1.1, contrast=0.8, saturation=1.3, hue=0.05, gray=True)
    assert rec[0:3] == rec[3:6] == rec[6:9] and rec[9:12] == rec[12:15] == rec[15:18] and len(set(rec[18:])) == 1
    for bad in (dict(brightness=8.5), dict(brightness=-0.1), dict(contrast=float("nan")), dict(saturation=float("inf")),
                dict(hue=0.6), dict(hue=-0.51), dict(order=("brightness", "contrast")), dict(order=("a", "b", "c", "d")),
                dict(pivot="median"), dict(contrast=0.0, pivot=3000.0), dict(saturation=20.0)):
        with pytest.raises(ValueError):
            hjd.color_matrix(**bad)
    assert max(abs(v) for v in hjd.color_matrix(brightness=7.99)[:9]) <= C.MAX_COEF
    doc = hjd.color_matrix.__doc__
    assert "torchvision" in doc and "clamp" in doc and "HSV" in doc and "YIQ" in doc and "M2 P1 + P2 (M1 + P1)" in doc


# ---- hjd_color_check --------------------------------------------------------------------------
def _item(hjd, src=0x10000, dst=0x20000, w=37, h=29, pitch=37, dst_pitch=37, rec=C.IDENTITY, reserved=0):
    return hjd._lib.HjdColorItem(src, dst, w, h, pitch, dst_pitch, (ctypes.c_int32 * 9)(*rec[:9]),
                                 (ctypes.c_int32 * 9)(*rec[9:18]), (ctypes.c_int32 * 3)(*rec[18:]), reserved)


def _check(hjd, items, n=None, fmt=PLANAR):
    arr = (hjd._lib.HjdColorItem * len(items))(*items)
    return hjd._lib.load().hjd_color_check(arr, len(items) if n is None else n, fmt), hjd._lib.error_string()


def _refused(hjd, match, items, **kw):
    rc, msg = _check(hjd, items, **kw)
    assert rc == -1, (rc, msg)   # HJD_E_INVALID
    assert re.search(match, msg), msg


def _with(k, v):
    rec = list(C.IDENTITY)
    rec[k] = v
    return rec


def test_color_check_accepts(hjd):
    ok = _item(hjd)
    limits = _item(hjd, src=0x10001, dst=0x30001, w=5, h=3, pitch=7, dst_pitch=5,
                   rec=[C.MAX_COEF, -C.MAX_COEF] * 9 + [C.MAX_OFFSET, -C.MAX_OFFSET, 0])
    assert _check(hjd, [ok, limits])[0] == 0
    assert _check(hjd, [_item(hjd, dst_pitch=74)], fmt=F16)[0] == 0 and _check(hjd, [_item(hjd, dst_pitch=148)], fmt=F32)[0] == 0
    assert _check(hjd, [_item(hjd, w=16384, h=16384, pitch=16384, dst_pitch=16384)])[0] == 0
    assert _check(hjd, [_item(hjd, w=1, h=1, pitch=1, dst_pitch=1)])[0] == 0
    assert _check(hjd, [_item(hjd, dst=0x10000)])[0] == 0           # in place: dst == src, equal pitches
    assert _check(hjd, [_item(hjd, pitch=1 << 30, dst_pitch=1 << 30)])[0] == 0   # pitches have no upper bound


def test_color_check_refuses_what_every_stage_refuses(hjd):
    ok = _item(hjd)
    assert hjd._lib.load().hjd_color_check(None, 1, PLANAR) == -1 and "NULL" in hjd._lib.error_string()
    for n in (0, -1, (1 << 20) + 1):
        _refused(hjd, "n = ", [ok], n=n)
    _refused(hjd, "color item 0: src or dst is NULL", [_item(hjd, src=0)])
    _refused(hjd, "color item 1: src or dst is NULL", [ok, _item(hjd, dst=0)])
    for bad in (0, -3, 16385):
        _refused(hjd, "item 0: source size", [_item(hjd, w=bad, pitch=1 << 20, dst_pitch=1 << 20)])
        _refused(hjd, "item 1: source size", [ok, _item(hjd, h=bad)])
    _refused(hjd, "src_pitch 36 is below", [_item(hjd, pitch=36)])
    _refused(hjd, "dst must be a multiple", [_item(hjd, dst=0x20001, dst_pitch=74)], fmt=F16)
    _refused(hjd, "dst must be a multiple", [_item(hjd, dst=0x20002, dst_pitch=148)], fmt=F32)


def test_color_check_refuses_a_bad_dst_pitch(hjd):
    _refused(hjd, "item 0: dst_pitch 36 must be >= 37", [_item(hjd, dst_pitch=36)])
    _refused(hjd, "dst_pitch 72 must be >= 74", [_item(hjd, dst_pitch=72)], fmt=F16)      # below 2 * 37
    _refused(hjd, "dst_pitch 75 .*multiple of 2", [_item(hjd, dst_pitch=75)], fmt=F16)
    _refused(hjd, "dst_pitch 150 .*multiple of 4", [_item(hjd, dst_pitch=150)], fmt=F32)


def test_color_check_refuses_a_coefficient_out_of_range(hjd):
    for k in (0, 4, 8, 9, 13, 17):
        for v in (32768, -32768, 1 << 20, -(1 << 31)):
            name = f"{'m' if k < 9 else 'p'}\\[{k % 9}\\] = {v}"
            _refused(hjd, f"item 1: {name} is outside -32767..32767", [_item(hjd), _item(hjd, rec=_with(k, v))])
    assert _check(hjd, [_item(hjd, rec=_with(17, -32767))])[0] == 0


def test_color_check_refuses_an_offset_out_of_range(hjd):
    for k in (18, 19, 20):
        for v in ((1 << 23) + 1, -(1 << 23) - 1, (1 << 31) - 1):
            _refused(hjd, f"item 0: t\\[{k - 18}\\] = {v} is outside", [_item(hjd, rec=_with(k, v))])
    assert _check(hjd, [_item(hjd, rec=_with(20, -(1 << 23)))])[0] == 0


def test_color_check_refuses_reserved_and_formats(hjd):
    _refused(hjd, "item 0: reserved must be 0", [_item(hjd, reserved=1)])
    _refused(hjd, "item 1: reserved must be 0", [_item(hjd), _item(hjd, reserved=-1)])
    for fmt in (0, 1, 2, 4, 7, -1):
        _refused(hjd, "output format", [_item(hjd)], fmt=fmt)


# ---- interfaces -------------------------------------------------------------------------------
def test_color_entry_points_are_bound(hjd):
    lib = hjd._lib.load()
    for name in ("hjd_color_check", "hjd_color_create", "hjd_color_set_normalize", "hjd_color_launch",
                 "hjd_color_destroy", "hjd_gdec_decode_resized_color", "hjd_gdec_decode_warped_color"):
        assert name in hjd._lib.SIGNATURES and getattr(lib, name).argtypes == hjd._lib.SIGNATURES[name][1]
        for header in ("hjd.h", "hjd_host.h"):
            if re.search(rf"\b{name}\(", open(os.path.join(REPO, "include", header)).read()):
                break
        else:
            raise AssertionError(f"{name} is in no header")
    header = open(os.path.join(REPO, "include", "hjd.h")).read()
    m = re.search(r"typedef struct hjd_color_item \{([^}]*)\} hjd_color_item;", header)
    assert m
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [d.strip() for d in fields.split(";") if d.strip()]
    assert decls == ["const void* src", "void* dst", "int32_t w, h, src_pitch, dst_pitch", "int32_t m[9], p[9], t[3]",
                     "int32_t reserved"]
    assert 2 * 8 + 4 * 4 + 21 * 4 + 4 == 120 == ctypes.sizeof(hjd._lib.HjdColorItem)
    I = hjd._lib.HjdColorItem
    assert [getattr(I, f).offset for f in ("src", "dst", "w", "h", "src_pitch", "dst_pitch", "m", "p", "t", "reserved")] == \
        [0, 8, 16, 20, 24, 28, 32, 68, 104, 116]
    assert "#define HJD_ABI_VERSION 1" in header and lib.hjd_abi_version() == 1
    assert "#define HJD_COLOR_MAX_COEF 32767" in header and "#define HJD_COLOR_MAX_OFFSET (1 << 23)" in header
    assert lib.hjd_color_launch(None, None) == -1
    one = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.hjd_color_set_normalize(None, one, one) == -1
    assert lib.hjd_color_destroy(None) == 0
    assert lib.hjd_color_create(None, None, 1, PLANAR, None) == -1
    assert lib.hjd_gdec_decode_resized_color(None, None, None, 1, None, None, None, None, None, 8, 8, 8, 0, None) == -1
    assert lib.hjd_gdec_decode_warped_color(None, None, None, 1, None, None, None, None, None, None, 8, 8, 8, None) == -1


def test_color_python_interface(hjd):
    for name in ("Color", "color_matrix", "COLOR_IDENTITY"):
        assert name in hjd.__all__ and hasattr(hjd, name)
    assert tuple(hjd.COLOR_IDENTITY) == C.IDENTITY
    assert list(inspect.signature(hjd.Color.__init__).parameters) == ["self", "ctx", "srcs", "outs", "colors", "normalize"]
    for method in ("launch", "set_normalize", "close"):
        assert callable(getattr(hjd.Color, method))
    p = inspect.signature(hjd.color_matrix).parameters
    assert list(p) == ["brightness", "contrast", "saturation", "hue", "gray", "invert", "order", "pivot"]
    assert [p[k].default for k in p] == [1.0, 1.0, 1.0, 0.0, False, False,
                                         ("brightness", "contrast", "saturation", "hue"), "mean"]
    G = hjd.GpuDecoder
    base = list(inspect.signature(G.decode_rgb_resized).parameters)
    assert {"apply_exif_orientation", "orientations"} <= set(base)
    assert list(inspect.signature(G.decode_rgb_resized_color).parameters) == base + ["colors"]
    assert list(inspect.signature(G.decode_rgb_warped_color).parameters) == \
        list(inspect.signature(G.decode_rgb_warped).parameters) + ["colors"]
    for fn, ref in ((G.decode_rgb_resized_color, G.decode_rgb_resized), (G.decode_rgb_warped_color, G.decode_rgb_warped)):
        a, b = inspect.signature(fn).parameters, inspect.signature(ref).parameters
        assert all(a[k].default == b[k].default for k in b if k != "self")
