"""The tone stage without a device: the numpy model of include/hjd.h's
definition (tests/tone_model.py) against Pillow, hjd_tone_curve_from_histogram
-- the function the device's curve-building kernel calls -- against the model,
tone_curve(), hjd_tone_check's refusals, and the interfaces."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import tone_model as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANAR, F16, F32 = 3, 5, 6


# ---- the model against Pillow -----------------------------------------------------------------
def _pillow_images():
    """The four shapes of the issue, seeded: (3, h, w) uint8."""
    rng = np.random.default_rng(2025)
    return {"37x53 values 30..199": rng.integers(30, 200, (3, 53, 37), dtype=np.uint8),
            "224x224 full range": rng.integers(0, 256, (3, 224, 224), dtype=np.uint8),
            "8x8 (step 0)": rng.integers(0, 256, (3, 8, 8), dtype=np.uint8),
            "64x64 values 100..102": rng.integers(100, 103, (3, 64, 64), dtype=np.uint8)}


def _pillow(op, src):
    from PIL import Image, ImageOps
    img = Image.fromarray(np.ascontiguousarray(src.transpose(1, 2, 0)), "RGB")
    return np.asarray(op(ImageOps, img)).transpose(2, 0, 1)


@pytest.mark.parametrize("name", list(_pillow_images()))
def test_model_agrees_with_pillow(name):
    src = _pillow_images()[name]
    if name.startswith("8x8"):   # 64 pixels: step = (64 - last) // 255 = 0
        assert all((64 - int(T.histogram(src)[c][src[c].max()])) // 255 == 0 for c in range(3))
    assert np.array_equal(T.tone_u8(src, T.EQUALIZE), _pillow(lambda ops, im: ops.equalize(im), src))
    sol = np.where(np.arange(256) < 128, np.arange(256), 255 - np.arange(256)).astype(np.uint8)
    assert np.array_equal(T.tone_u8(src, T.TABLE, np.tile(sol, (3, 1))), _pillow(lambda ops, im: ops.solarize(im, 128), src))
    post = (np.arange(256) & 0xE0).astype(np.uint8)
    assert np.array_equal(T.tone_u8(src, T.TABLE, np.tile(post, (3, 1))), _pillow(lambda ops, im: ops.posterize(im, 3), src))
    # Pillow's autocontrast is int(v * (255.0 / (hi - lo)) - lo * scale) in float64: the documented difference
    auto = T.tone_u8(src, T.AUTOCONTRAST).astype(np.int64) - _pillow(lambda ops, im: ops.autocontrast(im), src).astype(np.int64)
    assert np.abs(auto).max() <= 1


def test_model_laws():
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (3, 9, 11), dtype=np.uint8)
    read = []
    assert np.array_equal(T.tone_u8(src, T.TABLE, T.IDENTITY, read), src) and not read   # a copy; no histogram read
    T.tone_u8(src, T.EQUALIZE, T.IDENTITY, read)
    assert read == [True]
    flat = np.full((3, 5, 3), 200, np.uint8)   # one bin: both data curves are the identity
    assert np.array_equal(T.tone_u8(flat, T.AUTOCONTRAST), flat) and np.array_equal(T.tone_u8(flat, T.EQUALIZE), flat)
    two = np.where(rng.random((3, 40, 40)) < 0.5, 90, 160).astype(np.uint8)
    assert set(np.unique(T.tone_u8(two, T.AUTOCONTRAST))) == {0, 255}


# ---- hjd_tone_curve_from_histogram against the model ------------------------------------------
def _curve(hjd, mode, hist, lut=None):
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    assert h.shape == (3, 256)
    out = np.full((3, 256), 0xA5, np.uint8)
    lin = None if lut is None else np.ascontiguousarray(lut, dtype=np.uint8)
    rc = hjd._lib.load().hjd_tone_curve_from_histogram(mode, h.ctypes.data, None if lin is None else lin.ctypes.data,
                                                      out.ctypes.data)
    assert rc == 0, hjd._lib.error_string()
    return out


def _sparse(bins):
    """(3, 256) counts: `bins` {v: count} in channel 0, shifted by one and two bins in the others."""
    h = np.zeros((3, 256), np.int64)
    for c in range(3):
        for v, k in bins.items():
            h[c][min(255, v + c)] += k
    return h


def _edge_histograms():
    rng = np.random.default_rng(99)
    for _ in range(24):   # random, dense and sparse
        h = rng.integers(0, 5000, (3, 256))
        yield "random", np.where(rng.random((3, 256)) < rng.random(), h, 0)
    yield "empty", np.zeros((3, 256), np.int64)
    yield "one bin", _sparse({77: 1234})
    yield "two bins", _sparse({10: 300, 200: 500})
    yield "two bins, few pixels", _sparse({10: 3, 200: 500})
    for rest in (254, 255, 509, 510):   # N - last: step 0, 1, 1, 2
        yield f"N - last = {rest}", _sparse({5: rest - 100, 17: 60, 99: 40, 180: 7777})
    yield "a bin of 2^28", _sparse({131: 1 << 28})
    yield "a bin of 2^28 - 4000 below others", _sparse({3: (1 << 28) - 4000, 9: 1500, 250: 2500})
    yield "a bin of 2^28 - 4000 above others", _sparse({3: 1500, 9: 2500, 250: (1 << 28) - 4000})
    yield "lo = 0, hi = 255", np.stack([_sparse({0: 10, 128: 5, 253: 9})[0], _sparse({0: 1, 255: 1})[0],
                                       _sparse({0: 700, 1: 5, 254: 3, 255: 900})[0]])
    yield "hi = lo + 1", _sparse({100: 400, 101: 300})
    yield "hi = lo + 1 at the top", np.stack([_sparse({254: 400, 255: 300})[0]] * 3)


@pytest.mark.parametrize("mode", [T.TABLE, T.AUTOCONTRAST, T.EQUALIZE])
def test_curve_from_histogram_is_the_model(hjd, mode):
    rng = np.random.default_rng(5)
    lut = rng.integers(0, 256, (3, 256), dtype=np.uint8)
    for name, hist in _edge_histograms():
        assert np.array_equal(_curve(hjd, mode, hist), T.composed(mode, hist)), (name, mode)
        assert np.array_equal(_curve(hjd, mode, hist, lut), T.composed(mode, hist, lut)), (name, mode, "table")


def test_curve_from_histogram_steps_and_refusals(hjd):
    """The steps the N - last cases are named for, and what the function refuses."""
    for rest, step in ((254, 0), (255, 1), (509, 1), (510, 2)):
        hist = _sparse({5: rest - 100, 17: 60, 99: 40, 180: 7777})
        assert (int(hist[0].sum()) - 7777) // 255 == step
        got = _curve(hjd, T.EQUALIZE, hist)
        assert np.array_equal(got[0], np.arange(256)) == (step == 0)
    lib = hjd._lib.load()
    h, out = np.zeros((3, 256), np.uint32), np.zeros((3, 256), np.uint8)
    for mode in (-1, 3):
        assert lib.hjd_tone_curve_from_histogram(mode, h.ctypes.data, None, out.ctypes.data) == -1
        assert "mode" in hjd._lib.error_string()
    assert lib.hjd_tone_curve_from_histogram(0, None, None, out.ctypes.data) == -1
    assert lib.hjd_tone_curve_from_histogram(0, h.ctypes.data, None, None) == -1
    h[1][4], h[1][9] = 1 << 28, 1
    assert lib.hjd_tone_curve_from_histogram(2, h.ctypes.data, None, out.ctypes.data) == -1
    assert "2^28" in hjd._lib.error_string()


# ---- tone_curve -------------------------------------------------------------------------------
def test_tone_curve_defaults_are_the_identity(hjd):
    assert np.array_equal(hjd.TONE_IDENTITY, T.IDENTITY) and hjd.TONE_IDENTITY.dtype == np.uint8
    t = hjd.tone_curve()
    assert t.dtype == np.uint8 and t.shape == (3, 256) and np.array_equal(t, hjd.TONE_IDENTITY)
    assert (hjd.TONE_TABLE, hjd.TONE_AUTOCONTRAST, hjd.TONE_EQUALIZE) == (T.TABLE, T.AUTOCONTRAST, T.EQUALIZE)


def test_tone_curve_single_operations(hjd):
    v = np.arange(256)
    for t in (0, 1, 128, 200, 256):
        assert np.array_equal(hjd.tone_curve(solarize=t), np.tile(np.where(v < t, v, 255 - v), (3, 1)))
    for b in range(1, 9):
        assert np.array_equal(hjd.tone_curve(posterize=b), np.tile(v & (0xFF00 >> b) & 0xFF, (3, 1)))
    for g in (0.45, 1.0, 2.2):
        want = np.array([int(np.floor(255.0 * (k / 255.0) ** g + 0.5)) for k in range(256)])
        assert np.array_equal(hjd.tone_curve(gamma=g), np.tile(want, (3, 1)))
    assert np.array_equal(hjd.tone_curve(gamma=1.0), T.IDENTITY)
    assert np.array_equal(hjd.tone_curve(invert=True), np.tile(255 - v, (3, 1)))
    rng = np.random.default_rng(3)
    one, three = rng.integers(0, 256, 256), rng.integers(0, 256, (3, 256))
    assert np.array_equal(hjd.tone_curve(table=one), np.tile(one, (3, 1)))
    assert np.array_equal(hjd.tone_curve(table=three), three)


def test_tone_curve_order_law(hjd):
    """Applied in `order`, then invert, then table: the table of a composition is the composition of the tables."""
    def then(first, second):
        return np.take_along_axis(second, first.astype(np.int64), axis=1)

    g, p, s = hjd.tone_curve(gamma=0.6), hjd.tone_curve(posterize=2), hjd.tone_curve(solarize=100)
    assert np.array_equal(hjd.tone_curve(gamma=0.6, posterize=2, solarize=100), then(then(g, p), s))   # the default order
    assert np.array_equal(hjd.tone_curve(gamma=0.6, posterize=2, solarize=100, order=("solarize", "posterize", "gamma")),
                          then(then(s, p), g))
    assert not np.array_equal(then(p, s), then(s, p))   # (the order matters on this pair)
    assert np.array_equal(hjd.tone_curve(posterize=2, solarize=100, order=("solarize", "gamma", "posterize")), then(s, p))
    rng = np.random.default_rng(4)
    table = rng.integers(0, 256, (3, 256), dtype=np.uint8)
    assert np.array_equal(hjd.tone_curve(solarize=100, invert=True, table=table),
                          then(then(s, hjd.tone_curve(invert=True)), table))


def test_tone_curve_checks_its_arguments(hjd):
    for kw in ({"solarize": -1}, {"solarize": 257}, {"solarize": 1.5}, {"posterize": 0}, {"posterize": 9},
               {"posterize": 2.5}, {"gamma": 0.0}, {"gamma": -1.0}, {"gamma": float("nan")}, {"gamma": float("inf")},
               {"order": ("gamma", "solarize")}, {"order": ("gamma", "solarize", "solarize")},
               {"table": np.arange(255)}, {"table": np.full((3, 256), 256)}, {"table": np.full(256, -1)},
               {"table": np.zeros((3, 256), np.float32)}):
        with pytest.raises(ValueError):
            hjd.tone_curve(**kw)


# ---- hjd_tone_check ---------------------------------------------------------------------------
def _item(hjd, src=0x10000, dst=0x20000, w=37, h=29, pitch=37, dst_pitch=37, mode=0, reserved=0):
    it = hjd._lib.HjdToneItem(src, dst, w, h, pitch, dst_pitch)
    it.curve.mode, it.curve.reserved = mode, reserved
    ctypes.memmove(it.curve.lut, T.IDENTITY.tobytes(), 768)
    return it


def _check(hjd, items, n=None, fmt=PLANAR):
    arr = (hjd._lib.HjdToneItem * len(items))(*items)
    return hjd._lib.load().hjd_tone_check(arr, len(items) if n is None else n, fmt), hjd._lib.error_string()


def _refused(hjd, match, items, **kw):
    rc, msg = _check(hjd, items, **kw)
    assert rc == -1, (rc, msg)   # HJD_E_INVALID
    assert re.search(match, msg), msg


def test_tone_check_accepts(hjd):
    assert _check(hjd, [_item(hjd), _item(hjd, src=0x10001, dst=0x30001, w=5, h=3, pitch=7, dst_pitch=5, mode=2)])[0] == 0
    for mode in (0, 1, 2):
        assert _check(hjd, [_item(hjd, mode=mode)])[0] == 0
    assert _check(hjd, [_item(hjd, dst_pitch=74)], fmt=F16)[0] == 0 and _check(hjd, [_item(hjd, dst_pitch=148)], fmt=F32)[0] == 0
    assert _check(hjd, [_item(hjd, w=16384, h=16384, pitch=16384, dst_pitch=16384)])[0] == 0
    assert _check(hjd, [_item(hjd, w=1, h=1, pitch=1, dst_pitch=1)])[0] == 0
    assert _check(hjd, [_item(hjd, dst=0x10000)])[0] == 0           # in place: dst == src, equal pitches
    assert _check(hjd, [_item(hjd, pitch=1 << 30, dst_pitch=1 << 30)])[0] == 0   # pitches have no upper bound


def test_tone_check_refuses_null_items_and_n(hjd):
    assert hjd._lib.load().hjd_tone_check(None, 1, PLANAR) == -1 and "NULL" in hjd._lib.error_string()
    for n in (0, -1, (1 << 20) + 1):
        _refused(hjd, "n = ", [_item(hjd)], n=n)


def test_tone_check_refuses_null_pointers(hjd):
    _refused(hjd, "tone item 0: src or dst is NULL", [_item(hjd, src=0)])
    _refused(hjd, "tone item 1: src or dst is NULL", [_item(hjd), _item(hjd, dst=0)])


def test_tone_check_refuses_dimensions(hjd):
    for bad in (0, -3, 16385):
        _refused(hjd, "item 0: source size", [_item(hjd, w=bad, pitch=1 << 20, dst_pitch=1 << 20)])
        _refused(hjd, "item 1: source size", [_item(hjd), _item(hjd, h=bad)])


def test_tone_check_refuses_a_short_src_pitch(hjd):
    _refused(hjd, "src_pitch 36 is below", [_item(hjd, pitch=36)])


def test_tone_check_refuses_a_misaligned_dst(hjd):
    _refused(hjd, "dst must be a multiple", [_item(hjd, dst=0x20001, dst_pitch=74)], fmt=F16)
    _refused(hjd, "dst must be a multiple", [_item(hjd, dst=0x20002, dst_pitch=148)], fmt=F32)


def test_tone_check_refuses_a_bad_dst_pitch(hjd):
    _refused(hjd, "item 0: dst_pitch 36 must be >= 37", [_item(hjd, dst_pitch=36)])
    _refused(hjd, "dst_pitch 72 must be >= 74", [_item(hjd, dst_pitch=72)], fmt=F16)      # below 2 * 37
    _refused(hjd, "dst_pitch 75 .*multiple of 2", [_item(hjd, dst_pitch=75)], fmt=F16)
    _refused(hjd, "dst_pitch 150 .*multiple of 4", [_item(hjd, dst_pitch=150)], fmt=F32)


def test_tone_check_refuses_a_mode_out_of_range(hjd):
    for mode in (3, -1, 1 << 20, -(1 << 31)):
        _refused(hjd, f"item 1: mode {mode} is outside 0..2", [_item(hjd), _item(hjd, mode=mode)])


def test_tone_check_refuses_reserved(hjd):
    _refused(hjd, "item 0: reserved must be 0", [_item(hjd, reserved=1)])
    _refused(hjd, "item 1: reserved must be 0", [_item(hjd), _item(hjd, reserved=-1)])


def test_tone_check_refuses_formats(hjd):
    for fmt in (0, 1, 2, 4, 7, -1):
        _refused(hjd, "output format", [_item(hjd)], fmt=fmt)


# ---- interfaces -------------------------------------------------------------------------------
def test_tone_entry_points_are_bound(hjd):
    lib = hjd._lib.load()
    for name in ("hjd_tone_check", "hjd_tone_create", "hjd_tone_set_normalize", "hjd_tone_launch", "hjd_tone_destroy",
                 "hjd_tone_curve_from_histogram", "hjd_gdec_decode_resized_tone", "hjd_gdec_decode_warped_tone"):
        assert name in hjd._lib.SIGNATURES and getattr(lib, name).argtypes == hjd._lib.SIGNATURES[name][1]
        for header in ("hjd.h", "hjd_host.h"):
            if re.search(rf"\b{name}\(", open(os.path.join(REPO, "include", header)).read()):
                break
        else:
            raise AssertionError(f"{name} is in no header")
    header = open(os.path.join(REPO, "include", "hjd.h")).read()
    assert "enum { HJD_TONE_TABLE = 0, HJD_TONE_AUTOCONTRAST = 1, HJD_TONE_EQUALIZE = 2 };" in header
    for struct, want in (("hjd_tone_curve", ["int32_t mode", "int32_t reserved", "uint8_t lut[3][256]"]),
                         ("hjd_tone_item", ["const void* src", "void* dst", "int32_t w, h, src_pitch, dst_pitch",
                                            "hjd_tone_curve curve"])):
        m = re.search(rf"typedef struct {struct} \{{([^}}]*)\}} {struct};", header)
        assert m, struct
        fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert [d.strip() for d in fields.split(";") if d.strip()] == want
    C, I = hjd._lib.HjdToneCurve, hjd._lib.HjdToneItem
    assert 4 + 4 + 768 == 776 == ctypes.sizeof(C) and 2 * 8 + 4 * 4 + 776 == 808 == ctypes.sizeof(I)
    assert [getattr(C, f).offset for f in ("mode", "reserved", "lut")] == [0, 4, 8]
    assert [getattr(I, f).offset for f in ("src", "dst", "w", "h", "src_pitch", "dst_pitch", "curve")] == \
        [0, 8, 16, 20, 24, 28, 32]
    assert "#define HJD_ABI_VERSION 1" in header and lib.hjd_abi_version() == 1
    assert lib.hjd_tone_launch(None, None) == -1
    one = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.hjd_tone_set_normalize(None, one, one) == -1
    assert lib.hjd_tone_destroy(None) == 0
    assert lib.hjd_tone_create(None, None, 1, PLANAR, None) == -1
    assert lib.hjd_gdec_decode_resized_tone(None, None, None, 1, None, None, None, None, None, None, 8, 8, 8, 0, None) == -1
    assert lib.hjd_gdec_decode_warped_tone(None, None, None, 1, None, None, None, None, None, None, None, 8, 8, 8,
                                           None) == -1


def test_tone_python_interface(hjd):
    for name in ("Tone", "tone_curve", "TONE_TABLE", "TONE_AUTOCONTRAST", "TONE_EQUALIZE", "TONE_IDENTITY"):
        assert name in hjd.__all__ and hasattr(hjd, name)
    assert list(inspect.signature(hjd.Tone.__init__).parameters) == ["self", "ctx", "srcs", "outs", "curves", "modes",
                                                                     "normalize"]
    for method in ("launch", "set_normalize", "close"):
        assert callable(getattr(hjd.Tone, method))
    p = inspect.signature(hjd.tone_curve).parameters
    assert list(p) == ["solarize", "posterize", "gamma", "invert", "table", "order"]
    assert [p[k].default for k in p] == [None, None, None, False, None, ("gamma", "posterize", "solarize")]
    G = hjd.GpuDecoder
    assert list(inspect.signature(G.decode_rgb_resized_tone).parameters) == \
        list(inspect.signature(G.decode_rgb_resized_color).parameters) + ["curves", "modes"]
    assert list(inspect.signature(G.decode_rgb_warped_tone).parameters) == \
        list(inspect.signature(G.decode_rgb_warped_color).parameters) + ["curves", "modes"]
    for fn, ref in ((G.decode_rgb_resized_tone, G.decode_rgb_resized), (G.decode_rgb_warped_tone, G.decode_rgb_warped)):
        a, b = inspect.signature(fn).parameters, inspect.signature(ref).parameters
        assert all(a[k].default == b[k].default for k in b if k != "self")
