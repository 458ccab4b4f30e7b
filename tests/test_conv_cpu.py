"""The filter stage without a device: hjd_conv_apply_host -- which runs the two
functions the device's kernel calls (csrc/hjd_conv_math.h) -- against the numpy
model of include/hjd.h's definition (tests/conv_model.py), the overflow pins,
the model against scipy and Pillow, conv_gaussian(), conv_sharpness() and
conv_unsharp(), hjd_conv_check's refusals, and the interfaces.

The tests that use only the model, scipy and Pillow
(test_model_laws, test_model_overflow_pins, test_model_agrees_with_scipy_on_q12_taps)
pass without the library's filter stage; all others need its names."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import conv_model as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANAR, F16, F32 = 3, 5, 6
BORDERS = (C.KEEP, C.REFLECT, C.REPLICATE)
RADII = ((0, 0), (1, 1), (3, 0), (0, 5), (11, 1), (11, 11))


def _taps(rng, r, total=4096):
    """2 r + 1 random taps summing to `total`, none 0 at the ends."""
    k = rng.integers(1, 400, 2 * r + 1)
    k = (k * (total - (2 * r + 1)) // k.sum()) + 1
    k[r] += total - k.sum()
    assert k.sum() == total and k.min() >= 1
    return [int(v) for v in k]


def _ctypes_filter(hjd, f, reserved=0):
    cf = hjd._lib.HjdConvFilter(f["rx"], f["ry"], f["border"], f["a"], f["b"], reserved)
    for p, v in enumerate(f["kh"]):
        cf.kh[p] = v
    for p, v in enumerate(f["kv"]):
        cf.kv[p] = v
    return cf


def _host(hjd, src, f, spad=0, dpad=0):
    """hjd_conv_apply_host on (3, h, w) uint8 with padded rows; the padding of the output must stay 0xA5."""
    _, h, w = src.shape
    s = np.full((3, h, w + spad), 0x3C, np.uint8)
    s[..., :w] = src
    d = np.full((3, h, w + dpad), 0xA5, np.uint8)
    cf = _ctypes_filter(hjd, f)
    rc = hjd._lib.load().hjd_conv_apply_host(s.ctypes.data, w, h, w + spad, ctypes.byref(cf), d.ctypes.data, w + dpad)
    assert rc == 0, hjd._lib.error_string()
    assert (d[..., w:] == 0xA5).all()
    return d[..., :w].copy()


# ---- hjd_conv_apply_host against the model ----------------------------------------------------
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("rx,ry", RADII)
def test_host_reference_is_the_model(hjd, border, rx, ry):
    rng = np.random.default_rng(100 * rx + ry + 7 * border)
    # (w, h): ordinary; REFLECT at r = dim - 1; KEEP with 2 r >= dim; one row / column where legal
    sizes = [(37, 29), (rx + 1, ry + 1), (max(1, 2 * rx), max(1, 2 * ry)), (2 * rx + 1, 2 * ry + 1), (64 + rx, ry + 2), (rx + 3, 40)]
    if border != C.REFLECT:
        sizes += [(1, 1), (max(1, rx), max(1, ry)), (5, 1), (1, 9)]
    for k, (w, h) in enumerate(sizes):
        src = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        for a, b in ((0, 4096), (6932, -2836), (-4096, 8192), (1 << 20, -(1 << 20) + 977)):
            f = C.record(_taps(rng, rx), _taps(rng, ry, 4096 if k % 2 else 3000), a, b, border)
            assert C.legal(f, w, h)
            got = _host(hjd, src, f, spad=k % 3, dpad=(k + 1) % 3)
            assert np.array_equal(got, C.conv_u8(src, f)), (w, h, rx, ry, border, a, b)


def test_host_reference_refuses(hjd):
    lib = hjd._lib.load()
    s, d = np.zeros((3, 4, 4), np.uint8), np.zeros((3, 4, 4), np.uint8)

    def call(f, w=4, h=4, sp=4, dp=4, src=s, dst=d, reserved=0):
        cf = _ctypes_filter(hjd, f, reserved)
        return lib.hjd_conv_apply_host(src.ctypes.data, w, h, sp, ctypes.byref(cf), dst.ctypes.data, dp)
    assert call(C.IDENTITY) == 0
    assert call(C.record([1, 4094, 1], [4096], 0, 4096, C.REFLECT), w=1, sp=1, dp=1) == -1 and "REFLECT" in hjd._lib.error_string()
    assert call(C.IDENTITY, sp=3) == -1 and call(C.IDENTITY, dp=3) == -1 and call(C.IDENTITY, w=0) == -1
    assert call(C.IDENTITY, dst=s) == -1 and "in place" in hjd._lib.error_string()
    assert call(C.IDENTITY, reserved=1) == -1 and "reserved" in hjd._lib.error_string()
    assert lib.hjd_conv_apply_host(s.ctypes.data, 4, 4, 4, None, d.ctypes.data, 4) == -1
    assert lib.hjd_conv_apply_host(None, 4, 4, 4, ctypes.byref(_ctypes_filter(hjd, C.IDENTITY)), d.ctypes.data, 4) == -1


# ---- the laws and the overflow pins -----------------------------------------------------------
def test_model_laws():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (3, 9, 14), dtype=np.uint8)
    assert np.array_equal(C.conv_u8(src, C.IDENTITY), src)
    for border in BORDERS:
        f = C.record(_taps(rng, 2), _taps(rng, 3), 0, 4096, border)
        for v in (0, 1, 131, 255):   # a flat image stays flat
            flat = np.full((3, 9, 14), v, np.uint8)
            assert np.array_equal(C.conv_u8(flat, f), flat)
        mixed = src.copy()
        mixed[1] = 255 - mixed[1]
        assert np.array_equal(C.conv_u8(mixed, f)[0], C.conv_u8(src, f)[0])   # channels are independent
    # KEEP: the band is copied, the interior is REPLICATE's (it never reads outside)
    f = C.record(_taps(rng, 2), _taps(rng, 1), 9000, -4904, C.KEEP)
    out, rep = C.conv_u8(src, f), C.conv_u8(src, dict(f, border=C.REPLICATE))
    assert np.array_equal(out[:, 1:-1, 2:-2], rep[:, 1:-1, 2:-2])
    band = np.ones((9, 14), bool)
    band[1:-1, 2:-2] = False
    assert np.array_equal(out[:, band], src[:, band]) and not np.array_equal(out, src)
    # REFLECT is torch's reflect / numpy's "reflect" padding, REPLICATE numpy's "edge"
    g = C.record([4096], _taps(rng, 3), 0, 4096, C.REFLECT)
    pad = np.pad(src.astype(np.int64), ((0, 0), (3, 3), (0, 0)), mode="reflect")
    S = sum(k * pad[:, q:q + 9] for q, k in enumerate(g["kv"])) * 4096
    assert np.array_equal(C.conv_u8(src, g), ((S + (1 << 23)) >> 24).astype(np.uint8))


def _pins():
    """(name, src value or array, record, expected byte or None)."""
    full = [0] * 11 + [4096] + [0] * 11
    spread = [178] * 22 + [180]   # 23 taps summing to 4096
    assert sum(spread) == 4096
    yield "flat 255, full taps: S = 255 << 24 is above int32", 255, C.record(spread, spread, 0, 4096, C.REFLECT), 255
    yield "flat 255, a delta of 4096", 255, C.record(full, full, 0, 4096, C.REPLICATE), 255
    yield "a = 2^20, b = -2^20: T = 0", 255, C.record(spread, spread, 1 << 20, -(1 << 20), C.REFLECT), 0
    yield "a = -2^20, b = 2^20: T = 0", 255, C.record(spread, spread, -(1 << 20), 1 << 20, C.REFLECT), 0
    yield "a = 2^20 alone clamps to 255", 1, C.record([4096], [4096], 1 << 20, 0, C.KEEP), 255
    yield "b = -2^20 alone clamps to 0", 255, C.record(spread, spread, 0, -(1 << 20), C.REPLICATE), 0
    # negative T: the shift is arithmetic.  x = 200 under unit taps, S = 200 << 24.  b = -11: T + 2^35 = -152 << 24, just
    # below 0, shifts to -1 and clamps to 0 (a logical shift gives 2^28 - 1, which clamps to 255); b = -2048: T = -100 << 36
    yield "T + 2^35 just below 0 floors to -1 and clamps to 0", 200, C.record([4096], [4096], 0, -11, C.KEEP), 0
    yield "a large negative T clamps to 0", 200, C.record([4096], [4096], 0, -2048, C.KEEP), 0


def test_model_overflow_pins():
    for name, v, f, want in _pins():
        out = C.conv_u8(np.full((3, 30, 40), v, np.uint8), f)
        assert (out == want).all(), name
    # the one rounding, to nearest with halves up, behind a difference of two large products
    f = C.record([4096], [4096], 8192, -6144, C.KEEP)
    assert (C.conv_u8(np.full((3, 2, 2), 100, np.uint8), f) == 50).all()       # T = 50 << 36 exactly: 50
    f = C.record([4096], [4096], 8192, -6143, C.KEEP)                            # T = 50 << 36 + 100 << 24: still 50
    assert (C.conv_u8(np.full((3, 2, 2), 100, np.uint8), f) == 50).all()
    f = C.record([4096], [4096], 4096, -2048, C.KEEP)                            # T = 101 << 35: 50.5 rounds up to 51
    assert (C.conv_u8(np.full((3, 2, 2), 101, np.uint8), f) == 51).all()


def test_host_overflow_pins(hjd):
    for name, v, f, want in _pins():
        out = _host(hjd, np.full((3, 30, 40), v, np.uint8), f)
        assert (out == want).all(), name
    rng = np.random.default_rng(17)
    src = rng.integers(0, 256, (3, 12, 12), dtype=np.uint8)
    for a, b in ((-1, 0), (-(1 << 20), (1 << 20) - 1), (4096, -4097), (1, -1), (-3000, 2999)):   # negative T: the flooring shift
        f = C.record(_taps(rng, 1), _taps(rng, 1), a, b, C.REPLICATE)
        assert np.array_equal(_host(hjd, src, f), C.conv_u8(src, f)), (a, b)


# ---- Gaussian filters -------------------------------------------------------------------------
SIGMAS = (0.1, 0.5, 1.0, 2.0)


def _gauss_image():
    rng = np.random.default_rng(77)
    return rng.integers(0, 256, (3, 45, 52), dtype=np.uint8)


def _scipy_blur(src, kh, kv):
    """correlate1d(mode="mirror") on both axes in float64 with real taps."""
    from scipy.ndimage import correlate1d
    x = src.astype(np.float64)
    x = correlate1d(x, np.asarray(kh, np.float64), axis=2, mode="mirror")
    return correlate1d(x, np.asarray(kv, np.float64), axis=1, mode="mirror")


def test_model_agrees_with_scipy_on_q12_taps():
    """The same real map with one rounding: within 0.5 (+ float64 noise) of scipy with taps / 4096."""
    rng = np.random.default_rng(5)
    src = _gauss_image()
    for rx, ry in ((1, 1), (3, 0), (0, 5), (11, 11)):
        f = C.record(_taps(rng, rx), _taps(rng, ry), 0, 4096, C.REFLECT)
        want = _scipy_blur(src, np.array(f["kh"]) / 4096.0, np.array(f["kv"]) / 4096.0)
        assert np.abs(C.conv_u8(src, f).astype(np.float64) - want).max() <= 0.5 + 1e-6


@pytest.mark.parametrize("sigma", SIGMAS)
def test_conv_gaussian_taps_and_error_bound(hjd, sigma):
    from ocljpegdecoder_amd.backend import _gaussian_real
    rec = hjd.conv_gaussian(sigma)
    f = C.from_numpy(rec)
    assert sum(f["kh"]) == 4096 and sum(f["kv"]) == 4096 and f["kh"] == f["kv"]
    assert (f["a"], f["b"], f["border"]) == (0, 4096, C.REFLECT)
    ksize = min(23, 2 * int(np.ceil(3 * sigma)) + 1)
    assert f["rx"] <= ksize // 2 and (f["rx"] == 0 or f["kh"][0] or f["kh"][-1])   # trimmed: an end tap is not 0
    real = _gaussian_real(sigma, ksize)
    t = np.linspace(-(ksize - 1) / 2, (ksize - 1) / 2, ksize)
    assert np.allclose(real, np.exp(-0.5 * (t / sigma) ** 2) / np.exp(-0.5 * (t / sigma) ** 2).sum(), rtol=0, atol=1e-15)
    trim = (ksize - len(f["kh"])) // 2
    q = np.zeros(ksize)
    q[trim:ksize - trim] = np.array(f["kh"]) / 4096.0
    assert np.abs(q * 4096 - real * 4096).max() < 1.0   # largest remainder: every tap is floor or floor + 1
    # against the unquantised taps: 0.5 + 255 (2 e + e^2), e the taps' total error per axis
    e = np.abs(q - real).sum()
    bound = 0.5 + 255.0 * (2 * e + e * e)
    src = _gauss_image()
    diff = np.abs(C.conv_u8(src, f).astype(np.float64) - _scipy_blur(src, real, real)).max()
    print(f"sigma {sigma}: radius {f['rx']}, e = {e:.6f}, max |model - float64| = {diff:.4f}, bound {bound:.4f}")
    assert diff <= bound
    got = _host(hjd, src, f)
    assert np.array_equal(got, C.conv_u8(src, f))
    want = _scipy_blur(src, q, q)
    assert np.abs(got.astype(np.float64) - want).max() <= 0.5 + 1e-6


def test_conv_gaussian_arguments(hjd):
    f = C.from_numpy(hjd.conv_gaussian(2.0))
    assert f["rx"] == f["ry"] == 6   # 2 ceil(6) + 1 = 13 taps
    f = C.from_numpy(hjd.conv_gaussian(10.0))
    assert f["rx"] == f["ry"] == 11 and sum(f["kh"]) == 4096   # capped at 23
    f = C.from_numpy(hjd.conv_gaussian(1.0, ksize=(3, 7), sigma_y=2.0, border=hjd.CONV_REPLICATE))
    assert (f["rx"], f["ry"], f["border"]) == (1, 3, C.REPLICATE) and f["kh"] != f["kv"][2:5]
    f = C.from_numpy(hjd.conv_gaussian(0.1))
    assert f["rx"] == f["ry"] == 0 and f["kh"] == [4096]   # every other tap rounds to 0 and is trimmed
    f = C.from_numpy(hjd.conv_gaussian(2.0, ksize=23))
    assert sum(f["kh"]) == 4096 and f["rx"] < 11 and f["kh"][0] + f["kh"][-1] > 0   # exp(-0.5 * 5.5^2) * 4096 rounds to 0
    for kw in ({"sigma": 0}, {"sigma": -1.0}, {"sigma": float("nan")}, {"sigma": 1.0, "ksize": 4}, {"sigma": 1.0, "ksize": 25},
               {"sigma": 1.0, "ksize": 0}, {"sigma": 1.0, "sigma_y": 0.0}):
        with pytest.raises(ValueError):
            hjd.conv_gaussian(**kw)
    u = C.from_numpy(hjd.conv_unsharp(1.0, 0.5))
    assert (u["a"], u["b"], u["border"]) == (6144, -2048, C.REFLECT) and u["kh"] == C.from_numpy(hjd.conv_gaussian(1.0))["kh"]
    with pytest.raises(ValueError):
        hjd.conv_unsharp(1.0, 300.0)
    with pytest.raises(ValueError):
        hjd.conv_filter([1, 2], [4096], 0, 4096)
    with pytest.raises(ValueError):
        hjd.conv_filter([4097], [4096], 0, 4096)


# ---- sharpness --------------------------------------------------------------------------------
FACTORS = (0, 0.1, 0.5, 1, 1.5, 1.9, 2)


def _sharp_images():
    rng = np.random.default_rng(2026)
    yy, xx = np.mgrid[0:40, 0:56]
    return {"random": rng.integers(0, 256, (3, 40, 56), dtype=np.uint8),
            "checkerboard": np.stack([np.where((yy + xx) % 2, 200, 40), np.where((yy // 2 + xx // 3) % 2, 255, 0),
                                      np.where((yy + xx) % 2, 130, 120)]).astype(np.uint8),
            "0/255": np.where(rng.random((3, 40, 56)) < 0.5, 0, 255).astype(np.uint8)}


def _pillow_sharpness(src, factor):
    from PIL import Image, ImageEnhance
    img = Image.fromarray(np.ascontiguousarray(src.transpose(1, 2, 0)), "RGB")
    return np.asarray(ImageEnhance.Sharpness(img).enhance(factor)).transpose(2, 0, 1)


def test_conv_sharpness_records(hjd):
    assert hjd.conv_sharpness(1).tobytes() == hjd.CONV_IDENTITY.tobytes() == hjd.conv_sharpness(1.0).tobytes()
    i = C.from_numpy(hjd.CONV_IDENTITY)
    assert i == C.IDENTITY and (i["rx"], i["ry"], i["a"], i["b"]) == (0, 0, 4096, 0)
    for f in FACTORS:
        if f == 1:
            continue
        r = C.from_numpy(hjd.conv_sharpness(f))
        assert (r["rx"], r["ry"], r["border"], r["kh"], r["kv"]) == (1, 1, C.KEEP, [1024] * 3, [1024] * 3)
        assert r["a"] == round(4096 * (4 + 9 * f) / 13) and r["b"] == round(65536 * (1 - f) / 13)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            hjd.conv_sharpness(bad)


def test_conv_sharpness_against_pillow(hjd):
    """|ours - Pillow| <= 2 for f in 0..2 (derived: ours is within ~0.55 of the real map, Pillow rounds the smoothed image
    and truncates the blend: <= 0.5 |1 - f| + 1).  Measured: at most 1, none at f = 0, 1, 2 (printed)."""
    worst, differing, total = 0, 0, 0
    for name, src in _sharp_images().items():
        for f in FACTORS:
            rec = C.from_numpy(hjd.conv_sharpness(f))
            ours = _host(hjd, src, rec)
            assert np.array_equal(ours, C.conv_u8(src, rec))
            d = np.abs(ours.astype(np.int64) - _pillow_sharpness(src, f).astype(np.int64))
            print(f"sharpness {f} on {name}: max |diff| {d.max()}, {100.0 * (d != 0).mean():.2f} % of the pixels differ")
            assert d.max() <= 2, (name, f)
            worst, differing, total = max(worst, int(d.max())), differing + int((d != 0).sum()), total + d.size
    print(f"sharpness overall: max |diff| {worst}, {100.0 * differing / total:.2f} % of the pixels differ")


# ---- hjd_conv_check ---------------------------------------------------------------------------
def _item(hjd, src=0x10000, dst=0x20000, w=37, h=29, pitch=37, dst_pitch=37, f=None, reserved=0, **edit):
    f = dict(f or C.record([1000, 2096, 1000], [500, 3096, 500], 0, 4096, C.REFLECT), **edit)
    it = hjd._lib.HjdConvItem(src, dst, w, h, pitch, dst_pitch)
    it.filter = _ctypes_filter(hjd, f, reserved)
    return it


def _check(hjd, items, n=None, fmt=PLANAR):
    arr = (hjd._lib.HjdConvItem * len(items))(*items)
    return hjd._lib.load().hjd_conv_check(arr, len(items) if n is None else n, fmt), hjd._lib.error_string()


def _refused(hjd, match, items, **kw):
    rc, msg = _check(hjd, items, **kw)
    assert rc == -1, (rc, msg)   # HJD_E_INVALID
    assert re.search(match, msg), msg


def test_conv_check_accepts(hjd):
    assert _check(hjd, [_item(hjd), _item(hjd, src=0x10001, dst=0x30001, w=5, h=3, pitch=7, dst_pitch=5, border=C.KEEP)])[0] == 0
    for border in BORDERS:
        assert _check(hjd, [_item(hjd, border=border)])[0] == 0
    assert _check(hjd, [_item(hjd, dst_pitch=74)], fmt=F16)[0] == 0 and _check(hjd, [_item(hjd, dst_pitch=148)], fmt=F32)[0] == 0
    assert _check(hjd, [_item(hjd, w=16384, h=16384, pitch=16384, dst_pitch=16384)])[0] == 0
    assert _check(hjd, [_item(hjd, w=1, h=1, pitch=1, dst_pitch=1, f=C.IDENTITY)])[0] == 0
    assert _check(hjd, [_item(hjd, w=2, h=2, pitch=2, dst_pitch=2)])[0] == 0            # REFLECT at r = dim - 1
    assert _check(hjd, [_item(hjd, w=1, h=1, pitch=1, dst_pitch=1, border=C.KEEP)])[0] == 0   # KEEP with 2 r >= dim
    assert _check(hjd, [_item(hjd, w=1, h=1, pitch=1, dst_pitch=1, border=C.REPLICATE)])[0] == 0
    assert _check(hjd, [_item(hjd, pitch=1 << 30, dst_pitch=1 << 30)])[0] == 0   # pitches have no upper bound
    assert _check(hjd, [_item(hjd, a=1 << 20, b=-(1 << 20))])[0] == 0
    full = [0] * 11 + [4096] + [0] * 11
    assert _check(hjd, [_item(hjd, f=C.record(full, [1], 0, 4096, C.REPLICATE))])[0] == 0   # sums 4096 and 1


def test_conv_check_refuses_null_items_and_n(hjd):
    assert hjd._lib.load().hjd_conv_check(None, 1, PLANAR) == -1 and "NULL" in hjd._lib.error_string()
    for n in (0, -1, (1 << 20) + 1):
        _refused(hjd, "n = ", [_item(hjd)], n=n)


def test_conv_check_refuses_null_pointers(hjd):
    _refused(hjd, "conv item 0: src or dst is NULL", [_item(hjd, src=0)])
    _refused(hjd, "conv item 1: src or dst is NULL", [_item(hjd), _item(hjd, dst=0)])


def test_conv_check_refuses_dimensions(hjd):
    for bad in (0, -3, 16385):
        _refused(hjd, "item 0: source size", [_item(hjd, w=bad, pitch=1 << 20, dst_pitch=1 << 20)])
        _refused(hjd, "item 1: source size", [_item(hjd), _item(hjd, h=bad)])


def test_conv_check_refuses_a_short_src_pitch(hjd):
    _refused(hjd, "src_pitch 36 is below", [_item(hjd, pitch=36)])


def test_conv_check_refuses_a_misaligned_dst(hjd):
    _refused(hjd, "dst must be a multiple", [_item(hjd, dst=0x20001, dst_pitch=74)], fmt=F16)
    _refused(hjd, "dst must be a multiple", [_item(hjd, dst=0x20002, dst_pitch=148)], fmt=F32)


def test_conv_check_refuses_a_bad_dst_pitch(hjd):
    _refused(hjd, "item 0: dst_pitch 36 must be >= 37", [_item(hjd, dst_pitch=36)])
    _refused(hjd, "dst_pitch 72 must be >= 74", [_item(hjd, dst_pitch=72)], fmt=F16)
    _refused(hjd, "dst_pitch 75 .*multiple of 2", [_item(hjd, dst_pitch=75)], fmt=F16)
    _refused(hjd, "dst_pitch 150 .*multiple of 4", [_item(hjd, dst_pitch=150)], fmt=F32)


def test_conv_check_refuses_in_place(hjd):
    _refused(hjd, "item 1: dst == src", [_item(hjd), _item(hjd, dst=0x10000)])
    _refused(hjd, "item 0: dst == src", [_item(hjd, dst=0x10000, f=C.IDENTITY)])   # the identity record too


def test_conv_check_refuses_a_radius_out_of_range(hjd):
    for rx, ry in ((12, 1), (1, 12), (-1, 0), (0, -1), (1 << 20, 0)):
        _refused(hjd, r"item 1: radius \(-?\d+, -?\d+\) is outside 0..11", [_item(hjd), _item(hjd, rx=rx, ry=ry)])


def test_conv_check_refuses_a_border_out_of_range(hjd):
    for border in (3, -1, 1 << 20):
        _refused(hjd, f"item 0: border {border} is outside 0..2", [_item(hjd, border=border)])


def test_conv_check_refuses_reflect_with_a_radius_of_the_dimension(hjd):
    f3 = C.record([1000, 1000, 96, 1000, 1000], [4096], 0, 4096, C.REFLECT)
    _refused(hjd, "item 0: HJD_CONV_REFLECT needs radius", [_item(hjd, w=2, pitch=2, dst_pitch=2, f=f3)])
    _refused(hjd, "item 1: HJD_CONV_REFLECT needs radius", [_item(hjd), _item(hjd, h=1)])
    assert _check(hjd, [_item(hjd, w=3, pitch=3, dst_pitch=3, f=f3)])[0] == 0
    assert _check(hjd, [_item(hjd, w=2, pitch=2, dst_pitch=2, f=dict(f3, border=C.REPLICATE))])[0] == 0


def test_conv_check_refuses_tap_sums(hjd):
    _refused(hjd, "item 0: the taps of kh sum to 0", [_item(hjd, kh=[0, 0, 0])])
    _refused(hjd, "item 0: the taps of kv sum to 4097", [_item(hjd, kv=[1000, 2097, 1000])])
    _refused(hjd, "item 1: the taps of kh sum to 65535", [_item(hjd), _item(hjd, kh=[0, 65535, 0])])
    _refused(hjd, "the taps of kv sum to 131070", [_item(hjd, kv=[65535, 0, 65535])])


def test_conv_check_refuses_a_tap_beyond_the_radius(hjd):
    for name in ("kh", "kv"):
        for p in (3, 23):
            it = _item(hjd)
            getattr(it.filter, name)[p] = 1
            _refused(hjd, rf"item 0: {name}\[{p}\] = 1 lies beyond the 3 taps", [it])


def test_conv_check_refuses_gains(hjd):
    for a, b in (((1 << 20) + 1, 0), (0, (1 << 20) + 1), (-(1 << 20) - 1, 0), (0, -(1 << 31))):
        _refused(hjd, "item 0: gain", [_item(hjd, a=a, b=b)])


def test_conv_check_refuses_reserved(hjd):
    _refused(hjd, "item 0: reserved must be 0", [_item(hjd, reserved=1)])
    _refused(hjd, "item 1: reserved must be 0", [_item(hjd), _item(hjd, reserved=-1)])


def test_conv_check_refuses_formats(hjd):
    for fmt in (0, 1, 2, 4, 7, -1):
        _refused(hjd, "output format", [_item(hjd)], fmt=fmt)


def test_conv_check_refuses_2_to_the_31_tiles(hjd):
    """16384 x 16384 is 256 x 512 = 2^17 tiles of 64 x 32: 2^14 such items are 2^31."""
    big = _item(hjd, w=16384, h=16384, pitch=16384, dst_pitch=16384)
    n = 1 << 14
    arr = (hjd._lib.HjdConvItem * n)(*([big] * n))
    lib = hjd._lib.load()
    assert lib.hjd_conv_check(arr, n, PLANAR) == -1 and "tiles" in hjd._lib.error_string()
    assert lib.hjd_conv_check(arr, n - 1, PLANAR) == 0


# ---- interfaces -------------------------------------------------------------------------------
def test_conv_entry_points_are_bound(hjd):
    lib = hjd._lib.load()
    for name in ("hjd_conv_check", "hjd_conv_create", "hjd_conv_set_normalize", "hjd_conv_launch", "hjd_conv_destroy",
                 "hjd_conv_apply_host", "hjd_gdec_decode_resized_aug", "hjd_gdec_decode_warped_aug"):
        assert name in hjd._lib.SIGNATURES and getattr(lib, name).argtypes == hjd._lib.SIGNATURES[name][1]
        for header in ("hjd.h", "hjd_host.h"):
            if re.search(rf"\b{name}\(", open(os.path.join(REPO, "include", header)).read()):
                break
        else:
            raise AssertionError(f"{name} is in no header")
    header = open(os.path.join(REPO, "include", "hjd.h")).read()
    assert "enum { HJD_CONV_KEEP = 0, HJD_CONV_REFLECT = 1, HJD_CONV_REPLICATE = 2 };" in header
    assert re.search(r"#define HJD_CONV_MAX_RADIUS\s+11\b", header) and re.search(r"#define HJD_CONV_MAX_GAIN\s+\(1 << 20\)", header)
    for struct, want in (("hjd_conv_filter", ["int32_t rx, ry", "int32_t border", "int32_t a, b", "int32_t reserved",
                                              "uint16_t kh[24], kv[24]"]),
                         ("hjd_conv_item", ["const void* src", "void* dst", "int32_t w, h, src_pitch, dst_pitch",
                                            "hjd_conv_filter filter"])):
        m = re.search(rf"typedef struct {struct} \{{([^}}]*)\}} {struct};", header)
        assert m, struct
        fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert [d.strip() for d in fields.split(";") if d.strip()] == want
    F, I = hjd._lib.HjdConvFilter, hjd._lib.HjdConvItem
    assert 6 * 4 + 2 * 48 == 120 == ctypes.sizeof(F) and 2 * 8 + 4 * 4 + 120 == 152 == ctypes.sizeof(I)
    assert [getattr(F, f).offset for f in ("rx", "ry", "border", "a", "b", "reserved", "kh", "kv")] == [0, 4, 8, 12, 16, 20, 24, 72]
    assert [getattr(I, f).offset for f in ("src", "dst", "w", "h", "src_pitch", "dst_pitch", "filter")] == \
        [0, 8, 16, 20, 24, 28, 32]
    from ocljpegdecoder_amd.backend import _CONV_FILTER_DTYPE, _CONV_ITEM_DTYPE
    assert [_CONV_FILTER_DTYPE.fields[f][1] for f in ("rx", "ry", "border", "a", "b", "reserved", "kh", "kv")] == \
        [0, 4, 8, 12, 16, 20, 24, 72] and _CONV_ITEM_DTYPE.fields["rx"][1] == 32 and _CONV_ITEM_DTYPE.fields["kv"][1] == 104
    assert "#define HJD_ABI_VERSION 1" in header and lib.hjd_abi_version() == 1
    assert lib.hjd_conv_launch(None, None) == -1
    one = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.hjd_conv_set_normalize(None, one, one) == -1
    assert lib.hjd_conv_destroy(None) == 0
    assert lib.hjd_conv_create(None, None, 1, PLANAR, None) == -1
    assert lib.hjd_gdec_decode_resized_aug(None, None, None, 1, None, None, None, None, None, None, None, 8, 8, 8, 0, None) == -1
    assert lib.hjd_gdec_decode_warped_aug(None, None, None, 1, None, None, None, None, None, None, None, None, 8, 8, 8,
                                          None) == -1


def test_conv_python_interface(hjd):
    for name in ("Conv", "CONV_KEEP", "CONV_REFLECT", "CONV_REPLICATE", "CONV_IDENTITY", "conv_filter", "conv_sharpness",
                 "conv_gaussian", "conv_unsharp"):
        assert name in hjd.__all__ and hasattr(hjd, name)
    assert (hjd.CONV_KEEP, hjd.CONV_REFLECT, hjd.CONV_REPLICATE) == (C.KEEP, C.REFLECT, C.REPLICATE)
    assert list(inspect.signature(hjd.Conv.__init__).parameters) == ["self", "ctx", "srcs", "outs", "filters", "normalize"]
    for method in ("launch", "set_normalize", "close"):
        assert callable(getattr(hjd.Conv, method))
    p = inspect.signature(hjd.conv_gaussian).parameters
    assert list(p) == ["sigma", "ksize", "sigma_y", "border"] and [p[k].default for k in list(p)[1:]] == [None, None, hjd.CONV_REFLECT]
    assert list(inspect.signature(hjd.conv_sharpness).parameters) == ["factor"]
    assert list(inspect.signature(hjd.conv_unsharp).parameters)[:2] == ["sigma", "amount"]
    assert not hjd.CONV_IDENTITY.flags.writeable
    G = hjd.GpuDecoder
    assert list(inspect.signature(G.decode_rgb_resized_aug).parameters) == \
        list(inspect.signature(G.decode_rgb_resized_color).parameters) + ["convs", "curves", "modes"]
    assert list(inspect.signature(G.decode_rgb_warped_aug).parameters) == \
        list(inspect.signature(G.decode_rgb_warped_color).parameters) + ["convs", "curves", "modes"]
    for fn, ref in ((G.decode_rgb_resized_aug, G.decode_rgb_resized), (G.decode_rgb_warped_aug, G.decode_rgb_warped)):
        a, b = inspect.signature(fn).parameters, inspect.signature(ref).parameters
        assert all(a[k].default == b[k].default for k in b if k != "self")
    from ocljpegdecoder_amd.backend import _conv_filters
    recs = _conv_filters(None, 3)
    assert recs.shape == (3,) and all(r.tobytes() == hjd.CONV_IDENTITY.tobytes() for r in recs)
    recs = _conv_filters([hjd.conv_sharpness(0.5), hjd.CONV_IDENTITY], 2)
    assert recs[0].tobytes() == hjd.conv_sharpness(0.5).tobytes() and recs[1].tobytes() == hjd.CONV_IDENTITY.tobytes()
    assert _conv_filters(hjd.conv_gaussian(1.0), 2)[1].tobytes() == hjd.conv_gaussian(1.0).tobytes()
    for bad in ([hjd.CONV_IDENTITY], [hjd.CONV_IDENTITY, np.zeros(3)]):
        with pytest.raises(ValueError):
            _conv_filters(bad, 2)
