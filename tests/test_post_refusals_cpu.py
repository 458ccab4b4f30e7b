"""The refusals of hjd_resize_check_filter, hjd_orient_check and hjd_warp_check,
whole texts: the ones the three share (n, the format, NULL src / dst, dst's
alignment, the source's size, src_pitch, and for resize and warp out_pitch) and
each kind's own.  Host-only: no GPU."""
import ctypes

import pytest

PLANAR, F16, F32 = 3, 5, 6
SRC, DST = 0x10000, 0x20000
M = (1 << 16, 0, 0, 0, 1 << 16, 0)
NOT_PLANAR = "output format 1 is not HJD_OUT_RGB_PLANAR, HJD_OUT_RGB_PLANAR_F16 or _F32"


def _resize_item(hjd, src=SRC, dst=DST, w=37, h=29, pitch=37, flags=0):
    return hjd._lib.HjdResizeItem(src, dst, w, h, pitch, flags)


def _orient_item(hjd, src=SRC, dst=DST, w=37, h=29, pitch=37, orientation=1, dst_pitch=37, reserved=0):
    return hjd._lib.HjdOrientItem(src, dst, w, h, pitch, orientation, dst_pitch, reserved)


def _warp_item(hjd, src=SRC, dst=DST, w=37, h=29, pitch=37, flags=0, fill=0, reserved=0):
    return hjd._lib.HjdWarpItem(src, dst, w, h, pitch, flags, (ctypes.c_int32 * 6)(*M), fill, reserved)


def _resize(hjd, items, n=None, wo=24, ho=16, pitch=24, fmt=PLANAR, filt=0):
    arr = (hjd._lib.HjdResizeItem * len(items))(*items)
    rc = hjd._lib.load().hjd_resize_check_filter(arr, len(items) if n is None else n, wo, ho, pitch, fmt, filt)
    return rc, hjd._lib.error_string()


def _orient(hjd, items, n=None, fmt=PLANAR):
    arr = (hjd._lib.HjdOrientItem * len(items))(*items)
    rc = hjd._lib.load().hjd_orient_check(arr, len(items) if n is None else n, fmt)
    return rc, hjd._lib.error_string()


def _warp(hjd, items, n=None, wo=24, ho=16, pitch=24, fmt=PLANAR):
    arr = (hjd._lib.HjdWarpItem * len(items))(*items)
    rc = hjd._lib.load().hjd_warp_check(arr, len(items) if n is None else n, wo, ho, pitch, fmt)
    return rc, hjd._lib.error_string()


# kind -> (the check, an item of it, the noun of its table's refusals)
KINDS = {"resize": (_resize, _resize_item, "resize"), "orient": (_orient, _orient_item, "orient"),
         "warp": (_warp, _warp_item, "resize")}   # (the warp's output side is the resize's)


@pytest.mark.parametrize("kind", KINDS)
def test_common_refusals(hjd, kind):
    check, item, table = KINDS[kind]
    ok = item(hjd)
    assert check(hjd, [ok])[0] == 0
    # an F16 table: its own pitches, so that only dst's alignment is wrong
    f16 = dict(fmt=F16) if kind == "orient" else dict(fmt=F16, pitch=48)
    f16_item = dict(dst_pitch=74) if kind == "orient" else {}
    cases = [
        ((-1, f"{table}: n = 0 is outside 1..1048576"), [ok], dict(n=0)),
        ((-1, f"{table}: {NOT_PLANAR}"), [ok], dict(fmt=1)),
        ((-1, f"{kind} item 0: src or dst is NULL"), [item(hjd, src=0)], {}),
        ((-1, f"{kind} item 1: src or dst is NULL"), [ok, item(hjd, dst=0)], {}),
        ((-1, f"{kind} item 0: dst must be a multiple of the element size (2 bytes)"),
         [item(hjd, dst=DST + 1, **f16_item)], f16),
        ((-1, f"{kind} item 0: source size 0 x 29 is outside 1..16384"), [item(hjd, w=0)], {}),
        ((-1, f"{kind} item 1: source size 16385 x 29 is outside 1..16384"), [ok, item(hjd, w=16385, pitch=16385)], {}),
        ((-1, f"{kind} item 0: src_pitch 36 is below src_w 37"), [item(hjd, pitch=36)], {}),
    ]
    if kind != "orient":
        cases += [
            ((-1, "resize: out_pitch 23 must be >= 24 (1 bytes x out_w) and a multiple of 1"), [ok], dict(pitch=23)),
            ((-1, "resize: out_pitch 46 must be >= 48 (2 bytes x out_w) and a multiple of 2"), [ok],
             dict(pitch=46, fmt=F16)),
            ((-1, "resize: out_pitch 92 must be >= 96 (4 bytes x out_w) and a multiple of 4"), [ok],
             dict(pitch=92, fmt=F32)),
        ]
    for want, items, kw in cases:
        assert check(hjd, items, **kw) == want
    assert check(hjd, [item(hjd, dst=DST + 1, **f16_item)], **f16)[0] == -1
    assert check(hjd, [item(hjd, dst=DST + 2, **f16_item)], **f16)[0] == 0


def test_resize_refusals(hjd):
    lib = hjd._lib.load()
    ok = _resize_item(hjd)
    assert lib.hjd_resize_check_filter(None, 1, 24, 16, 24, PLANAR, 0) == -1
    assert hjd._lib.error_string() == "resize: items is NULL"
    assert _resize(hjd, [ok], filt=2) == \
        (-1, "resize: filter 2 is neither HJD_RESIZE_BILINEAR (0) nor HJD_RESIZE_TRIANGLE_AA (1)")
    assert _resize(hjd, [ok], wo=0, pitch=1 << 20) == (-1, "resize: output size 0 x 16 is outside 1..16384")
    assert _resize(hjd, [ok], ho=16385) == (-1, "resize: output size 24 x 16385 is outside 1..16384")
    assert _resize(hjd, [_resize_item(hjd, flags=6)]) == \
        (-1, "resize item 0: unknown flag bits 0x6 (bit 0: horizontal flip)")
    assert _resize(hjd, [ok, _resize_item(hjd, flags=3)]) == \
        (-1, "resize item 1: unknown flag bits 0x2 (bit 0: horizontal flip)")
    wide = _resize_item(hjd, w=8192, h=29, pitch=8192)
    tall = _resize_item(hjd, w=37, h=8192)
    assert _resize(hjd, [wide], filt=0)[0] == 0 and _resize(hjd, [tall], filt=0)[0] == 0
    assert _resize(hjd, [wide], filt=1) == \
        (-1, "resize item 0: src_w 8192 -> out_w 24: the antialiased filter takes src_w^2 <= 2^21 * out_w")
    assert _resize(hjd, [ok, tall], filt=1) == \
        (-1, "resize item 1: src_h 8192 -> out_h 16: the antialiased filter takes src_h^2 <= 2^21 * out_h")


def test_orient_refusals(hjd):
    lib = hjd._lib.load()
    ok = _orient_item(hjd)
    assert lib.hjd_orient_check(None, 1, PLANAR) == -1
    assert hjd._lib.error_string() == "orient: items is NULL"
    assert _orient(hjd, [_orient_item(hjd, orientation=0)]) == (-1, "orient item 0: orientation 0 is outside 1..8")
    assert _orient(hjd, [ok, _orient_item(hjd, dst=0x40000, orientation=9)]) == \
        (-1, "orient item 1: orientation 9 is outside 1..8")
    assert _orient(hjd, [_orient_item(hjd, dst_pitch=36)]) == \
        (-1, "orient item 0: dst_pitch 36 must be >= 37 (1 bytes x the oriented width 37) and a multiple of 1")
    assert _orient(hjd, [_orient_item(hjd, orientation=6, dst_pitch=57)], fmt=F16) == \
        (-1, "orient item 0: dst_pitch 57 must be >= 58 (2 bytes x the oriented width 29) and a multiple of 2")
    assert _orient(hjd, [_orient_item(hjd, orientation=6, dst_pitch=118)], fmt=F32) == \
        (-1, "orient item 0: dst_pitch 118 must be >= 116 (4 bytes x the oriented width 29) and a multiple of 4")
    assert _orient(hjd, [_orient_item(hjd, reserved=1)]) == (-1, "orient item 0: reserved must be 0")
    # an output may overlap nothing, a source only other sources
    assert _orient(hjd, [ok, _orient_item(hjd, dst=0x40000)])[0] == 0   # (one source, read twice)
    assert _orient(hjd, [ok, _orient_item(hjd, src=0x30000, dst=DST + 100)]) == \
        (-1, "orient item 1: its output overlaps item 0's source or output")
    assert _orient(hjd, [ok, _orient_item(hjd, src=DST + 37, dst=0x40000)]) == \
        (-1, "orient item 1: its source overlaps item 0's output")


def test_warp_refusals(hjd):
    lib = hjd._lib.load()
    ok = _warp_item(hjd)
    assert lib.hjd_warp_check(None, 1, 24, 16, 24, PLANAR) == -1
    assert hjd._lib.error_string() == "warp: items is NULL"
    assert _warp(hjd, [ok], wo=16385, pitch=1 << 20) == (-1, "resize: output size 16385 x 16 is outside 1..16384")
    assert _warp(hjd, [_warp_item(hjd, flags=6)]) == \
        (-1, "warp item 0: unknown flag bits 0x6 (bit 0: HJD_WARP_REPLICATE)")
    assert _warp(hjd, [ok, _warp_item(hjd, fill=0x1000000)]) == \
        (-1, "warp item 1: fill 0x1000000 is above 0xFFFFFF (0x00RRGGBB)")
    assert _warp(hjd, [_warp_item(hjd, reserved=-1)]) == (-1, "warp item 0: reserved must be 0")
    # the order of an item's refusals: the shared ones, the flags, the fill, reserved
    assert _warp(hjd, [_warp_item(hjd, pitch=36, flags=2, fill=1 << 24, reserved=1)])[1] == \
        "warp item 0: src_pitch 36 is below src_w 37"
    assert _warp(hjd, [_warp_item(hjd, flags=2, fill=1 << 24, reserved=1)])[1] == \
        "warp item 0: unknown flag bits 0x2 (bit 0: HJD_WARP_REPLICATE)"
    assert _warp(hjd, [_warp_item(hjd, fill=1 << 24, reserved=1)])[1] == \
        "warp item 0: fill 0x1000000 is above 0xFFFFFF (0x00RRGGBB)"
