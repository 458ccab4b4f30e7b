"""EXIF orientation without a GPU: the numpy model (orient_model.py) against
Pillow's ImageOps.exif_transpose, hjd_jpeg_orientation on well-formed and
broken EXIF blocks, hjd_orient_roi against slicing, hjd_orient_check's
refusals, and the reader under AddressSanitizer + UBSan as a stand-alone
program (tools/fuzz/orient_fuzz.cpp)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import orient_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIENTATIONS = range(1, 9)
ORIENT = (0x0112, 3, 1)   # tag, SHORT, count 1


# ---- the model ------------------------------------------------------------------
@pytest.mark.parametrize("o", ORIENTATIONS)
def test_model_vs_pillow(o):
    from PIL import Image, ImageOps
    S = np.random.default_rng(o).integers(0, 256, (5, 7, 3), dtype=np.uint8)   # 5 rows x 7 columns
    im = Image.fromarray(S)
    exif = Image.Exif()
    exif[0x0112] = o
    im.info["exif"] = exif.tobytes()
    im.getexif()[0x0112] = o
    ref = np.asarray(ImageOps.exif_transpose(im))
    got = M.orient(S.transpose(2, 0, 1), o)
    assert got.shape[1:] == M.oriented_size(7, 5, o)[::-1]
    np.testing.assert_array_equal(got.transpose(1, 2, 0), ref)


def test_model_is_a_permutation_and_tells_the_eight_apart():
    S = np.arange(5 * 7).reshape(5, 7)
    seen = [M.orient(S, o) for o in ORIENTATIONS]
    for a in seen:
        assert sorted(a.ravel()) == list(range(35))
    for i in range(8):
        for j in range(i):
            assert seen[i].shape != seen[j].shape or not np.array_equal(seen[i], seen[j])


# ---- reading the tag --------------------------------------------------------------
def _plain():
    return M.pil_jpeg(16, 8, 0, seed=1)


@pytest.mark.parametrize("o", ORIENTATIONS)
def test_pillow_written_tag(hjd, o):
    data = M.pil_jpeg(16, 8, 0, seed=o, orientation=o)
    assert b"Exif\0\0MM" in data           # Pillow writes big-endian
    assert hjd.exif_orientation(data) == o
    assert hjd.parse(data).width == 16     # and the file still decodes as ever


@pytest.mark.parametrize("order", [b"II", b"MM"])
@pytest.mark.parametrize("o", ORIENTATIONS)
def test_hand_built_app1(hjd, order, o):
    data = M.with_segments(_plain(), M.exif_app1(M.tiff_block(order, [ORIENT + (o,)])))
    assert hjd.exif_orientation(data) == o


def test_which_app1_and_which_entry(hjd):
    plain = _plain()
    assert b"JFIF" in plain and hjd.exif_orientation(plain) == 1       # no APP1 at all
    xmp = M.app1(b"http://ns.adobe.com/xap/1.0/\0<x/>")
    exif6 = M.exif_app1(M.tiff_block(b"II", [ORIENT + (6,)]))
    exif3 = M.exif_app1(M.tiff_block(b"MM", [ORIENT + (3,)]))
    assert hjd.exif_orientation(M.with_segments(plain, xmp)) == 1      # an APP1 that is not Exif
    assert hjd.exif_orientation(M.with_segments(plain, xmp, exif6)) == 6
    assert hjd.exif_orientation(M.with_segments(plain, exif3, exif6)) == 3   # the first Exif APP1
    # the tag after other entries, and IFD0 not right behind the header
    others = [(0x010F, 2, 4, 0x41424300), (0x011A, 5, 1, 99), (0x0128, 3, 1, 2)]
    for order in (b"II", b"MM"):
        tiff = M.tiff_block(order, others + [ORIENT + (8,)], ifd_offset=14)
        assert hjd.exif_orientation(M.with_segments(plain, M.exif_app1(tiff))) == 8
    # numpy arrays and bytearrays are taken as bytes are
    assert hjd.exif_orientation(np.frombuffer(M.with_segments(plain, exif6), np.uint8)) == 6


def test_broken_exif_is_orientation_1(hjd):
    plain = _plain()

    def tag(tiff):
        return hjd.exif_orientation(M.with_segments(plain, M.exif_app1(tiff)))

    for order in (b"II", b"MM"):
        assert tag(M.tiff_block(order, [ORIENT + (5,)])) == 5                       # the well-formed one
        for v in (0, 9, 65535):
            assert tag(M.tiff_block(order, [ORIENT + (v,)])) == 1                   # value outside 1..8
        assert tag(M.tiff_block(order, [(0x0112, 4, 1, 5)])) == 1                   # type LONG
        assert tag(M.tiff_block(order, [(0x0112, 3, 2, 5)])) == 1                   # count 2
        assert tag(M.tiff_block(order, [ORIENT + (5,)], magic=43)) == 1
        good = M.tiff_block(order, [ORIENT + (5,)])
        assert tag(b"XX" + good[2:]) == 1                                           # byte order
        off = (1000).to_bytes(4, "little" if order == b"II" else "big")
        assert tag(good[:4] + off + good[8:]) == 1                                  # IFD offset past the segment
        assert tag(M.tiff_block(order, [ORIENT + (5,)], count=3)) == 1              # entries run past the segment
        assert tag(M.tiff_block(order, [ORIENT + (5,)], count=65535)) == 1
        # the segment cut at every byte of the TIFF block (its length field says so):
        # 1 while the header, the count or the entry is cut, the value once the entry is whole
        assert len(good) == 8 + 2 + 12 + 4
        for k in range(len(good) + 1):
            assert tag(good[:k]) == (5 if k >= 22 else 1), k
    assert hjd.exif_orientation(M.with_segments(plain, M.app1(b"Exif\0"))) == 1     # not even the identifier
    assert hjd.exif_orientation(M.with_segments(plain, M.app1(b""))) == 1


def test_not_a_jpeg_is_the_parsers_error(hjd):
    from ocljpegdecoder_amd._lib import HjdError
    plain = _plain()
    with pytest.raises(HjdError, match="SOI missing"):
        hjd.exif_orientation(b"\x89PNG" + plain)
    bad_len = M.with_segments(plain, M.exif_app1(M.tiff_block(b"II", [ORIENT + (6,)])))
    bad_len = bad_len[:4] + b"\xff\xff" + bad_len[6:]          # the APP1 claims more bytes than the file has
    with pytest.raises(HjdError, match="bad segment length"):
        hjd.exif_orientation(bad_len)
    lib = hjd._lib.load()
    assert lib.hjd_jpeg_orientation(None, 0, None) == -1


# ---- geometry -----------------------------------------------------------------------
RECTS = [(0, 0, 1, 1), (2, 1, 3, 2), (0, 3, 4, 1), (4, 0, 1, 5)]   # on a 5-wide, 5-high corner every D has


@pytest.mark.parametrize("o", ORIENTATIONS)
def test_oriented_roi_vs_slicing(hjd, o):
    W, H = 9, 6
    S = np.random.default_rng(10 + o).integers(0, 256, (3, H, W), dtype=np.uint8)
    D = M.orient(S, o)
    dw, dh = hjd.oriented_size(W, H, o)
    assert (dw, dh) == M.oriented_size(W, H, o) and D.shape == (3, dh, dw)
    for roi in RECTS + [(0, 0, dw, dh), (dw - 1, dh - 1, 1, 1), (dw - 2, 0, 2, dh), (0, dh - 1, dw, 1)]:
        x, y, w, h = roi
        sx, sy, sw, sh = hjd.oriented_roi(W, H, o, roi)
        assert (sx, sy, sw, sh) == M.oriented_roi(W, H, o, roi)
        np.testing.assert_array_equal(D[:, y:y + h, x:x + w], M.orient(S[:, sy:sy + sh, sx:sx + sw], o))
    assert hjd.oriented_roi(W, H, 6, (1, 2, 3, 4)) == (2, H - 1 - 3, 4, 3)   # (x, y, w, h) -> (y, H - x - w, h, w)


def test_oriented_roi_refusals(hjd):
    from ocljpegdecoder_amd._lib import HjdError
    W, H = 9, 6
    for o in ORIENTATIONS:
        dw, dh = hjd.oriented_size(W, H, o)
        for roi in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0), (dw, 0, 1, 1), (0, dh, 1, 1),
                    (dw - 1, 0, 2, 1), (0, dh - 1, 1, 2), (0, 0, dw + 1, 1), (1, 0, 2 ** 31 - 1, 1)):
            with pytest.raises(HjdError, match="outside the") as e:
                hjd.oriented_roi(W, H, o, roi)
            assert e.value.code == -1
    with pytest.raises(HjdError, match="orientation"):
        hjd.oriented_roi(W, H, 9, (0, 0, 1, 1))
    with pytest.raises(HjdError, match="stored size"):
        hjd.oriented_roi(0, H, 1, (0, 0, 1, 1))
    with pytest.raises(ValueError):
        hjd.oriented_size(W, H, 0)
    lib = hjd._lib.load()
    assert lib.hjd_orient_roi(W, H, 1, None, None) == -1


# ---- hjd_orient_check ----------------------------------------------------------------
PLANAR, F16, F32 = 3, 5, 6


def _check(hjd, items, n, fmt):
    lib = hjd._lib.load()
    arr = (hjd._lib.HjdOrientItem * len(items))(*[hjd._lib.HjdOrientItem(*it) for it in items])
    rc = lib.hjd_orient_check(arr, n, fmt)
    return rc, hjd._lib.error_string()


def _refused(hjd, match, items, n, fmt):
    rc, msg = _check(hjd, items, n, fmt)
    assert rc == -1, (rc, msg)   # HJD_E_INVALID
    assert re.search(match, msg), msg


def test_orient_check(hjd):
    lib = hjd._lib.load()
    # src, dst, w, h, src_pitch, orientation, dst_pitch, reserved
    ok = (0x10000, 0x20000, 37, 29, 37, 1, 37, 0)
    turned = (0x10001, 0x30000, 5, 3, 7, 6, 3, 0)          # D is 3 wide
    assert _check(hjd, [ok, turned], 2, PLANAR)[0] == 0
    assert _check(hjd, [(0x10000, 0x20000, 37, 29, 37, 1, 74, 0), (0x10000, 0x30000, 5, 3, 7, 8, 6, 0)], 2,
                  F16)[0] == 0                                                         # sources may overlap
    assert _check(hjd, [(0x10000, 0x30000, 5, 3, 7, 5, 12, 0)], 1, F32)[0] == 0
    assert _check(hjd, [(0x1000, 0x40000000, 16384, 16384, 16384, 7, 16384, 0)], 1, PLANAR)[0] == 0
    assert _check(hjd, [(0x1000, 0x2000, 1, 1, 1, 3, 1, 0)], 1, PLANAR)[0] == 0
    assert lib.hjd_orient_check(None, 1, PLANAR) == -1 and "NULL" in hjd._lib.error_string()
    for n in (0, -1, (1 << 20) + 1):
        _refused(hjd, "n = ", [ok], n, PLANAR)
    for bad in (0, -3, 16385):
        _refused(hjd, "item 0: source size", [(0x10000, 0x20000, bad, 29, 1 << 20, 1, 1 << 20, 0)], 1, PLANAR)
        _refused(hjd, "item 1: source size", [ok, (0x10000, 0x30000, 37, bad, 37, 1, 37, 0)], 2, PLANAR)
    _refused(hjd, "item 0: src or dst is NULL", [(0, 0x20000, 37, 29, 37, 1, 37, 0)], 1, PLANAR)
    _refused(hjd, "item 1: src or dst is NULL", [ok, (0x10000, 0, 37, 29, 37, 1, 37, 0)], 2, PLANAR)
    _refused(hjd, "src_pitch", [(0x10000, 0x20000, 37, 29, 36, 1, 37, 0)], 1, PLANAR)
    for o in (0, 9, -1, 1 << 20):
        _refused(hjd, "orientation", [(0x10000, 0x20000, 37, 29, 37, o, 37, 0)], 1, PLANAR)
    # dst_pitch against the ORIENTED width: 37 for 1..4, 29 for 5..8
    _refused(hjd, "dst_pitch", [(0x10000, 0x20000, 37, 29, 37, 2, 36, 0)], 1, PLANAR)
    assert _check(hjd, [(0x10000, 0x20000, 37, 29, 37, 6, 29, 0)], 1, PLANAR)[0] == 0
    _refused(hjd, "dst_pitch", [(0x10000, 0x20000, 37, 29, 37, 6, 28, 0)], 1, PLANAR)
    _refused(hjd, "dst_pitch", [(0x10000, 0x20000, 37, 29, 37, 6, 57, 0)], 1, F16)     # < 2 * 29
    _refused(hjd, "dst_pitch", [(0x10000, 0x20000, 37, 29, 37, 6, 59, 0)], 1, F16)     # not a multiple of 2
    _refused(hjd, "dst_pitch", [(0x10000, 0x20000, 37, 29, 37, 6, 118, 0)], 1, F32)    # not a multiple of 4
    _refused(hjd, "dst must be a multiple", [(0x10000, 0x20001, 37, 29, 37, 1, 74, 0)], 1, F16)
    _refused(hjd, "dst must be a multiple", [(0x10000, 0x20002, 37, 29, 37, 1, 148, 0)], 1, F32)
    assert _check(hjd, [(0x10000, 0x20001, 37, 29, 37, 1, 37, 0)], 1, PLANAR)[0] == 0   # bytes: any dst
    _refused(hjd, "reserved", [(0x10000, 0x20000, 37, 29, 37, 1, 37, 5)], 1, PLANAR)
    for fmt in (0, 1, 2, 4, 7, -1):
        _refused(hjd, "output format", [ok], 1, fmt)
    # overlap: an output with its own source, with another item's source, with another output
    size = 3 * 29 * 37
    _refused(hjd, "overlaps", [(0x10000, 0x10000 + size - 1, 37, 29, 37, 1, 37, 0)], 1, PLANAR)
    assert _check(hjd, [(0x10000, 0x10000 + size, 37, 29, 37, 1, 37, 0)], 1, PLANAR)[0] == 0   # back to back
    _refused(hjd, "overlaps", [ok, (0x40000, 0x10010, 5, 3, 5, 1, 5, 0)], 2, PLANAR)
    _refused(hjd, "item 1: its output overlaps item 0", [ok, (0x40000, 0x20000 + size - 1, 5, 3, 5, 1, 5, 0)], 2, PLANAR)
    _refused(hjd, "overlaps", [(0x10000, 0x20000, 8, 8, 8, 1, 16, 0), (0x20000 + 3 * 8 * 16 - 1, 0x50000, 8, 8, 8, 1, 16, 0)],
             2, F16)                                                                  # the float output's extent
    assert _check(hjd, [(0x10000, 0x20000, 8, 8, 8, 1, 16, 0), (0x20000 + 3 * 8 * 16, 0x50000, 8, 8, 8, 1, 16, 0)], 2,
                  F16)[0] == 0


def test_orient_entry_points_are_bound(hjd):
    """Declared in the headers, exported, bound in _lib.py; NULL objects are refused without a device."""
    lib = hjd._lib.load()
    for name in ("hjd_orient_check", "hjd_orient_create", "hjd_orient_set_normalize", "hjd_orient_launch",
                 "hjd_orient_destroy", "hjd_orient_roi", "hjd_jpeg_orientation", "hjd_gdec_decode_oriented",
                 "hjd_gdec_decode_resized_oriented"):
        assert name in hjd._lib.SIGNATURES and getattr(lib, name).argtypes == hjd._lib.SIGNATURES[name][1]
        for header in ("hjd.h", "hjd_host.h"):
            if re.search(rf"\b{name}\(", open(os.path.join(REPO, "include", header)).read()):
                break
        else:
            raise AssertionError(f"{name} is in no header")
    assert lib.hjd_orient_launch(None, None) == -1
    one = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.hjd_orient_set_normalize(None, one, one) == -1
    assert lib.hjd_orient_destroy(None) == 0
    assert lib.hjd_gdec_decode_oriented(None, None, None, 1, None, None, None, None, None) == -1
    assert lib.hjd_gdec_decode_resized_oriented(None, None, None, 1, None, None, None, None, 8, 8, 8, 0, None) == -1
    assert callable(hjd.Orient) and callable(hjd.exif_orientation)
    # Python: the two arguments, off by default where a call existed before
    import inspect
    for fn in (hjd.GpuDecoder.decode, hjd.GpuDecoder.decode_resized, hjd.GpuDecoder.decode_rgb_resized):
        p = inspect.signature(fn).parameters
        assert p["apply_exif_orientation"].default is False and p["orientations"].default is None, fn
    p = inspect.signature(hjd.GpuDecoder.decode_rgb_oriented).parameters
    assert p["apply_exif_orientation"].default is True and p["orientations"].default is None
    assert list(p)[:-2] == list(inspect.signature(hjd.GpuDecoder.decode_rgb).parameters)


# ---- the reader under the sanitizers ---------------------------------------------------
def test_reader_under_asan_ubsan(tmp_path):
    """A stand-alone program over the host source, run as a child process."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone sanitizer program"
    exe = tmp_path / "orient_fuzz"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", f"-I{REPO}/include", f"-I{REPO}/ocljpegdecoder_amd/csrc",
                    f"{REPO}/ocljpegdecoder_amd/csrc/jpeg_host.cpp", f"{REPO}/tools/fuzz/orient_fuzz.cpp", "-o", str(exe),
                    "-lpthread"], check=True)
    plain = M.pil_jpeg(16, 8, 0, seed=1)
    files = {"pil6.jpg": M.pil_jpeg(16, 8, 0, seed=2, orientation=6),
             "ii.jpg": M.with_segments(plain, M.exif_app1(M.tiff_block(b"II", [ORIENT + (3,)]))),
             "xmp_then_exif.jpg": M.with_segments(plain, M.app1(b"http://ns.adobe.com/xap/1.0/\0<x/>"),
                                                  M.exif_app1(M.tiff_block(b"MM", [ORIENT + (8,)]))),
             "late_tag.jpg": M.with_segments(plain, M.exif_app1(M.tiff_block(
                 b"II", [(0x010F, 2, 4, 0x41424300), (0x0128, 3, 1, 2), ORIENT + (5,)], ifd_offset=14))),
             "jfif.jpg": plain}
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    r = subprocess.run([str(exe), "3000"] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"hjd_jpeg_orientation: \d+ calls", r.stdout)
