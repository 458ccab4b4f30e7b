"""Region-of-interest decode, host side: hjd_roi_geometry against a restatement
of the task-set formula, the refusals, the C ABI's
declarations and the Python names.  No GPU."""
import ctypes
import inspect
import os
import re

import pytest

import oracle_py as O

W, H = 769, 72
SAMPLINGS = [0, 1, 3, 4, 5, 6]   # 4:4:4, 4:2:0, 4:2:2, gray, 4:1:1, 4:4:0
SCALED = [0, 1, 4]               # the samplings scaled decode serves
TASK_BLOCKS = 48


def formula(w, h, s, scale, roi):
    """(tasks, blocks) of a ROI: MCU rows myf..myl times the strips covering
    MCU columns mxf..mxl, anchored at mxf; a strip's blocks are clipped at the
    frame's MCU-row end."""
    x, y, rw, rh = roi
    pw, ph, bpm, _ = O.GEOM[s]
    mcus = TASK_BLOCKS // bpm
    mcu_w = -(-w // pw)
    mw, mh = pw // scale, ph // scale          # MCU size on the output grid
    mxf, mxl = x // mw, (x + rw - 1) // mw
    myf, myl = y // mh, (y + rh - 1) // mh
    strips = -(-(mxl - mxf + 1) // mcus)
    rows = myl - myf + 1
    blocks = rows * sum(min(mcus, mcu_w - mxf - k * mcus) * bpm for k in range(strips))
    return rows * strips, blocks


def rect_sweep(gw, gh):
    """Rectangles on a gw x gh grid: corners, single pixels, the whole grid and
    a lattice of origins and sizes around strip and MCU boundaries."""
    xs = sorted({0, 1, 7, 8, 15, 16, 95, 96, 97, 127, 128, 129, 383, 384, 385, gw // 2, gw - 2, gw - 1} & set(range(gw)))
    ys = sorted({0, 1, 7, 8, 9, 15, 16, 17, gh // 2, gh - 1} & set(range(gh)))
    ws = [1, 2, 4, 33, 96, 128, 129, 384, 500, gw]
    hs = [1, 2, 8, 9, 16, 17, gh]
    for x in xs:
        for y in ys[::3]:
            for rw in ws:
                for rh in hs[::2]:
                    if x + rw <= gw and y + rh <= gh:
                        yield (x, y, rw, rh)
    for y in ys:
        for rh in hs:
            if y + rh <= gh:
                yield (gw // 3, y, min(5, gw - gw // 3), rh)


@pytest.mark.parametrize("s,scale", [(s, 1) for s in SAMPLINGS] + [(s, k) for k in (2, 4, 8) for s in SCALED])
def test_roi_geometry_equals_the_formula(hjd, s, scale):
    gw, gh = hjd.scaled_size(W, H, scale)
    n = 0
    for roi in rect_sweep(gw, gh):
        assert hjd.roi_geometry(W, H, s, scale, roi) == formula(W, H, s, scale, roi), (s, scale, roi)
        n += 1
    assert n > 100
    # the whole grid is the whole frame's task set and blocks
    pw, ph, bpm, _ = O.GEOM[s]
    mcus = TASK_BLOCKS // bpm
    tasks, blocks = hjd.roi_geometry(W, H, s, scale, (0, 0, gw, gh))
    assert tasks == -(-(-(-W // pw)) // mcus) * -(-H // ph)
    assert blocks == O.frame_blocks(W, H, s)


def test_blocks_are_clipped_at_the_mcu_row_end(hjd):
    # 4:2:0, 769 px: 49 MCUs per row; a strip anchored at MCU 45 has 4 MCUs left of its 8
    assert hjd.roi_geometry(W, H, 1, 1, (45 * 16, 0, 1, 1)) == (1, 4 * 6)
    assert hjd.roi_geometry(W, H, 1, 1, (45 * 16, 0, 49, 17)) == (2, 2 * 4 * 6)
    # anchored at MCU 1: one strip of 8 MCUs wherever it sits
    assert hjd.roi_geometry(W, H, 1, 1, (16, 16, 128, 16)) == (1, 48)
    assert hjd.roi_geometry(W, H, 1, 1, (16, 16, 129, 16)) == (2, 96)


def _refused(hjd, w, h, s, scale, roi, match):
    from ocljpegdecoder_amd._lib import HjdError
    with pytest.raises(HjdError, match=match) as e:
        hjd.roi_geometry(w, h, s, scale, roi)
    assert e.value.code == -1, e.value   # HJD_E_INVALID


@pytest.mark.parametrize("scale", [1, 2, 4, 8])
@pytest.mark.parametrize("s", SCALED)
def test_refusals(hjd, s, scale):
    gw, gh = hjd.scaled_size(W, H, scale)
    for roi in [(0, 0, 0, 1), (0, 0, 1, 0), (0, 0, -1, 1), (0, 0, 1, -3)]:
        _refused(hjd, W, H, s, scale, roi, "roi")
    for roi in [(-1, 0, 1, 1), (0, -1, 1, 1)]:
        _refused(hjd, W, H, s, scale, roi, "roi")
    for roi in [(0, 0, gw + 1, 1), (0, 0, 1, gh + 1), (gw, 0, 1, 1), (0, gh, 1, 1), (1, 0, gw, gh), (0, 1, gw, gh)]:
        _refused(hjd, W, H, s, scale, roi, "roi")
    assert hjd.roi_geometry(W, H, s, scale, (gw - 1, gh - 1, 1, 1))[0] == 1


def test_refuses_a_scaled_422(hjd):
    _refused(hjd, W, H, hjd.YUV422, 2, (0, 0, 1, 1), "scaled decode")
    assert hjd.roi_geometry(W, H, hjd.YUV422, 1, (0, 0, 1, 1)) == (1, 48)
    _refused(hjd, W, H, hjd.YUV420, 3, (0, 0, 1, 1), "scale")


def test_declarations_and_abi(hjd):
    inc = os.path.join(O.REPO, "include")
    hjd_h = open(os.path.join(inc, "hjd.h")).read()
    host_h = open(os.path.join(inc, "hjd_host.h")).read()
    assert re.search(r"#define\s+HJD_ABI_VERSION\s+1\b", hjd_h)
    assert re.search(r"typedef struct hjd_rect\s*\{\s*int32_t x, y, w, h;\s*\}\s*hjd_rect;", hjd_h)
    for decl in (r"int\s+hjd_roi_geometry\(int width, int height, int sampling, int scale, const hjd_rect\* roi,\s*"
                 r"int64_t\* tasks,\s*int64_t\* blocks\);",
                 r"int\s+hjd_plan_create_roi\([^;]*int scale, const hjd_rect\* rois, hjd_plan\*\* out\);",
                 r"int\s+hjd_plan_has_roi\(const hjd_plan\*"):
        assert re.search(decl, hjd_h), decl
    assert re.search(r"int\s+hjd_gdec_decode_roi\(hjd_gdec\*[^;]*const hjd_rect\* rois,[^;]*\);", host_h)
    from ocljpegdecoder_amd import _lib
    lib = _lib.load()
    assert lib.hjd_abi_version() == 1
    for name in ("hjd_roi_geometry", "hjd_plan_create_roi", "hjd_plan_has_roi", "hjd_gdec_decode_roi"):
        assert getattr(lib, name)
    assert ctypes.sizeof(_lib.HjdFrame) == 48      # hjd_frame keeps its layout
    assert ctypes.sizeof(_lib.HjdRect) == 16
    # through the raw C entry point, without the Python wrapper
    raw = ctypes.CDLL(os.path.join(O.REPO, "ocljpegdecoder_amd", "lib", "libhjd.so"))
    r = _lib.HjdRect(16, 16, 129, 16)
    t, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert raw.hjd_roi_geometry(W, H, 1, 1, ctypes.byref(r), ctypes.byref(t), ctypes.byref(b)) == 0
    assert (t.value, b.value) == (2, 96)
    r.w = W
    assert raw.hjd_roi_geometry(W, H, 1, 1, ctypes.byref(r), ctypes.byref(t), ctypes.byref(b)) == -1


def test_python_names(hjd):
    assert "roi_geometry" in hjd.__all__
    assert inspect.signature(hjd.FrameSpec).parameters["roi"].default is None
    assert inspect.signature(hjd.decode_frame).parameters["roi"].default is None
    assert inspect.signature(hjd.GpuDecoder.decode).parameters["rois"].default is None
    assert inspect.signature(hjd.GpuDecoder.decode_rgb).parameters["rois"].default is None
    assert list(inspect.signature(hjd.roi_geometry).parameters) == ["width", "height", "sampling", "scale", "roi"]


def test_frame_spec_resolves_the_pitch_against_the_roi(hjd):
    for fmt, row in ((hjd.OUT_BGRX, 4), (hjd.OUT_BGR24, 3), (hjd.OUT_RGB24, 3), (hjd.OUT_RGB_PLANAR, 1)):
        spec = hjd.FrameSpec(W, H, hjd.YUV420, out_format=fmt, roi=(133, 5, 131, 30))
        assert spec.pitch == hjd.default_pitch(131, fmt)
        for scale in (1, 2):
            c = spec.to_c(scale)
            assert c.out_pitch == hjd.default_pitch(131, fmt) and c.out_pitch >= row * 131
            assert (c.width, c.height) == (W, H)     # the record keeps the source size
        assert spec.out_size(2) == (131, 30)
        assert hjd.FrameSpec(W, H, hjd.YUV420, out_format=fmt, roi=(0, 0, 9, 9), out_pitch=64).to_c().out_pitch == 64
    whole = hjd.FrameSpec(W, H, hjd.YUV420)
    assert whole.pitch == 4 * W and whole.out_size(2) == hjd.scaled_size(W, H, 2)
