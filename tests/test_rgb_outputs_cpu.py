"""RGB24 / planar RGB output formats: the Python surface (no GPU)."""
import ocljpegdecoder_amd as hjd
from ocljpegdecoder_amd import backend


def test_constants_exist_and_are_exported():
    assert hjd.OUT_RGB24 == 2 and hjd.OUT_RGB_PLANAR == 3   # include/hjd.h enum hjd_out_format
    assert backend.OUT_RGB24 == 2 and backend.OUT_RGB_PLANAR == 3
    assert "OUT_RGB24" in hjd.__all__ and "OUT_RGB_PLANAR" in hjd.__all__
    assert (hjd.OUT_BGRX, hjd.OUT_BGR24) == (0, 1)


def test_out_bytes_entries():
    assert hjd.OUT_BYTES[hjd.OUT_RGB24] == 3
    assert hjd.OUT_BYTES[hjd.OUT_RGB_PLANAR] == 3
    assert hjd.OUT_BYTES[hjd.OUT_BGRX] == 4 and hjd.OUT_BYTES[hjd.OUT_BGR24] == 3


def test_default_pitch_of_the_rgb_formats_is_contiguous():
    for w in (1, 2, 3, 17, 385, 388, 3840):
        assert hjd.default_pitch(w, hjd.OUT_RGB24) == 3 * w
        assert hjd.default_pitch(w, hjd.OUT_RGB_PLANAR) == w


def test_default_pitch_of_bgrx_and_bgr24_is_unchanged():
    for w in (1, 2, 3, 17, 385, 388, 3840):
        assert hjd.default_pitch(w) == 4 * w
        assert hjd.default_pitch(w, hjd.OUT_BGRX) == 4 * w
        assert hjd.default_pitch(w, hjd.OUT_BGR24) == (3 * w + 3) & ~3


def test_frame_spec_pitch_and_header_enum():
    assert hjd.FrameSpec(17, 9, hjd.YUV420, out_format=hjd.OUT_RGB_PLANAR).pitch == 17
    assert hjd.FrameSpec(17, 9, hjd.YUV420, out_format=hjd.OUT_RGB24).pitch == 51
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hjd.h")).read()
    assert "HJD_OUT_RGB24 = 2" in text and "HJD_OUT_RGB_PLANAR = 3" in text
    assert "#define HJD_ABI_VERSION 1" in text
