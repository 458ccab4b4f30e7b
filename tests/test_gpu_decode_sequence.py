"""Calls of different kinds on one GpuDecoder, back to back with no sync()
between them: warped, resized (antialiased, oriented, display rois, flips),
oriented, plain with rois, resized (bilinear), warped again.  They share the
decoder's scratch, which each lays out its own way and the larger ones grow,
and the record area of its batch header.  Each result must equal, bit for bit
(the float planes on their bit patterns), the same call made alone on a fresh
decoder and synced -- which the other suites pin against the numpy models."""
import numpy as np
import pytest

import orient_model as M
from test_gpu_decode_oriented import SPECS, _bits, _decoder, _display_rois, _files, _kw

pytestmark = pytest.mark.gpu

WARP_ORIENTS = [6, 1, 3, 8]
FLIPS = [True, False, False, True]
PLAIN_ROIS = [(3, 5, 20, 9), (1, 0, 8, 8), (31, 23, 1, 1), (7, 2, 30, 11)]   # inside every file at scale 1 and 2


def _calls(hjd, pick, scale):
    """(function of a decoder -> its result, dtype) per call, in the order issued."""
    n = len(pick)
    plain = [_files(None)[k] for k in pick]
    stored = [hjd.scaled_size(SPECS[k][0], SPECS[k][1], scale) for k in pick]
    xf = [hjd.warp_xform(*M.oriented_size(w, h, o), 24, 16, angle=30.0, zoom=1.5)
          for (w, h), o in zip(stored, WARP_ORIENTS)]
    if scale == 1:
        rois7 = _display_rois(7)[:n]
    else:   # the same rectangles on the scaled displayed images
        (w0, h0), (w1, h1), (w2, h2) = [M.oriented_size(w, h, 7) for w, h in stored]
        rois7 = [(w0 - 30, h0 - 17, 30, 17), (0, 0, w1, h1), (w2 - 1, h2 - 1, 1, 1)]

    def warped(gd):
        return gd.decode_rgb_warped(plain, (16, 24), xf, orientations=WARP_ORIENTS[:n], scale=scale, **_kw("float16"))

    def resized_aa(gd):
        return gd.decode_rgb_resized([_files(7)[k] for k in pick], (16, 24), flips=FLIPS[:n], rois=rois7, scale=scale,
                                     apply_exif_orientation=True, antialias=True, **_kw("float16"))

    def oriented(gd):
        return gd.decode_rgb_oriented(plain, orientations=[6] * n, scale=scale, **_kw("uint8"))

    def rois(gd):
        return gd.decode_rgb(plain, rois=PLAIN_ROIS[:n], scale=scale)

    def resized(gd):
        return gd.decode_rgb_resized(plain, (7, 10), scale=scale, **_kw("uint8"))

    return [(warped, "float16"), (resized_aa, "float16"), (oriented, "uint8"), (rois, "uint8"), (resized, "uint8"),
            (warped, "float16")]


def _images(result, dtype):
    """The bit patterns of a call's result: one array per image."""
    return [_bits(t, dtype) for t in result]


@pytest.mark.parametrize("scale,pick", [(1, [0, 1, 2, 3]), (2, [0, 1, 2])])   # scale 2: the samplings it serves
def test_unsynced_sequence_equals_single_calls(hjd, ctx, scale, pick):
    calls = _calls(hjd, pick, scale)
    alone = {}
    for call, dtype in calls:
        if call not in alone:
            with _decoder(hjd, ctx) as gd:
                result = call(gd)
                gd.sync()
                alone[call] = _images(result, dtype)
    with _decoder(hjd, ctx) as gd:
        results = [call(gd) for call, _ in calls]   # no sync() in between
        gd.sync()
        assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX and gd.normalize == ((1.0,) * 3, (0.0,) * 3)
        for step, ((call, dtype), result) in enumerate(zip(calls, results)):
            got = _images(result, dtype)
            assert len(got) == len(pick)
            for k, (g, e) in enumerate(zip(got, alone[call])):
                np.testing.assert_array_equal(g, e, err_msg=f"call {step + 1} ({call.__name__}), file {pick[k]}")
