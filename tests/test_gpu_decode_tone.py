"""JPEG bytes -> one resized or warped batch with a tone curve per image:
GpuDecoder.decode_rgb_resized_tone / decode_rgb_warped_tone
(hjd_gdec_decode_resized_tone, _warped_tone).  The expectation is the tone
model (tests/tone_model.py) applied to the uint8 batch the call without tones
gives -- the colour call's where colours are given, which the colour suite
pins against its own model -- then normalised; every comparison is bit for
bit (the float planes on their bit patterns)."""
import numpy as np
import pytest

import tone_model as T
from test_gpu_decode_color import DTYPES, _colors, _guarded, _guards_untouched
from test_gpu_decode_resized import ROIS_1, _bits, _decoder, _files, _imagenet, _kw
from test_gpu_decode_warped import FILLS, REPLICATE, _sizes, _xforms

pytestmark = pytest.mark.gpu

SIZES = [(16, 24), (7, 23)]   # (h, w): whole quads and vector stores; guarded ones
MODES = [T.EQUALIZE, T.TABLE, T.AUTOCONTRAST, T.EQUALIZE]


def _curves(hjd):
    """One table per file, with MODES: solarize behind equalize, a posterize table alone, the
    identity behind autocontrast, a random table per channel behind equalize."""
    rng = np.random.default_rng(17)
    return [hjd.tone_curve(solarize=128), hjd.tone_curve(posterize=3, gamma=0.8), hjd.TONE_IDENTITY,
            rng.integers(0, 256, (3, 256), dtype=np.uint8)]


def _expect(hjd, base_u8, curves, modes, dtype):
    a, b = _imagenet(hjd)
    return [T.tone(base_u8[k], modes[k], np.asarray(curves[k]), np.dtype(dtype), a, b) for k in range(len(curves))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_resized_tone_is_the_model_on_the_resized_batch(hjd, ctx, size, dtype):
    datas, decoded = _files()
    flips = [True, False, False, True]
    curves, colors = _curves(hjd), _colors(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for rois, cols in (([ROIS_1[k] for k in range(4)], None), (None, colors), (None, None)):
            if cols is None:
                base = gd.decode_rgb_resized(list(datas), size, flips=flips, rois=rois)
            else:
                base = gd.decode_rgb_resized_color(list(datas), size, flips=flips, rois=rois, colors=cols)
            gd.sync()
            base = base.cpu().numpy()
            buf, out, nbytes = _guarded(4, size, dtype)
            got = gd.decode_rgb_resized_tone(list(datas), size, flips=flips, out=out, rois=rois, colors=cols, curves=curves,
                                             modes=MODES, **_kw(dtype))
            gd.sync()
            assert got is out
            assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX and gd.normalize == ((1.0,) * 3, (0.0,) * 3)
            _guards_untouched(buf, nbytes)
            for k, e in enumerate(_expect(hjd, base, curves, MODES, dtype)):
                np.testing.assert_array_equal(_bits(out[k], dtype), e,
                                              err_msg=f"file {k}, rois {rois is not None}, colours {cols is not None}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_warped_tone_is_the_model_on_the_warped_batch(hjd, ctx, size, dtype):
    datas, decoded = _files()
    xf = _xforms(hjd, _sizes(1), size)
    curves, colors = _curves(hjd), _colors(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for kw, cols in (({}, None), ({"orientations": [3, 6, 8, 1]}, colors)):
            if cols is None:
                base = gd.decode_rgb_warped(list(datas), size, xf, fill=FILLS, replicate=REPLICATE, **kw)
            else:
                base = gd.decode_rgb_warped_color(list(datas), size, xf, fill=FILLS, replicate=REPLICATE, colors=cols, **kw)
            gd.sync()
            base = base.cpu().numpy()
            buf, out, nbytes = _guarded(4, size, dtype)
            got = gd.decode_rgb_warped_tone(list(datas), size, xf, fill=FILLS, replicate=REPLICATE, out=out, colors=cols,
                                            curves=curves, modes=MODES, **kw, **_kw(dtype))
            gd.sync()
            assert got is out and gd.out_format == hjd.OUT_BGRX
            _guards_untouched(buf, nbytes)
            for k, e in enumerate(_expect(hjd, base, curves, MODES, dtype)):
                np.testing.assert_array_equal(_bits(out[k], dtype), e, err_msg=f"file {k}, {kw}")


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_identity_curves_are_the_call_without_tones(hjd, ctx, dtype):
    datas, decoded = _files()
    size = (7, 10)
    colors = _colors(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for kw in ({}, {"antialias": True}, {"orientations": [6, 3, 8, 2]}):
            base = gd.decode_rgb_resized(list(datas), size, **kw, **_kw(dtype))
            for tone_kw in ({}, {"curves": [hjd.TONE_IDENTITY] * 4, "modes": [hjd.TONE_TABLE] * 4},
                            {"curves": hjd.tone_curve(), "modes": 0}):
                got = gd.decode_rgb_resized_tone(list(datas), size, **tone_kw, **kw, **_kw(dtype))
                gd.sync()
                np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype), err_msg=str((kw, list(tone_kw))))
        base = gd.decode_rgb_resized_color(list(datas), size, colors=colors, **_kw(dtype))
        got = gd.decode_rgb_resized_tone(list(datas), size, colors=colors, **_kw(dtype))
        gd.sync()
        np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype), err_msg="with colours")
        xf = _xforms(hjd, _sizes(1), size)
        base = gd.decode_rgb_warped(list(datas), size, xf, fill=FILLS, **_kw(dtype))
        got = gd.decode_rgb_warped_tone(list(datas), size, xf, fill=FILLS, **_kw(dtype))
        gd.sync()
        np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_resized_tone_antialiased_oriented_and_scaled(hjd, ctx, dtype):
    datas, decoded = _files()
    size = (16, 24)
    curves = _curves(hjd)
    sub = [0, 2]   # scale 2: 4:2:0 and gray
    files, cv, md = [datas[k] for k in sub], [curves[k] for k in sub], [MODES[k] for k in sub]
    kw = {"antialias": True, "orientations": [5, 7], "scale": 2}
    with _decoder(hjd, ctx, datas, decoded) as gd:
        base = gd.decode_rgb_resized(files, size, **kw)
        got = gd.decode_rgb_resized_tone(files, size, curves=cv, modes=md, **kw, **_kw(dtype))
        gd.sync()
        for k, e in enumerate(_expect(hjd, base.cpu().numpy(), cv, md, dtype)):
            np.testing.assert_array_equal(_bits(got[k], dtype), e, err_msg=f"file {sub[k]}")


def test_a_small_batch_reuses_the_scratch_of_a_large_one(hjd, ctx):
    """Four images of 48 x 64 in mode 2, then two of 7 x 10 through the same decoder: `mid` and the
    tables of histograms and curves lie in the grow-only scratch, whose old contents the second call
    must not read."""
    datas, decoded = _files()
    curves = _curves(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for files, size, modes in ((list(datas), (48, 64), [T.EQUALIZE] * 4), (list(datas[:2]), (7, 10), [T.EQUALIZE] * 2),
                                   (list(datas[2:]), (7, 10), [T.AUTOCONTRAST, T.EQUALIZE])):
            cv = curves[:len(files)]
            base = gd.decode_rgb_resized(files, size)
            got = gd.decode_rgb_resized_tone(files, size, curves=cv, modes=modes)
            gd.sync()
            for k, e in enumerate(_expect(hjd, base.cpu().numpy(), cv, modes, "uint8")):
                np.testing.assert_array_equal(_bits(got[k], "uint8"), e, err_msg=f"{len(files)} files at {size}, file {k}")


def test_refused_curves_leave_the_decoder_usable(hjd, ctx):
    from ocljpegdecoder_amd._lib import HjdError
    datas, decoded = _files()
    size = (7, 10)
    curves = _curves(hjd)
    xf = _xforms(hjd, _sizes(1), size)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        first = gd.decode_rgb_resized_tone(list(datas), size, curves=curves, modes=MODES)     # in flight while the refusals come
        with pytest.raises(ValueError, match="one tone table"):
            gd.decode_rgb_resized_tone(list(datas), size, curves=curves[:3])
        with pytest.raises(ValueError, match="one mode"):
            gd.decode_rgb_warped_tone(list(datas), size, xf, modes=[1, 2])
        # refused by the library, before anything is staged or enqueued
        with pytest.raises(HjdError, match=r"frame 2: tone item 2: mode 3 is outside 0..2") as e:
            gd.decode_rgb_resized_tone(list(datas), size, curves=curves, modes=[0, 1, 3, 2])
        assert e.value.code == -1
        with pytest.raises(HjdError, match=r"frame 0: tone item 0: mode -1") as e:
            gd.decode_rgb_warped_tone(list(datas), size, xf, modes=[-1, 0, 0, 0])
        assert e.value.code == -1
        with pytest.raises(HjdError, match="frame 1: roi"):
            gd.decode_rgb_resized_tone(list(datas), size, curves=curves, modes=MODES,
                                       rois=[(0, 0, 8, 8), (70, 0, 20, 8), (0, 0, 8, 8), (0, 0, 8, 8)])
        assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX
        base = gd.decode_rgb_resized(list(datas), size)
        again = gd.decode_rgb_resized_tone(list(datas), size, curves=curves, modes=MODES)
        gd.sync()
        expect = _expect(hjd, base.cpu().numpy(), curves, MODES, "uint8")
        for k in range(4):
            np.testing.assert_array_equal(_bits(first[k], "uint8"), expect[k])
            np.testing.assert_array_equal(_bits(again[k], "uint8"), expect[k])
