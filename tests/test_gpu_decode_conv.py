"""JPEG bytes -> one resized or warped batch with a filter per image:
GpuDecoder.decode_rgb_resized_aug / decode_rgb_warped_aug
(hjd_gdec_decode_resized_aug, _warped_aug).  The expectation is the filter
model (tests/conv_model.py) applied to the uint8 batch the call without filters
gives -- the colour call's where colours are given, which the colour suite pins
against its own model -- then the tone model (tests/tone_model.py) where tones
follow (a histogram is that of the filtered image), then normalised; every
comparison is bit for bit (the float planes on their bit patterns)."""
import numpy as np
import pytest

import conv_model as C
import norm_model as N
import tone_model as T
from test_gpu_decode_color import DTYPES, _colors, _guarded, _guards_untouched
from test_gpu_decode_resized import ROIS_1, _bits, _decoder, _files, _imagenet, _kw
from test_gpu_decode_warped import FILLS, REPLICATE, _sizes, _xforms

pytestmark = pytest.mark.gpu

SIZES = [(16, 24), (7, 23)]   # (h, w): whole quads and vector stores; guarded ones
MODES = [T.EQUALIZE] * 4      # equalize behind a blur: the histogram is of the blurred image


def _convs(hjd):
    """One filter per file: a Gaussian blur (radius 3, REFLECT), a sharpness record (KEEP), the identity
    among the others, an unsharp mask under REPLICATE."""
    return [hjd.conv_gaussian(1.0), hjd.conv_sharpness(1.8), hjd.CONV_IDENTITY, hjd.conv_unsharp(0.7, 1.5, border=hjd.CONV_REPLICATE)]


def _curves(hjd):
    rng = np.random.default_rng(18)
    return [hjd.tone_curve(solarize=128), hjd.TONE_IDENTITY, hjd.tone_curve(posterize=3), rng.integers(0, 256, (3, 256), dtype=np.uint8)]


def _expect(hjd, base_u8, convs, dtype, curves=None, modes=None):
    a, b = _imagenet(hjd)
    out = []
    for k in range(len(convs)):
        u8 = C.conv_u8(base_u8[k], C.from_numpy(convs[k]))
        if curves is not None:
            u8 = T.tone_u8(u8, modes[k], np.asarray(curves[k]))
        out.append(u8 if dtype == "uint8" else N.apply(u8, a, b, np.dtype(dtype)))
    return out


# conv alone, colour + conv, conv + tone, all three
CASES = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_resized_aug_is_the_model_on_the_resized_batch(hjd, ctx, size, dtype):
    datas, decoded = _files()
    flips = [True, False, False, True]
    convs, curves, colors = _convs(hjd), _curves(hjd), _colors(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for k, (with_colors, with_tones) in enumerate(CASES):
            rois = [ROIS_1[i] for i in range(4)] if k == 0 else None
            cols = colors if with_colors else None
            if cols is None:
                base = gd.decode_rgb_resized(list(datas), size, flips=flips, rois=rois)
            else:
                base = gd.decode_rgb_resized_color(list(datas), size, flips=flips, rois=rois, colors=cols)
            gd.sync()
            base = base.cpu().numpy()
            buf, out, nbytes = _guarded(4, size, dtype)
            tone_kw = {"curves": curves, "modes": MODES} if with_tones else {}
            got = gd.decode_rgb_resized_aug(list(datas), size, flips=flips, out=out, rois=rois, colors=cols, convs=convs,
                                            **tone_kw, **_kw(dtype))
            gd.sync()
            assert got is out
            assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX and gd.normalize == ((1.0,) * 3, (0.0,) * 3)
            _guards_untouched(buf, nbytes)
            for i, e in enumerate(_expect(hjd, base, convs, dtype, curves if with_tones else None, MODES)):
                np.testing.assert_array_equal(_bits(out[i], dtype), e,
                                              err_msg=f"file {i}, colours {with_colors}, tones {with_tones}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_warped_aug_is_the_model_on_the_warped_batch(hjd, ctx, size, dtype):
    datas, decoded = _files()
    xf = _xforms(hjd, _sizes(1), size)
    convs, curves, colors = _convs(hjd), _curves(hjd), _colors(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for k, (with_colors, with_tones) in enumerate(CASES):
            kw = {"orientations": [3, 6, 8, 1]} if k % 2 else {}
            cols = colors if with_colors else None
            if cols is None:
                base = gd.decode_rgb_warped(list(datas), size, xf, fill=FILLS, replicate=REPLICATE, **kw)
            else:
                base = gd.decode_rgb_warped_color(list(datas), size, xf, fill=FILLS, replicate=REPLICATE, colors=cols, **kw)
            gd.sync()
            base = base.cpu().numpy()
            buf, out, nbytes = _guarded(4, size, dtype)
            tone_kw = {"curves": curves, "modes": MODES} if with_tones else {}
            got = gd.decode_rgb_warped_aug(list(datas), size, xf, fill=FILLS, replicate=REPLICATE, out=out, colors=cols,
                                           convs=convs, **tone_kw, **kw, **_kw(dtype))
            gd.sync()
            assert got is out and gd.out_format == hjd.OUT_BGRX
            _guards_untouched(buf, nbytes)
            for i, e in enumerate(_expect(hjd, base, convs, dtype, curves if with_tones else None, MODES)):
                np.testing.assert_array_equal(_bits(out[i], dtype), e, err_msg=f"file {i}, {kw}, colours {with_colors}, tones {with_tones}")


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_identity_convs_are_the_tone_call_and_none_is_the_plain_call(hjd, ctx, dtype):
    datas, decoded = _files()
    size = (7, 10)
    colors, curves = _colors(hjd), _curves(hjd)
    xf = _xforms(hjd, _sizes(1), size)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        # identity filters: the bytes of the _tone call
        base = gd.decode_rgb_resized_tone(list(datas), size, colors=colors, curves=curves, modes=MODES, **_kw(dtype))
        for convs in ([hjd.CONV_IDENTITY] * 4, hjd.CONV_IDENTITY, [hjd.conv_sharpness(1)] * 4, None):
            got = gd.decode_rgb_resized_aug(list(datas), size, colors=colors, convs=convs, curves=curves, modes=MODES, **_kw(dtype))
            gd.sync()
            np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype))
        base = gd.decode_rgb_warped_tone(list(datas), size, xf, fill=FILLS, curves=curves, modes=MODES, **_kw(dtype))
        got = gd.decode_rgb_warped_aug(list(datas), size, xf, fill=FILLS, convs=hjd.CONV_IDENTITY, curves=curves, modes=MODES,
                                       **_kw(dtype))
        gd.sync()
        np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype))
        # all three None (or the identity): byte for byte the call without stages
        for kw in ({}, {"antialias": True}, {"orientations": [6, 3, 8, 2]}):
            base = gd.decode_rgb_resized(list(datas), size, **kw, **_kw(dtype))
            for aug in ({}, {"convs": hjd.CONV_IDENTITY, "curves": hjd.TONE_IDENTITY, "colors": [hjd.COLOR_IDENTITY] * 4}):
                got = gd.decode_rgb_resized_aug(list(datas), size, **aug, **kw, **_kw(dtype))
                gd.sync()
                np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype), err_msg=str((kw, list(aug))))
        base = gd.decode_rgb_warped(list(datas), size, xf, fill=FILLS, **_kw(dtype))
        got = gd.decode_rgb_warped_aug(list(datas), size, xf, fill=FILLS, **_kw(dtype))
        gd.sync()
        np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_resized_aug_antialiased_oriented_and_scaled(hjd, ctx, dtype):
    datas, decoded = _files()
    size = (16, 24)
    convs, curves = _convs(hjd), _curves(hjd)
    sub = [0, 2]   # scale 2: 4:2:0 and gray
    files, cv, tc, md = [datas[k] for k in sub], [convs[0], convs[3]], [curves[k] for k in sub], [MODES[k] for k in sub]
    kw = {"antialias": True, "orientations": [5, 7], "scale": 2}
    with _decoder(hjd, ctx, datas, decoded) as gd:
        base = gd.decode_rgb_resized(files, size, **kw)
        got = gd.decode_rgb_resized_aug(files, size, convs=cv, curves=tc, modes=md, **kw, **_kw(dtype))
        gd.sync()
        for k, e in enumerate(_expect(hjd, base.cpu().numpy(), cv, dtype, tc, md)):
            np.testing.assert_array_equal(_bits(got[k], dtype), e, err_msg=f"file {sub[k]}")


def test_a_small_batch_reuses_the_scratch_of_a_large_one(hjd, ctx):
    """Four images of 48 x 64 with `mid2` (a blur and equalize), then two of 7 x 10 through the same
    decoder, with and without tones: the regions lie in the grow-only scratch, whose old contents the
    later calls must not read."""
    datas, decoded = _files()
    blur = [hjd.conv_gaussian(1.0), hjd.conv_gaussian(0.6, border=hjd.CONV_REPLICATE), hjd.conv_sharpness(0.3), hjd.conv_gaussian(2.0, ksize=5)]
    curves = _curves(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for files, size, tones in ((list(datas), (48, 64), True), (list(datas[:2]), (7, 10), True), (list(datas[2:]), (7, 10), False),
                                   (list(datas), (48, 64), False)):
            cv, tc, md = blur[:len(files)], curves[:len(files)], MODES[:len(files)]
            base = gd.decode_rgb_resized(files, size)
            got = gd.decode_rgb_resized_aug(files, size, convs=cv, **({"curves": tc, "modes": md} if tones else {}))
            gd.sync()
            for k, e in enumerate(_expect(hjd, base.cpu().numpy(), cv, "uint8", tc if tones else None, md)):
                np.testing.assert_array_equal(_bits(got[k], "uint8"), e, err_msg=f"{len(files)} files at {size}, file {k}")


def test_refused_convs_leave_the_decoder_usable(hjd, ctx):
    from ocljpegdecoder_amd._lib import HjdError
    datas, decoded = _files()
    size = (7, 10)
    convs = _convs(hjd)
    xf = _xforms(hjd, _sizes(1), size)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        first = gd.decode_rgb_resized_aug(list(datas), size, convs=convs)     # in flight while the refusals come
        with pytest.raises(ValueError, match="one filter record"):
            gd.decode_rgb_resized_aug(list(datas), size, convs=convs[:3])
        # refused by the library, before anything is staged or enqueued: REFLECT with a radius >= the out size
        wide = hjd.conv_gaussian(3.0)
        assert int(wide["ry"]) >= 7
        with pytest.raises(HjdError, match=r"frame 2: conv item 2: HJD_CONV_REFLECT needs radius") as e:
            gd.decode_rgb_resized_aug(list(datas), size, convs=[convs[0], convs[1], wide, convs[3]])
        assert e.value.code == -1
        with pytest.raises(HjdError, match=r"frame 0: conv item 0: border 7") as e:
            gd.decode_rgb_warped_aug(list(datas), size, xf, convs=[hjd.conv_filter([4096], [4096], 0, 4096, 7)] + convs[1:])
        assert e.value.code == -1
        with pytest.raises(HjdError, match="frame 1: roi"):
            gd.decode_rgb_resized_aug(list(datas), size, convs=convs, rois=[(0, 0, 8, 8), (70, 0, 20, 8), (0, 0, 8, 8), (0, 0, 8, 8)])
        assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX
        base = gd.decode_rgb_resized(list(datas), size)
        again = gd.decode_rgb_resized_aug(list(datas), size, convs=convs)
        ok = gd.decode_rgb_resized_aug(list(datas), size, convs=hjd.conv_gaussian(3.0, border=hjd.CONV_REPLICATE))   # REPLICATE may be wider than the image
        gd.sync()
        expect = _expect(hjd, base.cpu().numpy(), convs, "uint8")
        wide_rep = _expect(hjd, base.cpu().numpy(), [hjd.conv_gaussian(3.0, border=hjd.CONV_REPLICATE)] * 4, "uint8")
        for k in range(4):
            np.testing.assert_array_equal(_bits(first[k], "uint8"), expect[k])
            np.testing.assert_array_equal(_bits(again[k], "uint8"), expect[k])
            np.testing.assert_array_equal(_bits(ok[k], "uint8"), wide_rep[k])
