"""JPEG bytes -> one resized or warped batch with a colour record per image:
GpuDecoder.decode_rgb_resized_color / decode_rgb_warped_color
(hjd_gdec_decode_resized_color, _warped_color).  The expectation is the colour
model (tests/color_model.py) applied to the uint8 batch the call without
colours gives -- which the resized and warped suites pin against their own
models -- then normalised; every comparison is bit for bit (the float planes
on their bit patterns)."""
import numpy as np
import pytest

import color_model as C
import norm_model as N
from test_gpu_decode_resized import ROIS_1, _bits, _decoder, _files, _imagenet, _kw
from test_gpu_decode_warped import FILLS, REPLICATE, _sizes, _xforms
from test_gpu_scaled import FILL

pytestmark = pytest.mark.gpu

DTYPES = ["uint8", "float16", "float32"]
SIZES = [(16, 24), (7, 10)]   # (h, w): whole quads and vector stores; guarded ones


def _colors(hjd):
    """One record per file: a jitter with contrast about the mean, an inverse (p = 0), a
    grayscale with a fixed pivot (p = 0), a saturated record at the limits."""
    return [hjd.color_matrix(brightness=1.2, contrast=0.6, saturation=1.4, hue=0.1),
            hjd.color_matrix(invert=True),
            hjd.color_matrix(contrast=1.5, pivot=100, gray=True),
            [C.MAX_COEF] * 9 + [-C.MAX_COEF] * 9 + [C.MAX_OFFSET // 2] * 3]


def _expect(hjd, base_u8, colors, dtype):
    a, b = _imagenet(hjd)
    return [C.color(base_u8[k], colors[k], np.dtype(dtype), a, b) for k in range(len(colors))]


def _guarded(n, size, dtype):
    import torch
    nbytes = n * 3 * size[0] * size[1] * np.dtype(dtype).itemsize
    buf = torch.full((64 + nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[64:64 + nbytes].view(getattr(torch, dtype)).view(n, 3, size[0], size[1]), nbytes


def _guards_untouched(buf, nbytes):
    full = buf.cpu().numpy()
    assert (full[:64] == FILL).all() and (full[64 + nbytes:] == FILL).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_resized_color_is_the_model_on_the_resized_batch(hjd, ctx, size, dtype):
    datas, decoded = _files()
    flips = [True, False, False, True]
    colors = _colors(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for rois in ([ROIS_1[k] for k in range(4)], None):
            base = gd.decode_rgb_resized(list(datas), size, flips=flips, rois=rois)
            gd.sync()
            base = base.cpu().numpy()
            buf, out, nbytes = _guarded(4, size, dtype)
            got = gd.decode_rgb_resized_color(list(datas), size, flips=flips, out=out, rois=rois, colors=colors, **_kw(dtype))
            gd.sync()
            assert got is out
            assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX and gd.normalize == ((1.0,) * 3, (0.0,) * 3)
            _guards_untouched(buf, nbytes)
            for k, e in enumerate(_expect(hjd, base, colors, dtype)):
                np.testing.assert_array_equal(_bits(out[k], dtype), e, err_msg=f"file {k}, rois {rois is not None}")
        assert any(colors[0][9:18]) and not any(colors[1][9:18])


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_identity_records_are_the_call_without_colours(hjd, ctx, dtype):
    datas, decoded = _files()
    size = (7, 10)
    ident = [list(hjd.COLOR_IDENTITY)] * 4
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for kw in ({}, {"antialias": True}, {"orientations": [6, 3, 8, 2]}, {"scale": 2}):
            sub = [0, 2] if "scale" in kw else [0, 1, 2, 3]        # scale 2: 4:2:0 and gray
            files = [datas[k] for k in sub]
            kw = dict(kw, orientations=kw["orientations"][:len(sub)]) if "orientations" in kw else kw
            base = gd.decode_rgb_resized(files, size, **kw, **_kw(dtype))
            got = gd.decode_rgb_resized_color(files, size, colors=ident[:len(sub)], **kw, **_kw(dtype))
            gd.sync()
            np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype), err_msg=str(kw))
        xf = _xforms(hjd, _sizes(1), size)
        base = gd.decode_rgb_warped(list(datas), size, xf, fill=FILLS, **_kw(dtype))
        got = gd.decode_rgb_warped_color(list(datas), size, xf, fill=FILLS, colors=ident, **_kw(dtype))
        gd.sync()
        np.testing.assert_array_equal(_bits(got, dtype), _bits(base, dtype))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_resized_color_antialiased_oriented_and_scaled(hjd, ctx, dtype):
    datas, decoded = _files()
    size = (16, 24)
    colors = _colors(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for kw in ({"antialias": True}, {"orientations": [6, 3, 8, 2]}, {"orientations": [5, 1, 7, 4], "antialias": True},
                   {"scale": 2}):
            sub = [0, 2] if "scale" in kw else [0, 1, 2, 3]
            files, cols = [datas[k] for k in sub], [colors[k] for k in sub]
            base = gd.decode_rgb_resized(files, size, **kw)
            got = gd.decode_rgb_resized_color(files, size, colors=cols, **kw, **_kw(dtype))
            gd.sync()
            for k, e in enumerate(_expect(hjd, base.cpu().numpy(), cols, dtype)):
                np.testing.assert_array_equal(_bits(got[k], dtype), e, err_msg=f"file {sub[k]}, {kw}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(16, 24), (7, 23)])
def test_warped_color_is_the_model_on_the_warped_batch(hjd, ctx, size, dtype):
    datas, decoded = _files()
    xf = _xforms(hjd, _sizes(1), size)
    colors = _colors(hjd)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for kw in ({}, {"orientations": [3, 6, 8, 1]}):
            base = gd.decode_rgb_warped(list(datas), size, xf, fill=FILLS, replicate=REPLICATE, **kw)
            gd.sync()
            base = base.cpu().numpy()
            buf, out, nbytes = _guarded(4, size, dtype)
            got = gd.decode_rgb_warped_color(list(datas), size, xf, fill=FILLS, replicate=REPLICATE, out=out,
                                             colors=colors, **kw, **_kw(dtype))
            gd.sync()
            assert got is out and gd.out_format == hjd.OUT_BGRX
            _guards_untouched(buf, nbytes)
            for k, e in enumerate(_expect(hjd, base, colors, dtype)):
                np.testing.assert_array_equal(_bits(out[k], dtype), e, err_msg=f"file {k}, {kw}")


def test_refused_records_leave_the_decoder_usable(hjd, ctx):
    from ocljpegdecoder_amd._lib import HjdError
    datas, decoded = _files()
    size = (7, 10)
    colors = _colors(hjd)
    xf = _xforms(hjd, _sizes(1), size)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        first = gd.decode_rgb_resized_color(list(datas), size, colors=colors)     # in flight while the refusals come
        with pytest.raises(ValueError, match="one colour record"):
            gd.decode_rgb_resized_color(list(datas), size, colors=colors[:3])
        with pytest.raises(ValueError, match="one colour record"):
            gd.decode_rgb_warped_color(list(datas), size, xf)
        with pytest.raises(ValueError, match="21 integers"):
            gd.decode_rgb_resized_color(list(datas), size, colors=[colors[0][:20]] + colors[1:])
        # refused by the library, before anything is staged or enqueued
        bad = [list(c) for c in colors]
        bad[1][0] = 40000
        with pytest.raises(HjdError, match=r"frame 1: color item 1: m\[0\] = 40000") as e:
            gd.decode_rgb_resized_color(list(datas), size, colors=bad)
        assert e.value.code == -1
        bad[1][0], bad[2][19] = 4096, -(1 << 23) - 1
        with pytest.raises(HjdError, match=r"frame 2: color item 2: t\[1\]") as e:
            gd.decode_rgb_warped_color(list(datas), size, xf, colors=bad)
        assert e.value.code == -1
        bad[2][19], bad[3][17] = 0, -32768
        with pytest.raises(HjdError, match=r"frame 3: color item 3: p\[8\] = -32768"):
            gd.decode_rgb_resized_color(list(datas), size, colors=bad, antialias=True, orientations=[6] * 4)
        with pytest.raises(HjdError, match="frame 1: roi"):
            gd.decode_rgb_resized_color(list(datas), size, colors=colors,
                                        rois=[(0, 0, 8, 8), (70, 0, 20, 8), (0, 0, 8, 8), (0, 0, 8, 8)])
        assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX
        base = gd.decode_rgb_resized(list(datas), size)
        again = gd.decode_rgb_resized_color(list(datas), size, colors=colors)
        gd.sync()
        expect = _expect(hjd, base.cpu().numpy(), colors, "uint8")
        for k in range(4):
            np.testing.assert_array_equal(_bits(first[k], "uint8"), expect[k])
            np.testing.assert_array_equal(_bits(again[k], "uint8"), expect[k])
