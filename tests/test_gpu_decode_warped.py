"""JPEG bytes -> one warped batch: GpuDecoder.decode_rgb_warped / decode_warped
(hjd_gdec_decode_warped).  The expectation is the warp model
(tests/warp_model.py) applied to the full decode -- the oracle's at scale 1,
tests/scaled_model.py's at scale 2 -- through the matrix on the stored image,
composed by hand where an orientation applies; the decoder itself decodes only
the rectangle hjd_warp_roi finds and shifts the matrix to it.  Every
comparison is bit for bit (the float planes on their bit patterns)."""
import numpy as np
import pytest

import orient_model as OM
import warp_model as W
from test_gpu_decode_resized import _bits, _decoder, _files, _full_planar, _imagenet, _kw
from test_gpu_scaled import FILL

pytestmark = pytest.mark.gpu

DTYPES = ["uint8", "float16", "float32"]
SIZES = [(16, 24), (7, 23)]   # (h, w): the vector stores, the guarded ones
FILLS = [0x102030, 0, 0xC0FFEE, 0x0000FF]
REPLICATE = [False, True, False, True]


def _sizes(scale, pick=range(4)):
    """(W', H') of the picked files' decodes at `scale`."""
    return [_full_planar(k, scale).shape[:0:-1] for k in pick]


def _xforms(hjd, sizes, size, displayed=None):
    """One matrix per image of (displayed) size (w, h): turned and zoomed with
    its corners outside; turned the other way, sheared, zoomed in; zoomed out 2x
    and mirrored about a point near a corner; a small turn about the centre."""
    ho, wo = size
    args = [dict(angle=30.0, zoom=1.3), dict(angle=-75.0, zoom=0.8, shear=(10.0, -5.0)),
            dict(zoom=2.0, hflip=True, center=(5.0, 40.5)), dict(angle=10.0, zoom=1.1)]
    return [hjd.warp_xform(w, h, wo, ho, **args[k % 4]) for k, (w, h) in enumerate(displayed or sizes)]


def _expect(hjd, k, scale, m_stored, size, fill, replicate, dtype):
    a, b = _imagenet(hjd)
    return W.warp(_full_planar(k, scale), m_stored, size[1], size[0], fill, W.REPLICATE if replicate else 0,
                  np.dtype(dtype), a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_scale_1_every_sampling(hjd, ctx, size, dtype):
    import torch
    datas, decoded = _files()
    xf = _xforms(hjd, _sizes(1), size)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        # into a 0xA5-filled buffer with guard bands: nothing outside the batch is written (out= is reused)
        elem = np.dtype(dtype).itemsize
        nbytes = 4 * 3 * size[0] * size[1] * elem
        buf = torch.full((64 + nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
        out = buf[64:64 + nbytes].view(getattr(torch, dtype)).view(4, 3, size[0], size[1])
        for fills, replicate in ((FILLS, REPLICATE), ([0] * 4, [False] * 4)):
            got = gd.decode_rgb_warped(list(datas), size, xf, fill=fills, replicate=replicate, out=out, **_kw(dtype))
            gd.sync()
            assert got is out
            assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX and gd.normalize == ((1.0,) * 3, (0.0,) * 3)
            full = buf.cpu().numpy()
            assert (full[:64] == FILL).all() and (full[64 + nbytes:] == FILL).all()
            for k in range(4):
                np.testing.assert_array_equal(_bits(out[k], dtype),
                                              _expect(hjd, k, 1, xf[k], size, fills[k], replicate[k], dtype),
                                              err_msg=f"file {k}")


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_scale_2(hjd, ctx, dtype):
    datas, decoded = _files()
    pick = [0, 1, 2]   # 4:2:0, 4:4:4 and gray: the samplings scale 2 serves
    sub = [datas[k] for k in pick]
    size = (16, 24)
    xf = _xforms(hjd, _sizes(2, pick), size)
    with _decoder(hjd, ctx, sub, [decoded[k] for k in pick]) as gd:
        out = gd.decode_rgb_warped(sub, size, xf, fill=FILLS[:3], replicate=REPLICATE[:3], scale=2, **_kw(dtype))
        gd.sync()
        assert tuple(out.shape) == (3, 3) + size and gd.scale == 1
        for j, k in enumerate(pick):
            np.testing.assert_array_equal(_bits(out[j], dtype),
                                          _expect(hjd, k, 2, xf[j], size, FILLS[j], REPLICATE[j], dtype),
                                          err_msg=f"file {k}")


def _tagged(data, o):
    """The file with an EXIF block that carries orientation o: the same pixels."""
    return OM.with_segments(data, OM.exif_app1(OM.tiff_block(b"II", [(0x0112, 3, 1, o)])))


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_orientations_fold_into_the_matrix(hjd, ctx, dtype):
    datas, decoded = _files()
    size = (16, 24)
    stored = _sizes(1)
    with _decoder(hjd, ctx, [_tagged(d, 6) for d in datas], decoded) as gd:
        for orients, exif in (([3, 6, 8, 1], False), ([6, 6, 6, 6], True), ([5, 2, 7, 4], True)):
            displayed = [OM.oriented_size(w, h, o) for (w, h), o in zip(stored, orients)]
            xf = _xforms(hjd, stored, size, displayed)
            files = [_tagged(d, o) for d, o in zip(datas, orients)] if exif else list(datas)
            kw = {"apply_exif_orientation": True} if exif else {"orientations": orients}
            assert not exif or [hjd.exif_orientation(f) for f in files] == orients
            out = gd.decode_rgb_warped(files, size, xf, fill=FILLS, replicate=REPLICATE, **kw, **_kw(dtype))
            gd.sync()
            for k in range(4):
                m = W.compose_orient(xf[k], stored[k][0], stored[k][1], orients[k])
                np.testing.assert_array_equal(_bits(out[k], dtype),
                                              _expect(hjd, k, 1, m, size, FILLS[k], REPLICATE[k], dtype),
                                              err_msg=f"file {k}, orientation {orients[k]}")
        # whole-pixel matrices: exactly the crop of the oriented image, and the tags are ignored unless asked for
        for o in (3, 6, 8):
            crop = [[65536, 0, 2 << 16, 0, 65536, 1 << 16]] * 4
            out = gd.decode_rgb_warped(list(datas), size, crop, orientations=[o] * 4)
            gd.sync()
            for k in range(4):
                np.testing.assert_array_equal(_bits(out[k], "uint8"), OM.orient(_full_planar(k, 1), o)[:, 1:17, 2:26])
        out = gd.decode_rgb_warped([_tagged(d, 6) for d in datas], size, [W.IDENTITY] * 4)
        gd.sync()
        for k in range(4):
            np.testing.assert_array_equal(_bits(out[k], "uint8"), _full_planar(k, 1)[:, :16, :24])


def test_smaller_crops_reuse_the_scratch_and_outside_is_fill(hjd, ctx):
    """Two warped calls on one decoder, not synchronised in between: whole
    frames first, then maps that read a few pixels (one of them none: wholly
    outside its frame), and a plain call after them."""
    datas, decoded = _files()
    size = (7, 23)
    big = _xforms(hjd, _sizes(1), size)
    small = [[4000, 0, 10 << 16, 0, 4000, 10 << 16], [65536, 0, 78 << 16, 0, 65536, 38 << 16],
             [65536, 0, 500 << 16, 0, 65536, 0], [0, 3000, 0, 3000, 0, 5 << 16]]
    with _decoder(hjd, ctx, datas, decoded) as gd:
        first = gd.decode_rgb_warped(list(datas), size, big, fill=FILLS)
        second = gd.decode_rgb_warped(list(datas), size, small, fill=FILLS, replicate=REPLICATE)
        plain = gd.decode_rgb(list(datas))
        gd.sync()
        assert hjd.warp_roi(64, 48, small[2], 23, 7) == (63, 0, 1, 8)   # what is decoded for it: a sliver at the edge
        for k in range(4):
            np.testing.assert_array_equal(_bits(first[k], "uint8"), _expect(hjd, k, 1, big[k], size, FILLS[k], False, "uint8"))
            np.testing.assert_array_equal(_bits(second[k], "uint8"),
                                          _expect(hjd, k, 1, small[k], size, FILLS[k], REPLICATE[k], "uint8"))
            np.testing.assert_array_equal(plain[k].cpu().numpy(), _full_planar(k, 1))
        assert (_bits(second[2], "uint8") == np.array([0xC0, 0xFF, 0xEE], np.uint8)[:, None, None]).all()


def test_refusals_leave_the_decoder_usable(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    datas, decoded = _files()
    size = (7, 23)
    xf = _xforms(hjd, _sizes(1), size)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        with pytest.raises(ValueError, match="one matrix"):
            gd.decode_rgb_warped(list(datas), size, xf[:3])
        with pytest.raises(ValueError, match="six integers"):
            gd.decode_rgb_warped(list(datas), size, [xf[0][:5]] + xf[1:])
        with pytest.raises(ValueError, match="out must be"):
            gd.decode_rgb_warped(list(datas), size, xf, out=torch.empty((4, 3, 7, 24), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError, match="size"):
            gd.decode_rgb_warped(list(datas), (0, 23), xf)
        with pytest.raises(ValueError, match="fill"):
            gd.decode_rgb_warped(list(datas), size, xf, fill=[0, 0, 0x1000000, 0])
        # refused by the library, before anything is enqueued
        out = torch.empty((4, 3) + size, dtype=torch.uint8, device="cuda")
        gd.set_output_format(hjd.OUT_RGB24)           # a non-planar layout
        with pytest.raises(HjdError, match="output format") as e:
            gd.decode_warped(list(datas), out, xf)
        assert e.value.code == -1
        gd.set_output_format(hjd.OUT_BGRX)
        with pytest.raises(HjdError, match="frame 3: .*scaled decode") as e:
            gd.decode_rgb_warped(list(datas), size, xf, scale=2)      # the 4:2:2 file
        assert e.value.code == -1
        with pytest.raises(HjdError, match="frame 1: .*orientation 9"):
            gd.decode_rgb_warped(list(datas), size, xf, orientations=[1, 9, 1, 1])
        with pytest.raises(HjdError, match="frame 2: .*leaves int32"):
            gd.decode_rgb_warped(list(datas), size, [xf[0], xf[1], [-(1 << 31), 0, 0, 0, 65536, 0], xf[3]],
                                 orientations=[1, 1, 2, 1])
        with pytest.raises(HjdError, match="output size"):
            gd.decode_rgb_warped(list(datas), (1, 16385), xf)
        assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX
        plain = gd.decode_rgb(list(datas))
        out = gd.decode_rgb_warped(list(datas), size, xf)
        gd.sync()
        for k in range(4):
            np.testing.assert_array_equal(plain[k].cpu().numpy(), _full_planar(k, 1))
            np.testing.assert_array_equal(_bits(out[k], "uint8"), _expect(hjd, k, 1, xf[k], size, 0, False, "uint8"))
