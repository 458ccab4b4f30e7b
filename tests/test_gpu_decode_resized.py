"""JPEG bytes -> one resized batch: GpuDecoder.decode_rgb_resized (hjd_gdec_decode_resized).
The expectation is the resize model (tests/resize_model.py) applied to the crop
of the full decode -- the oracle's at scale 1, tests/scaled_model.py's at scale
2 -- so the pixel kernels' bytes are the ones the other suites pin, and the
comparison is bit for bit (the float planes on their bit patterns)."""
import functools

import numpy as np
import pytest

import norm_model as N
import oracle_py as O
import resize_model as R
import scaled_model as M
from test_entropy_emulation import _pil
from test_gpu_scaled import FILL, _bytes_of

pytestmark = pytest.mark.gpu

DTYPES = ["uint8", "float16", "float32"]
BITS = {"uint8": np.uint8, "float16": np.uint16, "float32": np.uint32}
SIZES = [(16, 24), (7, 10)]   # (h, w)


@functools.lru_cache(maxsize=None)
def _files():
    """q90 PIL files, 64x48 and 80x40: 4:2:0, 4:4:4, gray, 4:2:2, with their coefficients."""
    import ocljpegdecoder_amd as hjd
    datas = (_pil(64, 48, 90, 2, seed=31), _pil(80, 40, 90, 0, seed=32), _pil(64, 48, 90, 0, seed=33, gray=True),
             _pil(80, 40, 90, 1, seed=34))
    decoded = tuple(hjd.decode_coefs(d) for d in datas)
    assert [i.sampling for _, i in decoded] == [hjd.YUV420, hjd.YUV444, hjd.GRAY, hjd.YUV422]
    return datas, decoded


@functools.lru_cache(maxsize=None)
def _full_planar(k, scale):
    """(3, H', W') bytes of file k's whole decode at `scale`, computed once."""
    c, i = _files()[1][k]
    bgrx = (O.decode_q16(c, i.qt, i.width, i.height, i.sampling) if scale == 1 else
            M.decode_scaled(c, i.qt, i.width, i.height, i.sampling, scale))
    p = _bytes_of("OUT_RGB_PLANAR", bgrx)
    p.setflags(write=False)
    return p


def _imagenet(hjd):
    a, b = hjd.norm_constants(N.IMAGENET_MEAN, N.IMAGENET_STD)
    return tuple(float(v) for v in a), tuple(float(v) for v in b)


def _expect(hjd, k, scale, roi, size, flip, dtype):
    full = _full_planar(k, scale)
    crop = full if roi is None else np.ascontiguousarray(full[:, roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]])
    a, b = _imagenet(hjd)
    return R.resize(crop, size[1], size[0], bool(flip), np.dtype(dtype), a, b)


def _kw(dtype):
    import torch
    if dtype == "uint8":
        return {"dtype": torch.uint8}
    return {"dtype": getattr(torch, dtype), "mean": N.IMAGENET_MEAN, "std": N.IMAGENET_STD}


def _decoder(hjd, ctx, datas, decoded):
    return hjd.GpuDecoder(ctx, len(datas), 2 * sum(map(len, datas)), 2 * sum(i.nblocks for _, i in decoded))


def _bits(t, dtype):
    return t.cpu().numpy().view(BITS[dtype])


# rectangles of different sizes, odd x; the whole frame; one pixel
ROIS_1 = {0: (0, 0, 64, 48), 1: (33, 7, 21, 30), 2: (63, 47, 1, 1), 3: (5, 3, 70, 11)}   # files 0..3 at scale 1
ROIS_2 = {0: (3, 1, 20, 23), 2: (0, 0, 32, 24)}                                           # files 0, 2 at scale 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_scale_1_every_sampling(hjd, ctx, size, dtype):
    import torch
    datas, decoded = _files()
    flips = [True, False, False, True]
    with _decoder(hjd, ctx, datas, decoded) as gd:
        for rois in ([ROIS_1[k] for k in range(4)], None):
            # into a 0xA5-filled buffer with guard bands: nothing outside the batch is written
            elem = np.dtype(dtype).itemsize
            nbytes = 4 * 3 * size[0] * size[1] * elem
            buf = torch.full((64 + nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
            out = buf[64:64 + nbytes].view(getattr(torch, dtype)).view(4, 3, size[0], size[1])
            got = gd.decode_rgb_resized(list(datas), size, flips=flips, out=out, rois=rois, **_kw(dtype))
            gd.sync()
            assert got is out
            assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX and gd.normalize == ((1.0,) * 3, (0.0,) * 3)
            full = buf.cpu().numpy()
            assert (full[:64] == FILL).all() and (full[64 + nbytes:] == FILL).all()
            for k in range(4):
                np.testing.assert_array_equal(_bits(out[k], dtype),
                                              _expect(hjd, k, 1, rois[k] if rois else None, size, flips[k], dtype),
                                              err_msg=f"file {k}, rois {rois is not None}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_scale_2(hjd, ctx, size, dtype):
    datas, decoded = _files()
    pick = [0, 2]   # 4:2:0 and gray
    sub = [datas[k] for k in pick]
    with _decoder(hjd, ctx, sub, [decoded[k] for k in pick]) as gd:
        for rois in ([ROIS_2[k] for k in pick], None):
            out = gd.decode_rgb_resized(sub, size, flips=[False, True], scale=2, rois=rois, **_kw(dtype))
            gd.sync()
            assert tuple(out.shape) == (2, 3) + size and gd.scale == 1
            for j, k in enumerate(pick):
                np.testing.assert_array_equal(_bits(out[j], dtype),
                                              _expect(hjd, k, 2, rois[j] if rois else None, size, j == 1, dtype),
                                              err_msg=f"file {k}, rois {rois is not None}")


def test_growing_scratch_and_a_plain_call_in_between(hjd, ctx):
    """Two resized calls on one decoder, the second with larger crops (the
    scratch grows behind the first, which is not synchronised here), and a
    call without a size in between, which is today's decode."""
    datas, decoded = _files()
    size = (16, 24)
    small = [(1, 1, 3, 2), (7, 5, 4, 4), (63, 47, 1, 1), (9, 9, 2, 3)]
    with _decoder(hjd, ctx, datas, decoded) as gd:
        first = gd.decode_rgb_resized(list(datas), size, rois=small)
        plain = gd.decode_rgb(list(datas))
        second = gd.decode_rgb_resized(list(datas), size)        # whole frames: more scratch than `small` took
        third = gd.decode_rgb_resized(list(datas), size, rois=small, flips=[1, 1, 1, 1])   # fits again
        gd.sync()
        for k in range(4):
            np.testing.assert_array_equal(_bits(first[k], "uint8"), _expect(hjd, k, 1, small[k], size, False, "uint8"))
            np.testing.assert_array_equal(plain[k].cpu().numpy(), _full_planar(k, 1))
            np.testing.assert_array_equal(_bits(second[k], "uint8"), _expect(hjd, k, 1, None, size, False, "uint8"))
            np.testing.assert_array_equal(_bits(third[k], "uint8"), _expect(hjd, k, 1, small[k], size, True, "uint8"))


def test_refusals_leave_the_decoder_usable(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    datas, decoded = _files()
    size = (7, 10)
    with _decoder(hjd, ctx, datas, decoded) as gd:
        with pytest.raises(ValueError, match="chw"):
            gd.decode_rgb_resized(list(datas), size, layout="hwc")
        with pytest.raises(ValueError, match="out must be"):
            gd.decode_rgb_resized(list(datas), size, out=torch.empty((4, 3, 7, 11), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError, match="out must be"):
            gd.decode_rgb_resized(list(datas), size, out=torch.empty((4, 3, 7, 10), dtype=torch.float16, device="cuda"))
        for bad in ((0, 10), (7, 0)):
            with pytest.raises(ValueError, match="size"):
                gd.decode_rgb_resized(list(datas), bad)
        with pytest.raises(ValueError, match="flip"):
            gd.decode_rgb_resized(list(datas), size, flips=[1, 0])
        # refused by the library, before anything is enqueued
        with pytest.raises(HjdError, match="frame 1: roi") as e:
            gd.decode_rgb_resized(list(datas), size, rois=[(0, 0, 8, 8), (70, 0, 20, 8), (0, 0, 8, 8), (0, 0, 8, 8)])
        assert e.value.code == -1
        with pytest.raises(HjdError, match="scaled decode") as e:
            gd.decode_rgb_resized(list(datas), size, scale=2)      # the 4:2:2 file
        assert e.value.code == -1
        with pytest.raises(HjdError, match="output size") as e:
            gd.decode_rgb_resized(list(datas), (1, 16385))
        assert e.value.code == -1
        gd.set_output_format(hjd.OUT_RGB24)
        with pytest.raises(HjdError, match="output format"):
            gd.decode_resized(list(datas), torch.empty((4, 3, 7, 10), dtype=torch.uint8, device="cuda"))
        gd.set_output_format(hjd.OUT_BGRX)
        assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX
        out = gd.decode_rgb_resized(list(datas), size)
        gd.sync()
        for k in range(4):
            np.testing.assert_array_equal(_bits(out[k], "uint8"), _expect(hjd, k, 1, None, size, False, "uint8"))
