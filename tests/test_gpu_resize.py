"""The resize kernel alone (hjd_resize_*, backend.Resize) on seeded random
uint8 planes.  The expectation is tests/resize_model.py, the numpy model of the
definition in include/hjd.h; payloads are compared bit for bit (the float
planes on their bit patterns), and no byte outside a payload may be written:
every output lies in a 0xA5-filled buffer with guard bands."""
import functools

import numpy as np
import pytest

import norm_model as N
import resize_model as R

pytestmark = pytest.mark.gpu

FILL = 0xA5
DTYPES = ["uint8", "float16", "float32"]
BITS = {"uint8": np.uint8, "float16": np.uint16, "float32": np.uint32}
# the CPU test's shapes up to 400x40: an upscale, the identity's source, a reduction, one pixel, one row of output taps
SHAPES = [(5, 3), (16, 8), (37, 29), (1, 1), (400, 40)]


@functools.lru_cache(maxsize=None)
def _imagenet():
    import ocljpegdecoder_amd as hjd
    a, b = hjd.norm_constants(N.IMAGENET_MEAN, N.IMAGENET_STD)
    return tuple(float(v) for v in a), tuple(float(v) for v in b)


@functools.lru_cache(maxsize=None)
def _src(w, h):
    a = np.random.default_rng(1000 * w + h).integers(0, 256, (3, h, w), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _model_u8(w, h, wo, ho, flip):
    a = R.resize_u8(_src(w, h), wo, ho, flip)
    a.setflags(write=False)
    return a


def _expect(w, h, wo, ho, flip, dtype, norm):
    u8 = _model_u8(w, h, wo, ho, bool(flip))
    return u8 if dtype == "uint8" else N.apply(u8, norm[0], norm[1], np.dtype(dtype))


def _place_sources(shapes, offset=64, pad=0):
    """The sources on the device: each (3, h, w) at `offset` bytes of a buffer
    of its own, rows w + pad bytes apart, as a [..., :w] view."""
    import torch
    views = []
    for w, h in shapes:
        sp = w + pad
        host = np.full(offset + 3 * h * sp + 64, 0x3C, np.uint8)
        host[offset:offset + 3 * h * sp].reshape(3, h, sp)[..., :w] = _src(w, h)
        buf = torch.from_numpy(host).cuda()
        views.append(buf[offset:offset + 3 * h * sp].view(3, h, sp)[..., :w])
    return views


def _resize(hjd, ctx, shapes, wo, ho, dtype, flips=None, norm=None, src_offset=64, src_pad=0, guard=64, row_pad=0,
            relaunch_with=None):
    """One Resize object over `shapes` -> (N, 3, ho, wo) of dtype inside a
    0xA5-filled buffer (guard bytes in front, rows wo + row_pad elements
    apart); returns the payload's bit patterns (N, 3, ho, wo) and asserts that
    no other byte was written.  relaunch_with: constants set before a second
    launch of the same object, whose result is returned instead."""
    import torch
    n, elem = len(shapes), np.dtype(dtype).itemsize
    p = wo + row_pad
    nbytes = n * 3 * ho * p * elem
    total = guard + nbytes + 64
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[guard:guard + nbytes].view(getattr(torch, dtype)).view(n, 3, ho, p)[..., :wo]
    srcs = _place_sources(shapes, src_offset, src_pad)
    r = hjd.Resize(ctx, srcs, out, flips=flips, normalize=norm if dtype != "uint8" else None)
    r.launch()
    if relaunch_with is not None:
        torch.cuda.synchronize()
        r.set_normalize(*relaunch_with)
        r.launch()
    torch.cuda.synchronize()
    r.close()
    full = buf.cpu().numpy()
    idx = guard + np.arange(n * 3 * ho)[:, None] * (p * elem) + np.arange(wo * elem)[None, :]
    outside = np.ones(total, bool)
    outside[idx.ravel()] = False
    assert (full[outside] == FILL).all(), "bytes outside the payload were written"
    return np.ascontiguousarray(full[idx]).view(BITS[dtype]).reshape(n, 3, ho, wo)


def _check(hjd, ctx, shapes, wo, ho, dtype, flips=None, **kw):
    norm = _imagenet()
    got = _resize(hjd, ctx, shapes, wo, ho, dtype, flips=flips, norm=norm, **kw)
    for k, (w, h) in enumerate(shapes):
        np.testing.assert_array_equal(got[k], _expect(w, h, wo, ho, flips[k] if flips else False, dtype, norm),
                                      err_msg=f"item {k}: {w}x{h} -> {wo}x{ho} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_batch_in_one_launch(hjd, ctx, dtype):
    """Five sources of different sizes, one output size, every second item flipped (vector stores)."""
    _check(hjd, ctx, SHAPES, 24, 16, dtype, flips=[k % 2 == 1 for k in range(len(SHAPES))])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wo,ho", [(10, 7), (7, 5), (4, 1)])
def test_each_shape_alone(hjd, ctx, wo, ho, dtype):
    """Output widths that end inside a lane's four pixels (guarded stores), and one row of one quad."""
    for k, shape in enumerate(SHAPES):
        _check(hjd, ctx, [shape], wo, ho, dtype, flips=[k % 2 == 0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_is_the_source(hjd, ctx, dtype):
    w, h = 16, 8
    got = _resize(hjd, ctx, [(w, h)], w, h, dtype)   # a = 1, b = 0: the float planes hold the bytes' values
    exp = _src(w, h) if dtype == "uint8" else _src(w, h).astype(dtype).view(BITS[dtype])
    np.testing.assert_array_equal(got[0], exp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_source_pitch_and_address(hjd, ctx, dtype):
    _check(hjd, ctx, SHAPES, 24, 16, dtype, flips=[True, False, False, True, False], src_offset=61, src_pad=3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_pad,guard", [(1, 64),    # pitch 25 / 50 / 100 bytes: element-aligned, not 4 / 8 / 16
                                           (4, 64),    # pitch 28 / 56 / 112: the vector path with a gap after each row
                                           (0, 68)])   # aligned pitch, base not a multiple of 8 / 16 (bytes: of 4 below)
def test_destination_pitch_and_address(hjd, ctx, dtype, row_pad, guard):
    if dtype == "uint8" and guard == 68:
        guard = 61
    _check(hjd, ctx, SHAPES[:3], 24, 16, dtype, flips=[False, True, False], row_pad=row_pad, guard=guard)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_quads_than_threads(hjd, ctx, dtype):
    """1024 x 260: 66560 quads per image against 256 groups x 256 threads, so
    some threads take a second quad (the loop), and every image has many groups."""
    _check(hjd, ctx, [(37, 29), (5, 3)], 1024, 260, dtype, flips=[False, True])


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_set_normalize_between_two_launches(hjd, ctx, dtype):
    other = ((2.0, 0.5, 1.0 / 255.0), (-1.0, 0.0, 0.25))
    got = _resize(hjd, ctx, SHAPES[:2], 10, 7, dtype, norm=_imagenet(), relaunch_with=other)
    for k, (w, h) in enumerate(SHAPES[:2]):
        np.testing.assert_array_equal(got[k], _expect(w, h, 10, 7, False, dtype, other))
        assert not np.array_equal(got[k], _expect(w, h, 10, 7, False, dtype, _imagenet()))


def test_refusals_leave_nothing_behind(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    src = torch.zeros((3, 8, 8), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 3, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        hjd.Resize(ctx, [src, src], out)                      # two sources, one output image
    with pytest.raises(ValueError):
        hjd.Resize(ctx, [src], out.permute(0, 1, 3, 2))       # rows are not contiguous
    with pytest.raises(ValueError):
        hjd.Resize(ctx, [src.to(torch.int32)], out)
    r = hjd.Resize(ctx, [src], out)
    with pytest.raises(HjdError, match="HJD_OUT_RGB_PLANAR_F16") as e:
        r.set_normalize(1.0, 0.0)                             # a byte-format object has no constants
    assert e.value.code == -1
    r.launch()
    torch.cuda.synchronize()
    r.close()
    assert int(out.max()) == 0
