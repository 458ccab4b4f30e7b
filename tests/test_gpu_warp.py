"""The warp kernel alone (hjd_warp_*, backend.Warp) on seeded random uint8
planes.  The expectation is tests/warp_model.py, the numpy model of the
definition in include/hjd.h; payloads are compared bit for bit (the float
planes on their bit patterns), and no byte outside a payload may be written:
every output lies in a 0xA5-filled buffer with guard bands."""
import functools

import numpy as np
import pytest

import norm_model as N
import orient_model as OM
import warp_model as W
from test_gpu_resize import BITS, DTYPES, FILL, _imagenet, _place_sources, _src

pytestmark = pytest.mark.gpu

SHAPES = [(37, 29), (80, 40), (5, 3)]
FILLS = [0x102030, 0, 0xC0FFEE]
REPLICATE = [False, True, False]


@functools.lru_cache(maxsize=None)
def _xforms(wo, ho):
    """37 x 29 turned 30 degrees (its corners leave the image: fill); 80 x 40
    zoomed 0.5 about a point next to its top right corner (taps past two
    edges: replicate); 5 x 3 wholly outside (all fill)."""
    import ocljpegdecoder_amd as hjd
    return (tuple(hjd.warp_xform(37, 29, wo, ho, angle=30.0, zoom=1.3)),
            tuple(hjd.warp_xform(80, 40, wo, ho, zoom=0.5, center=(78.0, 1.5))),
            (65536, 3000, 9 << 16, -2000, 65536, 1 << 16))


@functools.lru_cache(maxsize=None)
def _model_u8(k, wo, ho, xform=None):
    w, h = SHAPES[k]
    a = W.warp_u8(_src(w, h), xform or _xforms(wo, ho)[k], wo, ho, FILLS[k], W.REPLICATE if REPLICATE[k] else 0)
    a.setflags(write=False)
    return a


def _expect(k, wo, ho, dtype, norm, xform=None):
    u8 = _model_u8(k, wo, ho, xform)
    return u8 if dtype == "uint8" else N.apply(u8, norm[0], norm[1], np.dtype(dtype))


def _warp(hjd, ctx, items, wo, ho, dtype, xforms=None, norm=None, src_offset=64, src_pad=0, guard=64, row_pad=0,
          relaunch_with=None, form=None):
    """One Warp object over the items (indices into SHAPES) -> (N, 3, ho, wo)
    of dtype inside a 0xA5-filled buffer (guard bytes in front, rows wo +
    row_pad elements apart); returns the payload's bit patterns and asserts
    that no other byte was written.  relaunch_with: constants set before a
    second launch of the same object, whose result is returned instead.  form:
    None, or the debug launch's way of dealing the output (False row-major,
    True tiled)."""
    import torch
    n, elem = len(items), np.dtype(dtype).itemsize
    p = wo + row_pad
    nbytes = n * 3 * ho * p * elem
    total = guard + nbytes + 64
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[guard:guard + nbytes].view(getattr(torch, dtype)).view(n, 3, ho, p)[..., :wo]
    srcs = _place_sources([SHAPES[k] for k in items], src_offset, src_pad)
    xf = xforms or [_xforms(wo, ho)[k] for k in items]
    r = hjd.Warp(ctx, srcs, out, xf, fills=[FILLS[k] for k in items], replicate=[REPLICATE[k] for k in items],
                 normalize=norm if dtype != "uint8" else None)
    if form is None:
        r.launch()
    else:
        r.launch_form(form)
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


def _check(hjd, ctx, items, wo, ho, dtype, **kw):
    norm = _imagenet()
    got = _warp(hjd, ctx, items, wo, ho, dtype, norm=norm, **kw)
    for j, k in enumerate(items):
        np.testing.assert_array_equal(got[j], _expect(k, wo, ho, dtype, norm),
                                      err_msg=f"item {k}: {SHAPES[k]} -> {wo}x{ho} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wo,ho", [(24, 16), (23, 7)])
def test_three_items_in_one_launch(hjd, ctx, wo, ho, dtype):
    """Different sizes, matrices, fills and border modes; 24 x 16 takes the vector stores, 23 x 7 the guarded ones."""
    assert (_model_u8(2, wo, ho) == np.array([0xC0, 0xFF, 0xEE], np.uint8)[:, None, None]).all()   # wholly outside
    assert len(np.unique(_model_u8(0, wo, ho))) > 16 and len(np.unique(_model_u8(1, wo, ho))) > 16
    _check(hjd, ctx, [0, 1, 2], wo, ho, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_source_pitch_and_address(hjd, ctx, dtype):
    _check(hjd, ctx, [0, 1, 2], 24, 16, dtype, src_offset=61, src_pad=3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_pad,guard", [(1, 64),    # pitch 25 / 50 / 100 bytes: element-aligned, not 4 / 8 / 16
                                           (4, 64),    # pitch 28 / 56 / 112: the vector path with a gap after each row
                                           (0, 65)])   # dst misaligned by one element (65, 66, 68 bytes)
def test_destination_pitch_and_address(hjd, ctx, dtype, row_pad, guard):
    if guard == 65:
        guard = 64 + np.dtype(dtype).itemsize
    _check(hjd, ctx, [0, 1, 2], 24, 16, dtype, row_pad=row_pad, guard=guard)


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_more_tiles_than_waves_and_both_forms(hjd, ctx, dtype):
    """1028 x 260: 257 quads by 260 rows is 33 x 33 tiles of 8 x 8 quads, the
    last of each row one quad wide and the last row four rows high, against
    256 groups of four waves (so some waves take a second tile); row-major it
    is 66820 quads against 65536 threads.  Both ways of dealing the output
    give the model's bytes."""
    wo, ho = 1028, 260
    xf = tuple(hjd.warp_xform(37, 29, wo, ho, angle=-20.0, zoom=0.04))
    exp = _expect(0, wo, ho, dtype, _imagenet(), xform=xf)
    for form in (None, False, True):
        got = _warp(hjd, ctx, [0], wo, ho, dtype, xforms=[xf], norm=_imagenet(), form=form)
        np.testing.assert_array_equal(got[0], exp, err_msg=f"form {form}")


def test_laws_on_the_device(hjd, ctx):
    """The crop and orientation 6 as integer matrices, byte for byte."""
    w, h = SHAPES[0]
    src = _src(w, h)
    got = _warp(hjd, ctx, [0], 24, 16, "uint8", xforms=[(65536, 0, 5 << 16, 0, 65536, 3 << 16)])
    np.testing.assert_array_equal(got[0], src[:, 3:19, 5:29])
    got = _warp(hjd, ctx, [0], h, w, "uint8", xforms=[tuple(W.orient_matrix(6, w, h))])
    np.testing.assert_array_equal(got[0], OM.orient(src, 6))


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_set_normalize_between_two_launches(hjd, ctx, dtype):
    other = ((2.0, 0.5, 1.0 / 255.0), (-1.0, 0.0, 0.25))
    got = _warp(hjd, ctx, [0, 1], 23, 7, dtype, norm=_imagenet(), relaunch_with=other)
    for j in range(2):
        np.testing.assert_array_equal(got[j], _expect(j, 23, 7, dtype, other))
        assert not np.array_equal(got[j], _expect(j, 23, 7, dtype, _imagenet()))


def test_refusals_leave_nothing_behind(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    src = torch.zeros((3, 8, 8), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 3, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        hjd.Warp(ctx, [src, src], out, [W.IDENTITY] * 2)          # two sources, one output image
    with pytest.raises(ValueError):
        hjd.Warp(ctx, [src], out, [W.IDENTITY, W.IDENTITY])       # two matrices, one source
    with pytest.raises(ValueError):
        hjd.Warp(ctx, [src], out, [(1, 2, 3)])
    with pytest.raises(ValueError):
        hjd.Warp(ctx, [src], out, [W.IDENTITY], fills=[1, 2])
    with pytest.raises(HjdError, match="fill") as e:
        hjd.Warp(ctx, [src], out, [W.IDENTITY], fills=[0x1000000])
    assert e.value.code == -1
    r = hjd.Warp(ctx, [src], out, [W.IDENTITY])
    with pytest.raises(HjdError, match="HJD_OUT_RGB_PLANAR_F16"):
        r.set_normalize(1.0, 0.0)                                  # a byte-format object has no constants
    assert r.lib.hjd_debug_warp_launch_form(r.handle, 2, None) == -1 and "form 2" in hjd._lib.error_string()
    r.launch()
    torch.cuda.synchronize()
    r.close()
    assert int(out.max()) == 0
