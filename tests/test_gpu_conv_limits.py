"""The filter kernel where its 32-bit tile arithmetic and its 64-bit offsets are
at their limits: a row and a column of 16384 pixels at radius 11 under REFLECT,
and source and destination pitches of 2^30 bytes with two rows, so that the
plane offsets inside ONE image reach 2^32.  Bit for bit against
tests/conv_model.py; the outputs lie in 0xA5-filled buffers of which no byte
outside the payload may change (the large ones counted on the device, with
test_gpu_stage_limits.py's helpers).  Each test asserts from the kernel's own
formula that its shape reaches the range it is there for, and prints the value."""
import functools

import numpy as np
import pytest

import conv_model as C
import norm_model as N
from test_gpu_conv import _filter, _item, _numpy_filter, _run
from test_gpu_resize import BITS, _imagenet, _src
from test_gpu_stage_limits import FILL, MAX, PITCH, _dev_source, count_not_fill, rows_of

pytestmark = pytest.mark.gpu

SW, SH = 400, 2   # 7 tiles of 64 columns; REFLECT on two rows takes ry = 1


@functools.lru_cache(maxsize=None)
def _record():
    return _filter(11, 1, C.REFLECT, gain=1)


@pytest.mark.parametrize("w,h,rx,ry", [(MAX, 1, 11, 0), (1, MAX, 0, 11), (MAX - 1, 12, 11, 11)])
def test_at_the_dimension_limits(hjd, ctx, w, h, rx, ry):
    tiles = -(-w // 64) * -(-h // 32)
    print(f"conv {w}x{h} radius ({rx}, {ry}): {tiles} tiles of 64 x 32, last tile at column {64 * (-(-w // 64) - 1)}, row {32 * (-(-h // 32) - 1)}")
    assert max(w, h) >= MAX - 1 and tiles >= 256 and rx < w and ry < h
    for dtype in (["uint8", "float16", "float32"] if (w, h) == (MAX, 1) else ["uint8"]):
        # aligned (vector stores where w is a multiple of 4) and one byte off with padded rows
        items = [_item(w, h, _filter(rx, ry, C.REFLECT, gain=0)), _item(w, h, _filter(rx, ry, C.REFLECT, gain=1, seed=1), 1, 3),
                 _item(w, h, _filter(rx, ry, C.REPLICATE, gain=2)), _item(w, h, _filter(rx, ry, C.KEEP, gain=3), 2, 1)]
        _run(hjd, ctx, items, dtype, _imagenet())


@pytest.mark.parametrize("pitch", [PITCH, PITCH + 1])
def test_source_pitch_of_1gib(hjd, ctx, pitch):
    """Rows 2^30 (+ 1) bytes apart, two rows: plane G lies at 2^31, plane B at 2^32."""
    import torch
    S, f = _src(SW, SH), _record()
    print(f"conv: source row 1 at {pitch}, plane stride {SH * pitch}, plane B at {2 * SH * pitch}")
    assert SH * pitch >= 2 ** 31 and 2 * SH * pitch >= 2 ** 32
    big = torch.empty((3, SH, pitch), dtype=torch.uint8, device="cuda")
    src = big[..., :SW]
    src.copy_(torch.from_numpy(S.copy()))
    filters = [_numpy_filter(hjd, f), _numpy_filter(hjd, dict(f, border=C.KEEP))]
    out = torch.full((2, 3, SH, SW), FILL, dtype=torch.uint8, device="cuda")
    op = hjd.Conv(ctx, [src, src], out, filters=filters)
    op.launch()
    torch.cuda.synchronize()
    op.close()
    for k, rec in enumerate(filters):
        np.testing.assert_array_equal(out[k].cpu().numpy(), C.conv_u8(S, C.from_numpy(rec)), err_msg=f"item {k}")
    np.testing.assert_array_equal(src.cpu().numpy(), S, err_msg="the source was written")
    del big, src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype,pitch", [("uint8", PITCH), ("uint8", PITCH + 1), ("float32", PITCH)])
def test_destination_pitch_of_1gib(hjd, ctx, dtype, pitch):
    """Output rows 2^30 bytes apart (+ 1 for the bytes: element stores only), two rows per plane:
    plane B lies at 2^32.  The payload is compared on the host, the rest of the 6 GiB buffer counted
    on the device."""
    import torch
    S, norm, f = _src(SW, SH), _imagenet(), _record()
    elem, guard = np.dtype(dtype).itemsize, 64
    print(f"conv {dtype}: output row 1 at {pitch}, plane stride {SH * pitch}, plane B at {2 * SH * pitch}")
    assert SH * pitch >= 2 ** 31 and 2 * SH * pitch >= 2 ** 32
    buf = torch.empty((guard + 3 * SH * pitch + 64 + (-3 * SH * pitch) % 8,), dtype=torch.uint8, device="cuda")
    small = _dev_source(S)
    for wo in (SW, SW - 1):   # the vector stores, the per-element stores
        buf.fill_(FILL)
        carrier = buf[guard:guard + 3 * SH * wo * elem].view(getattr(torch, dtype)).view(3, SH, wo)
        op = hjd.Conv(ctx, [small[..., :wo]], [(carrier, pitch)], filters=_numpy_filter(hjd, f),
                      normalize=norm if dtype != "uint8" else None)
        op.launch()
        torch.cuda.synchronize()
        op.close()
        e = C.conv_u8(np.ascontiguousarray(S[..., :wo]), f)
        got = rows_of(buf, guard, 3 * SH, pitch, wo * elem)
        bits = e if dtype == "uint8" else N.apply(e, norm[0], norm[1], np.dtype(dtype))
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(BITS[dtype]).reshape(3, SH, wo), bits, err_msg=f"wo {wo}")
        assert count_not_fill(buf) == int((got != FILL).sum()), f"bytes outside the payload were written: wo {wo}"
    del buf, carrier
    torch.cuda.empty_cache()
