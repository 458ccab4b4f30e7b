"""The colour kernels where their 32-bit quad arithmetic and their 64-bit
offsets are at their limits: images of 16384 x 1 and 1 x 16384, and source and
destination pitches of 2^30 bytes with two rows, so that the plane offsets
inside ONE image reach 2^32.  Bit for bit against tests/color_model.py; the
outputs lie in 0xA5-filled buffers of which no byte outside the payload may
change (the large ones counted on the device, with test_gpu_stage_limits.py's
helpers).  Each test asserts from the kernel's own formula that its shape
reaches the range it is there for, and prints the value."""
import numpy as np
import pytest

import color_model as C
import norm_model as N
from test_gpu_color import _records, _run
from test_gpu_resize import BITS, _imagenet, _src
from test_gpu_stage_limits import FILL, MAX, PITCH, _dev_source, _small, count_not_fill, rows_of

pytestmark = pytest.mark.gpu

SW, SH = 40, 2


@pytest.mark.parametrize("w,h", [(MAX, 1), (1, MAX), (MAX - 1, 1)])
def test_at_the_dimension_limits(hjd, ctx, w, h):
    quads = -(-w // 4) * h
    groups = min(256, -(-quads // 256))
    print(f"color {w}x{h}: {quads} quads in {groups} groups of 256 threads")
    assert max(w, h) >= MAX - 1 and groups >= 16
    recs = _records()
    src = _src(w, h)
    for dtype in (["uint8", "float16", "float32"] if (w, h) == (MAX, 1) else ["uint8"]):
        # aligned (dword loads, vector stores where w is a multiple of 4) and one byte off with padded rows
        items = [(src, recs["random_p0"], 0, 0, 0, 0), (src, recs["limits+1-1+1"], 1, 3, 1, 3),
                 (src, recs["inverse"], 0, 0, 0, 0)]
        _run(hjd, ctx, items, dtype, _imagenet())


@pytest.mark.parametrize("pitch", [PITCH, PITCH + 1])
def test_source_pitch_of_1gib(hjd, ctx, pitch):
    """Rows 2^30 (+ 1: the byte loads) bytes apart, two rows: plane G lies at 2^31, plane B at 2^32.
    Both kernels read them (the record has a p)."""
    import torch
    S = np.ascontiguousarray(_small(SW, 3)[:, :SH])
    print(f"color: source row 1 at {pitch}, plane stride {SH * pitch}, plane B at {2 * SH * pitch}")
    assert SH * pitch >= 2 ** 31 and 2 * SH * pitch >= 2 ** 32
    big = torch.empty((3, SH, pitch), dtype=torch.uint8, device="cuda")
    src = big[..., :SW]
    src.copy_(torch.from_numpy(S))
    recs = [_records()["random_p1"], _records()["inverse"]]
    out = torch.full((2, 3, SH, SW), FILL, dtype=torch.uint8, device="cuda")
    op = hjd.Color(ctx, [src, src], out, recs)
    op.launch()
    torch.cuda.synchronize()
    op.close()
    for k, rec in enumerate(recs):
        np.testing.assert_array_equal(out[k].cpu().numpy(), C.color_u8(S, rec), err_msg=f"item {k}")
    np.testing.assert_array_equal(src.cpu().numpy(), S, err_msg="the source was written")
    del big, src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_destination_pitch_of_1gib(hjd, ctx, dtype):
    """Output rows 2^30 bytes apart (2^28 float elements), two rows per plane: plane B lies at 2^32.
    The payload is compared on the host, the rest of the 6 GiB buffer counted on the device."""
    import torch
    S, norm = np.ascontiguousarray(_small(SW, 3)[:, :SH]), _imagenet()
    elem, guard = np.dtype(dtype).itemsize, 64
    print(f"color {dtype}: output row 1 at {PITCH}, plane stride {SH * PITCH}, plane B at {2 * SH * PITCH}")
    assert SH * PITCH >= 2 ** 31 and 2 * SH * PITCH >= 2 ** 32
    buf = torch.empty((guard + 3 * SH * PITCH + 64,), dtype=torch.uint8, device="cuda")
    small = _dev_source(S)
    rec = _records()["random_p2"]
    exp = C.color_u8(S, rec)
    for wo in (SW, SW - 1):                         # the vector stores, the per-element stores
        buf.fill_(FILL)
        carrier = buf[guard:guard + 3 * SH * wo * elem].view(getattr(torch, dtype)).view(3, SH, wo)
        op = hjd.Color(ctx, [small[..., :wo]], [(carrier, PITCH)], [rec], normalize=norm if dtype != "uint8" else None)
        op.launch()
        torch.cuda.synchronize()
        op.close()
        e = C.color_u8(np.ascontiguousarray(S[..., :wo]), rec)
        got = rows_of(buf, guard, 3 * SH, PITCH, wo * elem)
        bits = e if dtype == "uint8" else N.apply(e, norm[0], norm[1], np.dtype(dtype))
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(BITS[dtype]).reshape(3, SH, wo), bits, err_msg=f"wo {wo}")
        assert count_not_fill(buf) == int((got != FILL).sum()), f"bytes outside the payload were written: wo {wo}"
    assert exp.shape == (3, SH, SW)
    del buf, carrier
    torch.cuda.empty_cache()
