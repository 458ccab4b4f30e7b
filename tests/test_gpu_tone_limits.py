"""The tone kernels where their 32-bit quad arithmetic and their 64-bit
offsets are at their limits: images of 16384 x 1 and 1 x 16384, and source and
destination pitches of 2^30 bytes with two rows, so that the plane offsets
inside ONE image reach 2^32.  Modes 1 and 2: the histogram kernel reads the
same addresses.  Bit for bit against tests/tone_model.py; the outputs lie in
0xA5-filled buffers of which no byte outside the payload may change (the
large ones counted on the device, with test_gpu_stage_limits.py's helpers).
Each test asserts from the kernel's own formula that its shape reaches the
range it is there for, and prints the value."""
import functools

import numpy as np
import pytest

import norm_model as N
import tone_model as T
from test_gpu_resize import BITS, _imagenet
from test_gpu_stage_limits import FILL, MAX, PITCH, _dev_source, count_not_fill, rows_of
from test_gpu_tone import _narrow, _run, _tables

pytestmark = pytest.mark.gpu

SW, SH = 400, 2   # 800 pixels: equalize's step is 3, its curve not the identity


@functools.lru_cache(maxsize=None)
def _image():
    a = _narrow(SW, SH)
    assert all(not np.array_equal(T.data_curve(mode, T.histogram(a))[0], np.arange(256)) for mode in (1, 2))
    return a


@pytest.mark.parametrize("w,h", [(MAX, 1), (1, MAX), (MAX - 1, 1)])
def test_at_the_dimension_limits(hjd, ctx, w, h):
    quads = -(-w // 4) * h
    groups = min(256, -(-quads // 256))
    print(f"tone {w}x{h}: {quads} quads in {groups} groups of 256 threads, {min(16, groups)} of the histogram")
    assert max(w, h) >= MAX - 1 and groups >= 16
    src = _narrow(w, h)
    for dtype in (["uint8", "float16", "float32"] if (w, h) == (MAX, 1) else ["uint8"]):
        # aligned (dword loads, vector stores where w is a multiple of 4) and one byte off with padded rows
        items = [(src, T.EQUALIZE, _tables()["random"], 0, 0, 0, 0), (src, T.AUTOCONTRAST, T.IDENTITY, 1, 3, 1, 3),
                 (src, T.EQUALIZE, _tables()["solarize"], 0, 0, 0, 0)]
        _run(hjd, ctx, items, dtype, _imagenet())


@pytest.mark.parametrize("pitch", [PITCH, PITCH + 1])
def test_source_pitch_of_1gib(hjd, ctx, pitch):
    """Rows 2^30 (+ 1: the byte loads) bytes apart, two rows: plane G lies at 2^31, plane B at 2^32.
    The histogram kernel and the tone kernel read them."""
    import torch
    S = _image()
    print(f"tone: source row 1 at {pitch}, plane stride {SH * pitch}, plane B at {2 * SH * pitch}")
    assert SH * pitch >= 2 ** 31 and 2 * SH * pitch >= 2 ** 32
    big = torch.empty((3, SH, pitch), dtype=torch.uint8, device="cuda")
    src = big[..., :SW]
    src.copy_(torch.from_numpy(S))
    modes, lut = [T.AUTOCONTRAST, T.EQUALIZE], _tables()["random"]
    out = torch.full((2, 3, SH, SW), FILL, dtype=torch.uint8, device="cuda")
    op = hjd.Tone(ctx, [src, src], out, curves=lut, modes=modes)
    op.launch()
    torch.cuda.synchronize()
    op.close()
    for k, mode in enumerate(modes):
        np.testing.assert_array_equal(out[k].cpu().numpy(), T.tone_u8(S, mode, lut), err_msg=f"item {k}")
    np.testing.assert_array_equal(src.cpu().numpy(), S, err_msg="the source was written")
    del big, src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype,pitch", [("uint8", PITCH), ("uint8", PITCH + 1), ("float32", PITCH)])
def test_destination_pitch_of_1gib(hjd, ctx, dtype, pitch):
    """Output rows 2^30 bytes apart (+ 1 for the bytes: element stores only), two rows per plane:
    plane B lies at 2^32.  The payload is compared on the host, the rest of the 6 GiB buffer counted
    on the device."""
    import torch
    S, norm = _image(), _imagenet()
    elem, guard = np.dtype(dtype).itemsize, 64
    print(f"tone {dtype}: output row 1 at {pitch}, plane stride {SH * pitch}, plane B at {2 * SH * pitch}")
    assert SH * pitch >= 2 ** 31 and 2 * SH * pitch >= 2 ** 32
    buf = torch.empty((guard + 3 * SH * pitch + 64 + (-3 * SH * pitch) % 8,), dtype=torch.uint8, device="cuda")
    small = _dev_source(S)
    for wo, mode in ((SW, T.EQUALIZE), (SW - 1, T.AUTOCONTRAST)):   # the vector stores, the per-element stores
        buf.fill_(FILL)
        carrier = buf[guard:guard + 3 * SH * wo * elem].view(getattr(torch, dtype)).view(3, SH, wo)
        op = hjd.Tone(ctx, [small[..., :wo]], [(carrier, pitch)], curves=_tables()["random"], modes=mode,
                      normalize=norm if dtype != "uint8" else None)
        op.launch()
        torch.cuda.synchronize()
        op.close()
        e = T.tone_u8(np.ascontiguousarray(S[..., :wo]), mode, _tables()["random"])
        got = rows_of(buf, guard, 3 * SH, pitch, wo * elem)
        bits = e if dtype == "uint8" else N.apply(e, norm[0], norm[1], np.dtype(dtype))
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(BITS[dtype]).reshape(3, SH, wo), bits, err_msg=f"wo {wo}")
        assert count_not_fill(buf) == int((got != FILL).sum()), f"bytes outside the payload were written: wo {wo}"
    del buf, carrier
    torch.cuda.empty_cache()
