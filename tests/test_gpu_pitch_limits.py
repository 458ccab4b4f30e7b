"""The fused pixel kernel at HJD_MAX_OUT_PITCH (include/hjd.h), B = 2^28 bytes
between rows: the 32-bit per-lane offset of a store (store4, hjd_kernels.hpp)
then holds up to 15 * B + one strip row, just below 2^32, and the 64-bit plane
stride of the planar formats passes 2^32.  Both kernels, every sampling, the
oracle's pixels (tests/scaled_model.py's at scale 2), bit for bit.  The payload
is compared on the host; that nothing else in the 0xA5-filled buffer changed is
counted on the device.  The buffers are 2 to 6 GiB (rows * B).

Dropped: the planar F32 frame two strips high at the bound (47 rows of B: 11.75
GiB beside the scan's temporaries, past the suite's 12 GiB cap); the planar
formats run one strip high."""
import ctypes

import numpy as np
import pytest

import norm_model as N
from test_gpu_norm_outputs import _imagenet
from test_gpu_roi import _dev_coefs, _full, _slice
from test_gpu_scaled import _bytes_of, _frame
from test_gpu_stage_limits import FILL, count_not_fill, rows_of

pytestmark = pytest.mark.gpu

B = 1 << 28
GUARD = 64
ROW_BYTES = {"OUT_BGRX": 4, "OUT_BGR24": 3, "OUT_RGB24": 3, "OUT_RGB_PLANAR": 1, "OUT_RGB_PLANAR_F32": 4}
# sampling -> (its enum value, rows the lane offset spans, strip width in pixels): hjd_internal.h's table
BRANCH = {"444": (0, 2, 128), "420": (1, 2, 128), "422": (3, 7, 192), "gray": (4, 7, 384), "411": (5, 7, 256),
          "440": (6, 15, 96)}


def _expect(w, h, s, fmt_name, scale, roi, norm):
    full = _full(w, h, s, scale)
    bgrx = full if roi is None else _slice(full, roi)
    if fmt_name != "OUT_RGB_PLANAR_F32":
        return _bytes_of(fmt_name, bgrx)
    return N.apply(_bytes_of("OUT_RGB_PLANAR", bgrx), norm[0], norm[1], "float32")


def _decode_at_bound(hjd, ctx, buf, w, h, s, fmt_name, kernel, scale=1, roi=None):
    """One frame with out_pitch = B into buf (refilled here); compares the
    payload and asserts that no other byte changed."""
    import torch
    planar = fmt_name.startswith("OUT_RGB_PLANAR")
    norm = _imagenet() if fmt_name == "OUT_RGB_PLANAR_F32" else None
    ow, oh = (roi[2], roi[3]) if roi is not None else hjd.scaled_size(w, h, scale)
    rows, row_bytes = (3 * oh if planar else oh), ROW_BYTES[fmt_name] * ow
    need = GUARD + (rows - 1) * B + row_bytes
    assert need + 64 <= buf.numel()
    buf.fill_(FILL)
    spec = hjd.FrameSpec(w, h, s, out_offset=GUARD, out_pitch=B, qt_index=(0, 1, 2), out_format=getattr(hjd, fmt_name),
                         roi=roi)
    plan = hjd.Plan(ctx, [spec], 0, qtables=_frame(w, h, s)[1], scale=scale, normalize=norm)
    assert plan.out_bytes_needed == need
    plan.set_kernel(kernel)
    assert plan.launch_shape()["kernel"] == ("latency" if kernel == hjd.KERNEL_LATENCY else "persistent")
    plan.launch(_dev_coefs(w, h, s), buf)
    torch.cuda.synchronize()
    plan.close()
    got = rows_of(buf, GUARD, rows, B, row_bytes)
    exp = _expect(w, h, s, fmt_name, scale, roi, norm)
    what = f"{w}x{h} sampling {s} {fmt_name} kernel {kernel} scale {scale} roi {roi}"
    if fmt_name == "OUT_RGB_PLANAR_F32":
        np.testing.assert_array_equal(got.view(np.uint32).reshape(3, oh, ow), exp, err_msg=what)
    else:
        np.testing.assert_array_equal(got.reshape(exp.shape), exp, err_msg=what)
    assert count_not_fill(buf) == int((got != FILL).sum()), f"bytes outside the payload were written: {what}"


def _empty_cache():
    import torch
    torch.cuda.empty_cache()


def _buffer(rows):
    import torch
    return torch.empty((GUARD + (rows - 1) * B + 4096,), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("fmt_name", ["OUT_BGRX", "OUT_RGB24"])
@pytest.mark.parametrize("name", list(BRANCH))
def test_every_sampling_at_the_bound(hjd, ctx, name, fmt_name):
    """One MCU row (8 or 16 pixel rows) B bytes apart: w = 40 is one edge strip
    (guarded stores), w = 385 adds full strips (vector stores) and, for gray, the
    second strip column."""
    s, span, strip_w = BRANCH[name]
    h = 16 if name in ("420", "440") else 8
    peak = span * B + 4 * strip_w                   # the largest lane offset the branch can form
    print(f"{name}: rows {h}, lane offset up to {peak} = 2^{np.log2(peak):.3f}, last row at {(h - 1) * B}")
    assert peak <= 2 ** 32 - 1 and (h - 1) * B >= 2 ** 30
    if name == "440":
        assert span * B >= 2 ** 31                  # y * pitch past int32, 15/16 of the way to the wrap
    assert name != "gray" or 385 > strip_w
    buf = _buffer(h)
    for w in (40, 385):
        for kernel in (hjd.KERNEL_PERSISTENT, hjd.KERNEL_LATENCY):
            _decode_at_bound(hjd, ctx, buf, w, h, s, fmt_name, kernel)
    del buf
    _empty_cache()


@pytest.mark.parametrize("fmt_name", ["OUT_RGB_PLANAR", "OUT_RGB_PLANAR_F32"])
def test_planar_gray_frame_plane_stride_past_4gib(hjd, ctx, fmt_name):
    h = 8
    plane = h * B
    print(f"plane stride {plane}, plane B at {2 * plane}, last row at {(3 * h - 1) * B}")
    assert 2 * plane >= 2 ** 32 and (3 * h - 1) * B >= 2 ** 32
    buf = _buffer(3 * h)
    for w in (40, 385):
        for kernel in (hjd.KERNEL_PERSISTENT, hjd.KERNEL_LATENCY):
            _decode_at_bound(hjd, ctx, buf, w, h, 4, fmt_name, kernel)
    del buf
    _empty_cache()


@pytest.mark.parametrize("fmt_name", ["OUT_BGRX", "OUT_RGB24"])
def test_scaled_420_at_the_bound(hjd, ctx, fmt_name):
    """scale 2: 80 x 32 comes out 40 x 16, two scaled strips of 8 rows."""
    assert 7 * B + 4 * 64 <= 2 ** 32 - 1 and 15 * B >= 2 ** 31
    buf = _buffer(16)
    _decode_at_bound(hjd, ctx, buf, 80, 32, 1, fmt_name, hjd.KERNEL_PERSISTENT, scale=2)
    del buf
    _empty_cache()


@pytest.mark.parametrize("fmt_name", ["OUT_BGRX", "OUT_RGB24"])
def test_roi_from_an_odd_x_at_the_bound(hjd, ctx, fmt_name):
    """4:2:0, the rectangle starts at x = 5, y = 3: dx = 5 (guarded stores), dy = 3,
    the strip base 3 * B + 20 bytes in front of the payload, two MCU rows."""
    roi = (5, 3, 40, 16)
    assert roi[0] % 2 == 1 and (roi[3] - 1) * B >= 2 ** 31
    buf = _buffer(16)
    _decode_at_bound(hjd, ctx, buf, 80, 32, 1, fmt_name, hjd.KERNEL_PERSISTENT, roi=roi)
    del buf
    _empty_cache()


def test_refusals_above_the_bound(hjd, ctx):
    """A plan and the GPU decoder's per-image pitches refuse B + the alignment;
    nothing is written and the decoder goes on working."""
    import torch
    from ocljpegdecoder_amd._lib import HjdError, check
    from ocljpegdecoder_amd.jpeg import _byte_arrays
    from test_gpu_roi import _files
    qt = _frame(40, 16, 1)[1]
    with pytest.raises(HjdError, match=r"frame 0: out_pitch 268435472 is above HJD_MAX_OUT_PITCH \(268435456\)$"):
        hjd.Plan(ctx, [hjd.FrameSpec(40, 16, 1, out_pitch=B + 16, qt_index=(0, 1, 2))], 0, qtables=qt)
    hjd.Plan(ctx, [hjd.FrameSpec(40, 16, 1, out_pitch=B, qt_index=(0, 1, 2))], 0, qtables=qt).close()
    datas, decoded = _files()
    info = decoded[0][1]
    out = torch.full((info.height, info.width), -1, dtype=torch.int32, device="cuda")
    with hjd.GpuDecoder(ctx, 2, 1 << 16, 1 << 10) as gd:
        _keep, arr_d, arr_s = _byte_arrays([datas[0]])
        ptrs = (ctypes.c_void_p * 1)(out.data_ptr())
        pitches = (ctypes.c_int32 * 1)(B + 16)
        with pytest.raises(HjdError, match=r"frame 0: out_pitch 268435472 is above HJD_MAX_OUT_PITCH \(268435456\)$"):
            check(gd.lib.hjd_gdec_decode(gd.handle, arr_d, arr_s, 1, ptrs, pitches, None), "hjd_gdec_decode")
        gd.sync()
        assert int(out.min()) == -1 and int(out.max()) == -1
        gd.decode([datas[0]], [out])
        gd.sync()
        assert int(out.min()) != -1
