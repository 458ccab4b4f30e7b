"""HJD_MAX_OUT_PITCH (include/hjd.h): the fused pixel kernel forms a store's
per-lane offset in 32 bits, so out_pitch has an upper bound, B = 2^28, one for
every sampling, scale and output format.  Host only: hjd_frame_check, and
hjd_plan_create / _scaled / _roi (raw, and through Plan) with a stand-in
context -- every frame is checked before the context is first used, and on a
machine without a device a plan that got past the checks would end in the
runtime's own error, not in a plan.  hjd_gdec_decode's per-image pitches need a
decoder, so their refusal is in tests/test_gpu_pitch_limits.py."""
import ctypes
import re
import types

import numpy as np
import pytest

B = 1 << 28
# name -> (bytes per pixel within a row, what pitch and offset must be multiples of)
FORMATS = {"OUT_BGRX": (4, 4), "OUT_BGR24": (3, 4), "OUT_RGB24": (3, 1), "OUT_RGB_PLANAR": (1, 1),
           "OUT_RGB_PLANAR_F16": (2, 2), "OUT_RGB_PLANAR_F32": (4, 4)}
W, H = 40, 16


def _text(pitch, frame=0):
    return f"frame {frame}: out_pitch {pitch} is above HJD_MAX_OUT_PITCH (268435456)"


def _refused(text):
    from ocljpegdecoder_amd._lib import HjdError
    return pytest.raises(HjdError, match=re.escape(text) + "$")


def test_the_bound_is_the_largest_power_of_two_the_lane_offset_takes():
    """(rows - 1) * B + the strip's row bytes <= 2^32 - 1 in every branch of
    colour_stage / colour_stage_scaled (hjd_internal.h has the table): rows the
    32-bit offset spans, strip pixels, at 4 bytes per pixel."""
    branches = {"420": (2, 128), "444": (2, 128), "422": (7, 192), "411": (7, 256), "440": (15, 96), "gray": (7, 384),
                "scaled": (7, 192)}
    assert all(r * B + 4 * px <= 2 ** 32 - 1 for r, px in branches.values())
    assert any(r * 2 * B + 4 * px > 2 ** 32 - 1 for r, px in branches.values())
    assert B & (B - 1) == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_check(hjd, fmt):
    f, (_, align) = getattr(hjd, fmt), FORMATS[fmt]

    def spec(sampling=hjd.YUV420, **kw):
        return hjd.FrameSpec(W, H, sampling, out_format=f, **kw)

    for s in (hjd.YUV444, hjd.YUV420, hjd.YUV422, hjd.GRAY, hjd.YUV411_H4V1, hjd.YUV440):
        hjd.frame_check(spec(s, out_pitch=B))                       # the bound itself is legal
        with _refused(_text(B + align)) as e:
            hjd.frame_check(spec(s, out_pitch=B + align))
        assert e.value.code == -1
    with _refused(_text(2 ** 31 - 4)):
        hjd.frame_check(spec(out_pitch=2 ** 31 - 4))
    for scale in (2, 4, 8):
        hjd.frame_check(spec(out_pitch=B), scale=scale)
        with _refused(_text(B + align)):
            hjd.frame_check(spec(out_pitch=B + align), scale=scale)
    hjd.frame_check(spec(roi=(3, 1, 20, 9), out_pitch=B))
    with _refused(_text(B + align)):
        hjd.frame_check(spec(roi=(3, 1, 20, 9), out_pitch=B + align))
    # the refusals from before the bound keep their text and come first
    with _refused("frame 0: bad output pitch/offset"):
        hjd.frame_check(spec(out_pitch=FORMATS[fmt][0] * W - align))
    if align > 1:
        with _refused("frame 0: bad output pitch/offset"):
            hjd.frame_check(spec(out_pitch=B + 1))


def _stand_in(hjd):
    """A context no call may use: zeroed memory of its own, kept alive by the object."""
    mem = ctypes.create_string_buffer(4096)
    return types.SimpleNamespace(lib=hjd._lib.load(), handle=ctypes.c_void_p(ctypes.addressof(mem)), device=0, _mem=mem)


@pytest.mark.parametrize("fmt", FORMATS)
def test_plans_refuse_it_before_they_use_the_context(hjd, fmt):
    f, (_, align) = getattr(hjd, fmt), FORMATS[fmt]
    ctx = _stand_in(hjd)
    qt = np.ones((3, 64), np.int32)
    ok = hjd.FrameSpec(W, H, hjd.YUV420, qt_index=(0, 1, 2), out_format=f)
    over = hjd.FrameSpec(W, H, hjd.YUV420, qt_index=(0, 1, 2), out_format=f, out_pitch=B + align)
    with _refused("hjd_plan_create failed with status -1: " + _text(B + align)):
        hjd.Plan(ctx, [over], 0, qtables=qt)
    with _refused("hjd_plan_create failed with status -1: " + _text(B + align, 1)):
        hjd.Plan(ctx, [ok, over], 0, qtables=qt)                    # the message names the frame
    with _refused("hjd_plan_create_scaled failed with status -1: " + _text(B + align)):
        hjd.Plan(ctx, [over], 0, qtables=qt, scale=2)
    with _refused("hjd_plan_create_roi failed with status -1: " + _text(B + align)):
        hjd.Plan(ctx, [hjd.FrameSpec(W, H, hjd.YUV420, qt_index=(0, 1, 2), out_format=f, out_pitch=B + align,
                                     roi=(3, 1, 20, 9))], 0, qtables=qt)
    # the C entry point itself
    lib = hjd._lib.load()
    frames = (hjd._lib.HjdFrame * 2)(ok.to_c(), over.to_c())
    rects = (hjd._lib.HjdRect * 2)(hjd._lib.HjdRect(0, 0, W, H), hjd._lib.HjdRect(3, 1, 20, 9))
    plan = ctypes.c_void_p(1)
    rc = lib.hjd_plan_create_roi(ctx.handle, frames, 2, 0, qt.ctypes.data_as(hjd._lib.c_i32p), 3, 1, rects,
                                 ctypes.byref(plan))
    assert rc == -1 and hjd._lib.error_string() == _text(B + align, 1) and not plan.value
