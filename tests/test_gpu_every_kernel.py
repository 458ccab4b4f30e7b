"""Every entry of the pixel kernels' table launched once on one
400 x 40 frame through the ordinary plan API.  Before each launch
hjd_debug_kernel_key must map the plan's shape to the entry's key; after it
every payload byte must equal what the sibling tests expect (the oracle, the
scaled model, the float table) and no byte outside the payload may be written
(0xA5-filled buffers with guard bands).  The 24 stage-skipping variants write
wrong pixels by design: they must launch and stay inside the payload."""
import ctypes
import functools

import numpy as np
import pytest

import norm_model as N
import oracle_py as O
from test_gpu_norm_outputs import BITS, _imagenet, _index, _planar
from test_gpu_roi import _full, _slice, _strip
from test_gpu_scaled import FILL, _bytes_of, _extract, _frame, _payload_index

pytestmark = pytest.mark.gpu

W, H = 400, 40        # every sampling: an interior and a cut strip per MCU row, a cropped bottom row; 50 x 5 at 1/8
GUARD = 64
SAMPLING = [0, 1, 3, 4, 5, 6]                          # the kernels' sampling index -> enum hjd_sampling
OUT_BITS = {0: "OUT_BGRX", 32: "OUT_BGR24", 512: "OUT_RGB24", 1024: "OUT_RGB_PLANAR",
            1024 | 1 << 14: "OUT_RGB_PLANAR_F16", 1024 | 1 << 15: "OUT_RGB_PLANAR_F32"}
DTYPE = {"OUT_RGB_PLANAR_F16": "float16", "OUT_RGB_PLANAR_F32": "float32"}
STAGE_BITS = 4 | 8 | 16 | 64 | 256
D16 = 128


def _keys(hjd):
    lib = hjd._lib.load()
    n = lib.hjd_debug_kernel_table(None, 0)
    keys = np.zeros((n, 4), dtype=np.int32)
    lib.hjd_debug_kernel_table(keys.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n)
    assert n == 331
    return [tuple(k) for k in keys.tolist()]


def _is_twin_counterpart(key):
    """A v_perm kernel whose shape takes the d16 twin where that gather is selected."""
    lat, s, f, v = key
    return not lat and s == 0 and f == 0 and (v & ~(32 | 512 | 1024 | 3 << 14 | 1 | STAGE_BITS)) == 0


def _shape(key):
    """The plan that takes the table entry `key`."""
    lat, s, f, v = key
    d = dict(sampling=SAMPLING[s], in_fmt=f, fmt_name=OUT_BITS[v & (32 | 512 | 1024 | 3 << 14)], scale=1 << ((v >> 11) & 3),
             roi=None, variant=v & 3, stages=v & STAGE_BITS, latency=bool(lat))
    if v & (1 << 13):
        # x % 4 == 0; MCU row 1's first strip lies inside on all four sides, row 0 and row 2 are cut
        # above and below, and the second strip is cut on the right
        sw, mh = _strip(d["sampling"], d["scale"])
        d["roi"] = (0, 1, min(sw + 5, -(-W // d["scale"])), 2 * mh)
    return d


@functools.lru_cache(maxsize=None)
def _coefs(s, in_fmt):
    import torch
    coefs, qt = _frame(W, H, s)
    return torch.from_numpy(np.array(coefs if in_fmt == 0 else O.dequant_natural(coefs, qt, s))).cuda()


def _launch(hjd, ctx, key, d16):
    """Create the plan of `key`, check that its shape selects `key`, launch it;
    returns (shape, payload index, the buffer's bytes) after the guard-band check."""
    import torch
    d = _shape(key)
    s, fmt_name, scale, roi = d["sampling"], d["fmt_name"], d["scale"], d["roi"]
    out_format = getattr(hjd, fmt_name)
    ow, oh = (roi[2], roi[3]) if roi else hjd.scaled_size(W, H, scale)
    # a ROI's pitch is padded to 16 bytes, so that its whole strips keep the vector stores
    pitch = -(-hjd.default_pitch(ow, out_format) // 16) * 16 if roi else hjd.default_pitch(ow, out_format)
    idx = (_index(ow, oh, pitch, GUARD, np.dtype(DTYPE[fmt_name]).itemsize) if fmt_name in DTYPE else
           _payload_index(fmt_name, ow, oh, pitch, GUARD))
    total = int(idx.max()) + 1 + GUARD
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    spec = hjd.FrameSpec(W, H, s, out_offset=GUARD, out_pitch=pitch, qt_index=(0, 1, 2), out_format=out_format, roi=roi)
    plan = hjd.Plan(ctx, [spec], d["in_fmt"], qtables=_frame(W, H, s)[1] if d["in_fmt"] == 0 else None, scale=scale,
                    normalize=_imagenet() if fmt_name in DTYPE else None)
    try:
        mode = hjd.KERNEL_LATENCY if d["latency"] else hjd.KERNEL_PERSISTENT
        plan.set_kernel(mode)
        plan.set_variant(d["variant"])
        got = (ctypes.c_int32 * 4)()
        hjd._lib.check(ctx.lib.hjd_debug_kernel_key(s, d["in_fmt"], out_format, scale, int(roi is not None), d["variant"],
                                                    d["stages"], mode, plan.tasks, 0, int(d16), got),
                       "hjd_debug_kernel_key")
        assert tuple(got) == key, (d, d16)
        if d["stages"]:
            plan.launch_stages(d["stages"], _coefs(s, d["in_fmt"]), buf)
        else:
            plan.launch(_coefs(s, d["in_fmt"]), buf)
        torch.cuda.synchronize()
    finally:
        plan.close()
    full = buf.cpu().numpy()
    outside = np.ones(total, bool)
    outside[idx.ravel()] = False
    assert (full[outside] == FILL).all(), f"{key}: bytes outside the payload were written"
    return d, (ow, oh, pitch), full[idx]


def _check_pixels(hjd, ctx, key, d16):
    d, (ow, oh, pitch), px = _launch(hjd, ctx, key, d16)
    bgrx = _full(W, H, d["sampling"], d["scale"])
    if d["roi"]:
        bgrx = _slice(bgrx, d["roi"])
    if d["fmt_name"] in DTYPE:
        dtype = DTYPE[d["fmt_name"]]
        got = np.ascontiguousarray(px).view(BITS[dtype]).reshape(3, oh, ow)
        exp = N.apply(_planar(bgrx), *_imagenet(), dtype)
    else:
        got = px.reshape(3, oh, ow) if d["fmt_name"] == "OUT_RGB_PLANAR" else px.reshape(oh, ow, -1)
        exp = _bytes_of(d["fmt_name"], bgrx)
    np.testing.assert_array_equal(got, exp, err_msg=f"kernel {key}: {d}")


def test_every_product_kernel(hjd, ctx):
    """The 300 product kernels that are no d16 twin; the seven whose shape
    takes a twin where the d16 gather is selected run with HJD_D16=0."""
    keys = [k for k in _keys(hjd) if not k[3] & (STAGE_BITS | D16)]
    assert len(keys) == 300 and sum(map(_is_twin_counterpart, keys)) == 7
    for key in keys:
        if _is_twin_counterpart(key):
            with hjd.debug_tuning("HJD_D16", "0"):
                assert ctx.d16_gather()[1] is False
                _check_pixels(hjd, ctx, key, False)
        else:
            _check_pixels(hjd, ctx, key, ctx.d16_gather()[1])


def test_every_d16_twin(hjd, ctx):
    keys = [k for k in _keys(hjd) if k[3] & D16 and not k[3] & STAGE_BITS]
    assert len(keys) == 7
    if not ctx.d16_gather()[1]:
        pytest.skip("the d16 gather is not selected on this device (probe or HJD_D16): the twins are never launched")
    for key in keys:
        _check_pixels(hjd, ctx, key, True)


@pytest.mark.parametrize("gather", ["v_perm", "d16"])
def test_every_stage_variant(hjd, ctx, gather):
    """Wrong pixels by design: the launch succeeds and writes nothing outside the payload."""
    keys = [k for k in _keys(hjd) if k[3] & STAGE_BITS and bool(k[3] & D16) == (gather == "d16")]
    assert len(keys) == (8 if gather == "d16" else 16)
    if gather == "d16":
        if not ctx.d16_gather()[1]:
            pytest.skip("the d16 gather is not selected on this device (probe or HJD_D16)")
        for key in keys:
            _launch(hjd, ctx, key, True)
    else:
        with hjd.debug_tuning("HJD_D16", "0"):
            for key in keys:
                _launch(hjd, ctx, key, False)


def test_variant_bits_on_the_other_byte_formats(hjd, ctx):
    """include/hjd.h: a BGR24 plan takes hjd_plan_set_variant's bits and fails at
    a persistent launch (its latency kernel ignores them); an RGB24 or planar
    plan refuses them in the setter."""
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    qt = _frame(W, H, 1)[1]
    bgrx = _full(W, H, 1, 1)
    for fmt_name in ("OUT_BGR24", "OUT_RGB24", "OUT_RGB_PLANAR"):
        plan = hjd.Plan(ctx, [hjd.FrameSpec(W, H, 1, qt_index=(0, 1, 2), out_format=getattr(hjd, fmt_name))], 0, qtables=qt)
        try:
            if fmt_name != "OUT_BGR24":
                with pytest.raises(HjdError, match="BGRX-only") as e:
                    plan.set_variant(1)
                assert e.value.code == -1
                continue
            plan.set_variant(1)
            out = torch.zeros(plan.out_bytes_needed, dtype=torch.uint8, device="cuda")
            plan.set_kernel(hjd.KERNEL_PERSISTENT)
            with pytest.raises(HjdError, match="BGRX-only") as e:
                plan.launch(_coefs(1, 0), out)
            assert e.value.code == -1
            plan.set_kernel(hjd.KERNEL_LATENCY)
            plan.launch(_coefs(1, 0), out)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.cpu().numpy().reshape(H, W, 3), _bytes_of("OUT_BGR24", bgrx))
        finally:
            plan.close()
