"""Normalised float planar outputs of the fused kernel (OUT_RGB_PLANAR_F16 /
_F32).  The bytes that are converted are the oracle's (scale 1)
or tests/scaled_model.py's; the conversion is tests/norm_model.py's exact
table.  Every comparison is on bit patterns (uint16 / uint32 views), and no
byte outside a frame's payload may be written (0xA5-filled buffers with guard
bands)."""
import functools

import numpy as np
import pytest

import norm_model as N
import oracle_py as O
import scaled_model as M
from test_gpu_roi import _dev_coefs, _files, _expect, _full, _slice
from test_gpu_scaled import FILL, _bytes_of, _frame, _invalid

pytestmark = pytest.mark.gpu

ALL_SAMPLINGS = [0, 1, 3, 4, 5, 6]   # 4:4:4, 4:2:0, 4:2:2, gray, 4:1:1, 4:4:0
SCALED_SAMPLINGS = [0, 1, 4]
SCALES = [2, 4, 8]
W1, H1 = 769, 40                     # two full strips and a partial one for every sampling, cropped edges
WS, HS = 769, 72
DTYPES = ["float16", "float32"]
FMT = {"float16": "OUT_RGB_PLANAR_F16", "float32": "OUT_RGB_PLANAR_F32"}
BITS = {"float16": np.uint16, "float32": np.uint32}


@functools.lru_cache(maxsize=None)
def _imagenet():
    import ocljpegdecoder_amd as hjd
    return hjd.norm_constants(N.IMAGENET_MEAN, N.IMAGENET_STD)


# half subnormals, an exact +0 and half overflow in one frame
EDGE = ((2.0 ** -20, 1.0, 300.0), (0.0, -128.0, 0.0))


@functools.lru_cache(maxsize=None)
def _two_roundings():
    """Constants whose half result depends on the rounding to fp32 in between:
    for some bytes v the exact v * a lies just past a half tie that its fp32
    rounding lands on.  R: a = 2^-26 (ties on the subnormal grid); G, B: the
    first two such multipliers of a seeded search, b = 0."""
    rng = np.random.default_rng(5)
    cand = (rng.uniform(0.5, 2.0, 20000) / 255.0).astype(np.float32)
    x = cand.astype(np.float64)[:, None] * np.arange(256, dtype=np.float64)[None, :]   # exact: 24 + 8 bits
    once = x.astype(np.float16).view(np.uint16)
    twice = x.astype(np.float32).astype(np.float16).view(np.uint16)
    rows = np.flatnonzero((once != twice).any(axis=1))
    assert rows.size >= 2
    a = (np.float32(2.0 ** -26), cand[rows[0]], cand[rows[1]])
    return (tuple(float(v) for v in a), (0.0, 0.0, 0.0)), [np.flatnonzero(once[r] != twice[r]) for r in rows[:2]]


def _planar(bgrx):
    return _bytes_of("OUT_RGB_PLANAR", bgrx)


def _index(ow, oh, pitch, offset, elem):
    return offset + np.arange(3 * oh)[:, None] * pitch + np.arange(ow * elem)[None, :]


def _run(hjd, ctx, d_coefs, qt, w, h, s, dtype, norm, scale=1, roi=None, pad=0, guard=64, kernel=None):
    """One frame into a 0xA5-filled buffer with guard bands; returns the
    payload's bit patterns (3, oh, ow) and asserts that no other byte was
    written.  pad: extra pitch in elements."""
    import torch
    out_format = getattr(hjd, FMT[dtype])
    elem = np.dtype(dtype).itemsize
    ow, oh = (roi[2], roi[3]) if roi is not None else hjd.scaled_size(w, h, scale)
    pitch = elem * (ow + pad)
    total = guard + 3 * oh * pitch + 64
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    spec = hjd.FrameSpec(w, h, s, out_offset=guard, out_pitch=pitch if pad else 0, qt_index=(0, 1, 2),
                         out_format=out_format, roi=roi)
    plan = hjd.Plan(ctx, [spec], 0, qtables=qt, scale=scale, normalize=norm)
    assert plan.out_bytes_needed == guard + (3 * oh - 1) * pitch + elem * ow <= total
    assert plan.pixels == ow * oh
    if kernel is not None:
        plan.set_kernel(kernel)
        assert plan.launch_shape()["kernel"] == ("latency" if kernel == hjd.KERNEL_LATENCY else "persistent")
    plan.launch(d_coefs, buf)
    torch.cuda.synchronize()
    plan.close()
    full = buf.cpu().numpy()
    idx = _index(ow, oh, pitch, guard, elem)
    outside = np.ones(total, bool)
    outside[idx.ravel()] = False
    assert (full[outside] == FILL).all(), "bytes outside the payload were written"
    return np.ascontiguousarray(full[idx]).view(BITS[dtype]).reshape(3, oh, ow)


def _check(hjd, ctx, w, h, s, dtype, norm, scale=1, roi=None, **kw):
    got = _run(hjd, ctx, _dev_coefs(w, h, s), _frame(w, h, s)[1], w, h, s, dtype, norm, scale=scale, roi=roi, **kw)
    full = _full(w, h, s, scale)
    u8 = _planar(full if roi is None else _slice(full, roi))
    exp = N.apply(u8, norm[0], norm[1], dtype) if norm is not None else N.apply(u8, 1, 0, dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (f"{len(bad)} elements differ; first (c, y, x) = {bad[0]}: byte {u8[tuple(bad[0])]}, "
                           f"got {got[tuple(bad[0])]:#x}, expected {exp[tuple(bad[0])]:#x}")
    return u8


# ---- 1: every sampling, both kernels ------------------------------------------------------
@pytest.mark.parametrize("kernel", ["persistent", "latency"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", ALL_SAMPLINGS)
def test_full_size_vs_oracle(hjd, ctx, s, dtype, kernel):
    _check(hjd, ctx, W1, H1, s, dtype, _imagenet(),
           kernel=hjd.KERNEL_LATENCY if kernel == "latency" else hjd.KERNEL_PERSISTENT)


# ---- 2: the guarded path ------------------------------------------------------------------
@pytest.mark.parametrize("how", ["pitch_pad", "offset"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", [0, 1])
def test_guarded_stores(hjd, ctx, s, dtype, how):
    """A pitch pad of one element, or out_offset 66 (F16) / 68 (F32), breaks
    the 8- / 16-byte alignment: every strip takes the per-element stores."""
    kw = {"pad": 1} if how == "pitch_pad" else {"guard": 66 if dtype == "float16" else 68}
    for kernel in (hjd.KERNEL_PERSISTENT, hjd.KERNEL_LATENCY):
        _check(hjd, ctx, W1, H1, s, dtype, _imagenet(), kernel=kernel, **kw)


# ---- 3: rounding mode, subnormals, zero, overflow -------------------------------------------
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_subnormals_zero_and_overflow(hjd, ctx, dtype, pad):
    u8 = _check(hjd, ctx, W1, H1, 1, dtype, EDGE, kernel=hjd.KERNEL_PERSISTENT, pad=pad)
    # the frame holds what the constants are for
    assert (u8[0] < 64).any() and (u8[0] > 0).any()    # R: half subnormals
    assert (u8[1] == 128).any()                        # G: the exact +0
    assert (u8[2] > 218).any() and (u8[2] <= 218).any()   # B: both sides of the half overflow


@pytest.mark.parametrize("pad", [0, 1])
def test_half_is_rounded_twice(hjd, ctx, pad):
    """F16 is the fp32 fma result rounded to half, not one rounding of the
    exact value: constants for which the two differ on bytes the frame holds
    (vector stores and, with the pitch pad, the per-element stores)."""
    norm, vs = _two_roundings()
    u8 = _check(hjd, ctx, W1, H1, 1, "float16", norm, kernel=hjd.KERNEL_PERSISTENT, pad=pad)
    for c, v in ((1, vs[0]), (2, vs[1])):
        assert np.isin(u8[c], v).any(), "the frame lacks the bytes that tell one rounding from two"
    assert np.isin(u8[0], [2, 6, 10]).any()            # ties on the subnormal grid


def test_g_flag_frame(hjd, ctx):
    """test_gpu_scaled's (U, V) = (-200, 200) | (-100, 100) frame: the colour
    stage's flagged path feeds the float stores."""
    import torch
    for s in (0, 1):
        w, h = 96, 32
        pw, _, bpm, _ = O.GEOM[s]
        n = O.frame_blocks(w, h, s)
        comp = O.block_components(s, n)
        left = ((np.arange(n) // bpm) % (w // pw)) < (w // pw) // 2
        coefs = np.zeros((n, 64), np.int16)
        luma = np.flatnonzero(comp == 0)
        coefs[luma, 0] = 8 * (52 + np.arange(luma.size) % 31)
        coefs[comp == 1, 0] = np.where(left, -1600, -800)[comp == 1]
        coefs[comp == 2, 0] = np.where(left, 1600, 800)[comp == 2]
        qt = np.ones((3, 64), np.int32)
        u8 = _planar(M.decode_scaled(coefs, qt, w, h, s, 1))
        for dtype in DTYPES:
            got = _run(hjd, ctx, torch.from_numpy(coefs).cuda(), qt, w, h, s, dtype, _imagenet(),
                       kernel=hjd.KERNEL_PERSISTENT)
            np.testing.assert_array_equal(got, N.apply(u8, *_imagenet(), dtype))


# ---- 4: scaled ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SCALED_SAMPLINGS)
@pytest.mark.parametrize("scale", SCALES)
def test_scaled_vs_model(hjd, ctx, scale, s, dtype):
    _check(hjd, ctx, WS, HS, s, dtype, _imagenet(), scale=scale)


# ---- 5: regions of interest ------------------------------------------------------------------
ROIS_1 = [(132, 9, 500, 22),     # x % 4 == 0: interior strips on vector stores
          (133, 5, 131, 30),     # odd x: per-element stores
          (0, 0, 1, 1),
          (0, 0, W1, H1)]        # the whole frame


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", ALL_SAMPLINGS)
def test_roi_vs_oracle(hjd, ctx, s, dtype):
    for roi in ROIS_1:
        _check(hjd, ctx, W1, H1, s, dtype, _imagenet(), roi=roi)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SCALED_SAMPLINGS)
@pytest.mark.parametrize("scale", SCALES)
def test_scaled_roi_vs_model(hjd, ctx, scale, s, dtype):
    gw, gh = hjd.scaled_size(WS, HS, scale)
    x4 = (gw // 6) // 4 * 4 + 4
    _check(hjd, ctx, WS, HS, s, dtype, _imagenet(), scale=scale, roi=(x4, max(1, gh // 4), gw * 13 // 20, gh // 2))
    _check(hjd, ctx, WS, HS, s, dtype, _imagenet(), scale=scale, roi=(x4 + 1, gh // 8, gw // 6 + 3, gh - gh // 8 - 2))


# ---- 6: a mixed batch in one plan ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("scale", [1, 2])
def test_mixed_batch_in_one_plan(hjd, ctx, scale, s, dtype):
    """Three frames of different sizes (one sampling: a plan has one) at
    distinct offsets of one buffer with gaps between them, at one and sixteen
    tasks per wave: each equals the model and the gaps stay untouched."""
    import torch
    elem = np.dtype(dtype).itemsize
    sizes = [(388, 33), (17, 9), (256, 32)]
    specs, coefs_all, off, blk, qt = [], [], 128, 0, None
    for w, h in sizes:
        coefs, qt = _frame(w, h, s)
        sw, sh = hjd.scaled_size(w, h, scale)
        specs.append(hjd.FrameSpec(w, h, s, coef_offset=blk, out_offset=off, qt_index=(0, 1, 2),
                                   out_format=getattr(hjd, FMT[dtype])))
        coefs_all.append(coefs)
        blk += coefs.shape[0]
        off += 3 * sw * sh * elem + 100   # a gap the kernel must leave alone (a multiple of the element size)
    total = off + 64
    d_coefs = torch.from_numpy(np.concatenate(coefs_all)).cuda()
    plan = hjd.Plan(ctx, specs, hjd.IN_Q16_ZIGZAG, qtables=qt, scale=scale, normalize=_imagenet())
    assert plan.out_bytes_needed <= total
    plan.set_kernel(hjd.KERNEL_PERSISTENT)
    for chunk in (1, 16):
        plan.set_chunk(chunk)
        buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        plan.launch(d_coefs, buf)
        torch.cuda.synchronize()
        full = buf.cpu().numpy()
        inside = np.zeros(total, bool)
        for sp, (w, h) in zip(specs, sizes):
            sw, sh = hjd.scaled_size(w, h, scale)
            idx = _index(sw, sh, elem * sw, sp.out_offset, elem)
            inside[idx.ravel()] = True
            got = np.ascontiguousarray(full[idx]).view(BITS[dtype]).reshape(3, sh, sw)
            exp = N.apply(_planar(_full(w, h, s, scale)), *_imagenet(), dtype)
            np.testing.assert_array_equal(got, exp, err_msg=f"{w}x{h} chunk {chunk}")
        assert (full[~inside] == FILL).all()
    plan.close()


# ---- 7: the 4:4:4 d16 twin and its fallback ----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_d16_twin_equals_its_fallback(hjd, ctx, dtype):
    d, qt = _dev_coefs(W1, H1, 0), _frame(W1, H1, 0)[1]
    a = _run(hjd, ctx, d, qt, W1, H1, 0, dtype, _imagenet(), kernel=hjd.KERNEL_PERSISTENT)
    with hjd.debug_tuning("HJD_D16", "0"):
        assert ctx.d16_gather()[1] is False
        b = _run(hjd, ctx, d, qt, W1, H1, 0, dtype, _imagenet(), kernel=hjd.KERNEL_PERSISTENT)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, N.apply(_planar(_full(W1, H1, 0, 1)), *_imagenet(), dtype))


# ---- 8: JPEG bytes -> normalised tensors ---------------------------------------------------------
def _bits(t):
    import torch
    return t.cpu().numpy().view(np.uint16 if t.dtype == torch.float16 else np.uint32)


def test_decode_rgb_float(hjd, ctx):
    import torch
    datas, decoded = _files()          # 4:2:0 200x120, 4:4:4 131x77, gray 160x90
    datas = list(datas)
    a, b = _imagenet()
    with hjd.GpuDecoder(ctx, 3, 2 * sum(map(len, datas)), 2 * sum(i.nblocks for _, i in decoded)) as gd:
        before = gd.decode_rgb(datas)
        gd.sync()
        for tdt, dtype in ((torch.float16, "float16"), (torch.float32, "float32"), (torch.float16, "float16")):
            # list output, whole frames
            outs = gd.decode_rgb(datas, dtype=tdt, mean=N.IMAGENET_MEAN, std=N.IMAGENET_STD)
            gd.sync()
            assert (gd.out_format, gd.scale) == (hjd.OUT_BGRX, 1)                      # restored
            assert gd.normalize == ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
            for o, d in zip(outs, decoded):
                assert o.dtype == tdt and tuple(o.shape) == (3, d[1].height, d[1].width)
                np.testing.assert_array_equal(_bits(o), N.apply(_planar(_expect(d, 1)), a, b, dtype))
            # ToTensor: no mean, no std
            outs = gd.decode_rgb(datas[:1], dtype=tdt)
            gd.sync()
            np.testing.assert_array_equal(_bits(outs[0]),
                                          N.apply(_planar(_expect(decoded[0], 1)), *hjd.norm_constants(), dtype))
            # out= an (N, 3, h, w) tensor, ROIs on files of different sizes, scale 2
            rois = [(4, 8, 32, 24), (17, 3, 32, 24), (48, 21, 32, 24)]
            batch = torch.full((3, 3, 24, 32), float("nan"), dtype=tdt, device="cuda")
            assert gd.decode_rgb(datas, out=batch, scale=2, rois=rois, dtype=tdt, mean=N.IMAGENET_MEAN,
                                 std=N.IMAGENET_STD) is batch
            gd.sync()
            exp = np.stack([N.apply(_planar(_expect(d, 2, r)), a, b, dtype) for d, r in zip(decoded, rois)])
            np.testing.assert_array_equal(_bits(batch), exp)
            with pytest.raises(ValueError, match="out must be"):                        # the dtype must match
                gd.decode_rgb(datas, out=batch.to(torch.float32 if tdt == torch.float16 else torch.float16),
                              scale=2, rois=rois, dtype=tdt)
            with pytest.raises(ValueError, match="out must be"):
                gd.decode_rgb(datas, out=batch, scale=2, rois=rois)                     # uint8 into a float tensor
        # the decoder's own constants survive a call that brings its own
        own = hjd.norm_constants(0.5, 0.25)
        gd.set_normalize(*own)
        gd.decode_rgb(datas[:1], dtype=torch.float32, mean=N.IMAGENET_MEAN, std=N.IMAGENET_STD)
        gd.sync()
        gd.set_output_format(hjd.OUT_RGB_PLANAR_F32)
        o = torch.empty((3, decoded[0][1].height, decoded[0][1].width), dtype=torch.float32, device="cuda")
        gd.decode(datas[:1], [o])
        gd.sync()
        np.testing.assert_array_equal(_bits(o), N.apply(_planar(_expect(decoded[0], 1)), *own, "float32"))
        gd.set_output_format(hjd.OUT_BGRX)
        # a following uint8 call equals the one before
        after = gd.decode_rgb(datas)
        gd.sync()
        for x, y, d in zip(before, after, decoded):
            assert y.dtype == torch.uint8
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
            np.testing.assert_array_equal(y.cpu().numpy(), _planar(_expect(d, 1)))


# ---- 9: the C default ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_default_constants_write_the_byte_value(hjd, ctx, dtype):
    u8 = _check(hjd, ctx, W1, H1, 1, dtype, None, kernel=hjd.KERNEL_PERSISTENT)
    got = _run(hjd, ctx, _dev_coefs(W1, H1, 1), _frame(W1, H1, 1)[1], W1, H1, 1, dtype, None)
    np.testing.assert_array_equal(got.view(dtype), u8.astype(dtype))     # float(u8), exactly


def test_decode_frame_normalize(hjd, ctx):
    norm = _imagenet()
    out, plan = hjd.decode_frame(ctx, _dev_coefs(W1, H1, 1), _frame(W1, H1, 1)[1], W1, H1, 1,
                                 out_format=hjd.OUT_RGB_PLANAR_F16, normalize=norm, roi=(132, 9, 500, 22))
    import torch
    torch.cuda.synchronize()
    plan.close()
    assert out.dtype == torch.float16 and tuple(out.shape) == (3, 22, 500)
    np.testing.assert_array_equal(_bits(out), N.apply(_planar(_slice(_full(W1, H1, 1, 1), (132, 9, 500, 22))), *norm,
                                                      "float16"))


def test_decode_jpeg_float(hjd, ctx):
    import torch
    datas, decoded = _files()
    norm = _imagenet()
    for fmt, dtype in ((hjd.OUT_RGB_PLANAR_F16, "float16"), (hjd.OUT_RGB_PLANAR_F32, "float32")):
        out = hjd.decode_jpeg(ctx, datas[0], out_format=fmt, normalize=norm)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), N.apply(_planar(_expect(decoded[0], 1)), *norm, dtype))
    with pytest.raises(ValueError, match="normalize"):
        hjd.decode_jpeg(ctx, datas[0], out_format=hjd.OUT_RGB_PLANAR, normalize=norm)


# ---- refusals that need a device ------------------------------------------------------------------
def test_refusals(hjd, ctx):
    import ctypes
    import torch
    from ocljpegdecoder_amd._lib import check
    from ocljpegdecoder_amd.jpeg import _byte_arrays
    qt = O.std_qtables()

    def plan(fmt, in_fmt=0, **kw):
        return hjd.Plan(ctx, [hjd.FrameSpec(100, 40, 1, qt_index=(0, 1, 2), out_format=fmt, **kw)], in_fmt,
                        qtables=qt if in_fmt == 0 else None)

    for fmt in (hjd.OUT_BGRX, hjd.OUT_BGR24, hjd.OUT_RGB24, hjd.OUT_RGB_PLANAR):
        p = plan(fmt)
        with _invalid("hjd_plan_set_normalize"):
            p.set_normalize(1, 0)
        p.close()
        with _invalid("hjd_plan_set_normalize"):
            hjd.Plan(ctx, [hjd.FrameSpec(100, 40, 1, qt_index=(0, 1, 2), out_format=fmt)], 0, qtables=qt,
                     normalize=(1, 0))
    for fmt, elem in ((hjd.OUT_RGB_PLANAR_F16, 2), (hjd.OUT_RGB_PLANAR_F32, 4)):
        with _invalid("HJD_IN_I32_NATURAL"):
            plan(fmt, in_fmt=hjd.IN_I32_NATURAL)
        with _invalid("pitch"):
            plan(fmt, out_offset=elem + 1)
        with _invalid("pitch"):
            plan(fmt, out_pitch=elem * 100 + 1)
        with _invalid("pitch"):
            plan(fmt, out_pitch=elem * 99)
        p = plan(fmt)
        with _invalid("finite"):
            p.set_normalize((1, float("inf"), 1), 0)
        with _invalid("finite"):
            p.set_normalize(1, (0, 0, float("nan")))
        with _invalid("variant"):
            p.set_variant(1)
        p.set_normalize(*_imagenet())
        p.close()
        with hjd.JpegStream(ctx, 1 << 10) as st:
            with _invalid("float"):
                st.set_output_format(fmt)
            assert st.out_format == hjd.OUT_BGRX
        with hjd.GpuJpegStream(ctx, 2, 1 << 16, 1 << 10) as st:
            with _invalid("float"):
                st.set_output_format(fmt)
            assert st.out_format == hjd.OUT_BGRX
        with hjd.GpuDecoder(ctx, 2, 1 << 16, 1 << 10) as gd:
            with _invalid("finite"):
                gd.set_normalize(1, float("nan"))
            gd.set_output_format(fmt)
            # a pitch that is no multiple of the element size, through the raw entry point
            datas, decoded = _files()
            info = decoded[0][1]
            o = torch.empty((3, info.height, info.width + 1), device="cuda",
                            dtype=torch.float16 if elem == 2 else torch.float32)
            _keep, arr_d, arr_s = _byte_arrays([datas[0]])
            ptrs = (ctypes.c_void_p * 1)(o.data_ptr())
            pitches = (ctypes.c_int32 * 1)(elem * info.width + 1)
            with _invalid("pitch"):
                check(gd.lib.hjd_gdec_decode(gd.handle, arr_d, arr_s, 1, ptrs, pitches, None), "hjd_gdec_decode")
