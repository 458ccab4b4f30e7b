"""Region-of-interest decode in the fused kernel: hjd_plan_create_roi,
FrameSpec(roi=), GpuDecoder.decode_rgb(rois=), jpeg2bmp --roi.  A ROI frame's
output is defined as full[y:y+h, x:x+w] of the same plan without the ROI, so
the expectation is always the cached oracle frame (scale 1) or model frame
(tests/scaled_model.py) sliced; equality is exact, and no byte outside the
w x h payload may be written (0xA5-filled buffers with guard bands)."""
import functools

import numpy as np
import pytest

import oracle_py as O
import scaled_model as M
from test_entropy_emulation import _pil
from test_gpu_scaled import FILL, FORMATS, ROW_BYTES, _bytes_of, _extract, _frame, _invalid, _payload_index

pytestmark = pytest.mark.gpu

ALL_SAMPLINGS = [0, 1, 3, 4, 5, 6]   # 4:4:4, 4:2:0, 4:2:2, gray, 4:1:1, 4:4:0
SCALED_SAMPLINGS = [0, 1, 4]
SCALES = [2, 4, 8]
W1, H1 = 769, 40                     # scale-1 source: two full strips and a partial one for every sampling
WS, HS = 769, 72                     # scaled source


def _strip(s, scale=1):
    """(strip width, MCU height) on the output grid of `scale`."""
    pw, ph, bpm, _ = O.GEOM[s]
    return (48 // bpm) * pw // scale, ph // scale


@functools.lru_cache(maxsize=None)
def _full(w, h, s, scale):
    """BGRX words of the whole frame _frame(w, h, s) at `scale`, computed once."""
    coefs, qt = _frame(w, h, s)
    exp = O.decode_q16(coefs, qt, w, h, s) if scale == 1 else M.decode_scaled(coefs, qt, w, h, s, scale)
    exp.setflags(write=False)
    return exp


def _slice(full, roi):
    x, y, w, h = roi
    return np.ascontiguousarray(full[y:y + h, x:x + w])


@functools.lru_cache(maxsize=None)
def _dev_coefs(w, h, s):
    import torch
    return torch.from_numpy(np.array(_frame(w, h, s)[0])).cuda()


def _decode(hjd, ctx, d_coefs, qt, w, h, s, scale, fmt_name, roi, pad=0, guard=64):
    """One ROI frame into a 0xA5-filled buffer with guard bands; returns the
    payload and asserts that no other byte was written and that the plan's
    counts are roi_geometry's."""
    import torch
    out_format = getattr(hjd, fmt_name)
    rw, rh = roi[2], roi[3]
    pitch = hjd.default_pitch(rw, out_format) + pad
    rows = 3 * rh if fmt_name == "OUT_RGB_PLANAR" else rh
    total = guard + rows * pitch + 64
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    spec = hjd.FrameSpec(w, h, s, out_offset=guard, out_pitch=pitch if pad else 0, qt_index=(0, 1, 2),
                         out_format=out_format, roi=roi)
    plan = hjd.Plan(ctx, [spec], 0, qtables=qt, scale=scale)
    tasks, blocks = hjd.roi_geometry(w, h, s, scale, roi)
    assert plan.has_roi and plan.scale == scale
    assert (plan.tasks, plan.pixels, plan.coef_bytes) == (tasks, rw * rh, 128 * blocks)
    assert plan.out_bytes_needed <= total
    assert plan.launch_shape()["kernel"] == "persistent"
    plan.launch(d_coefs, buf)
    torch.cuda.synchronize()
    plan.close()
    full = buf.cpu().numpy()
    outside = np.ones(total, bool)
    outside[_payload_index(fmt_name, rw, rh, pitch, guard).ravel()] = False
    assert (full[outside] == FILL).all(), "bytes outside the payload were written"
    return _extract(fmt_name, full, rw, rh, pitch, guard)


def _check(hjd, ctx, w, h, s, scale, fmt_name, roi, **kw):
    got = _decode(hjd, ctx, _dev_coefs(w, h, s), _frame(w, h, s)[1], w, h, s, scale, fmt_name, roi, **kw)
    np.testing.assert_array_equal(got, _bytes_of(fmt_name, _slice(_full(w, h, s, scale), roi)), err_msg=str(roi))


# ---- scale 1 ----------------------------------------------------------------------
def _rects_1(s):
    sw, mh = _strip(s)
    return [(0, 0, W1, H1),                  # the whole frame
            (0, 0, 1, 1), (768, 39, 1, 1),
            (sw, mh, sw, mh),                # every task a full aligned strip: vector stores only
            (132, 9, 500, 22),               # x % 4 == 0: cut strips on both sides, interior strips on vector stores
            (133, 5, 131, 30),               # odd x: byte path
            (sw - 2, mh - 2, 4, 4),          # straddles a strip boundary and an MCU-row boundary
            (600, 30, 169, 10)]              # reaches the frame's cropped right and bottom edge


@pytest.mark.parametrize("k", range(8))
@pytest.mark.parametrize("fmt_name", FORMATS)
@pytest.mark.parametrize("s", ALL_SAMPLINGS)
def test_roi_vs_oracle(hjd, ctx, s, fmt_name, k):
    _check(hjd, ctx, W1, H1, s, 1, fmt_name, _rects_1(s)[k])


@pytest.mark.parametrize("fmt_name", FORMATS)
@pytest.mark.parametrize("s", ALL_SAMPLINGS)
def test_pitch_pad(hjd, ctx, s, fmt_name):
    _check(hjd, ctx, W1, H1, s, 1, fmt_name, (132, 9, 500, 22), pad=12)


@pytest.mark.parametrize("fmt_name", ["OUT_RGB24", "OUT_RGB_PLANAR"])
@pytest.mark.parametrize("s", ALL_SAMPLINGS)
def test_odd_out_offset(hjd, ctx, s, fmt_name):
    _check(hjd, ctx, W1, H1, s, 1, fmt_name, (132, 9, 500, 22), guard=61)


def test_fewer_tasks_than_the_whole_frame(hjd, ctx):
    for s in ALL_SAMPLINGS:
        sw, mh = _strip(s)
        whole = hjd.Plan(ctx, [hjd.FrameSpec(W1, H1, s, qt_index=(0, 1, 2))], 0, qtables=_frame(W1, H1, s)[1])
        rows, strips = -(-H1 // mh), -(-W1 // sw)
        assert whole.tasks == rows * strips and not whole.has_roi
        assert hjd.roi_geometry(W1, H1, s, 1, (0, 0, W1, H1))[0] == whole.tasks
        assert hjd.roi_geometry(W1, H1, s, 1, (sw, mh, sw, mh))[0] == 1 < whole.tasks
        # one strip wide wherever it sits: one task per MCU row
        assert hjd.roi_geometry(W1, H1, s, 1, (sw - 2, 0, 4, H1))[0] == rows < whole.tasks
        whole.close()


# ---- scaled -----------------------------------------------------------------------
def _rects_scaled(hjd, s, scale):
    gw, gh = hjd.scaled_size(WS, HS, scale)
    sw, mh = _strip(s, scale)
    x4 = (gw // 6) // 4 * 4 + 4
    return [(0, 0, gw, gh),
            (0, 0, 1, 1), (gw - 1, gh - 1, 1, 1),
            (sw, mh, sw, mh),
            (x4, max(1, gh // 4), gw * 13 // 20, gh // 2),          # x % 4 == 0, cut on both sides
            (x4 + 1, gh // 8, gw // 6 + 3, gh - gh // 8 - 2),       # odd x
            (sw - 2, max(0, mh - 2), 4, 4),                         # straddles a strip and an MCU-row boundary
            (gw - gw // 5, gh - gh // 4, gw // 5, gh // 4)]         # the cropped right and bottom edge


@pytest.mark.parametrize("k", range(8))
@pytest.mark.parametrize("fmt_name", ["OUT_RGB_PLANAR", "OUT_BGRX"])
@pytest.mark.parametrize("s", SCALED_SAMPLINGS)
@pytest.mark.parametrize("scale", SCALES)
def test_scaled_roi_vs_model(hjd, ctx, scale, s, fmt_name, k):
    _check(hjd, ctx, WS, HS, s, scale, fmt_name, _rects_scaled(hjd, s, scale)[k])


# ---- blocks outside the ROI's MCUs are not used ---------------------------------------
@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("s", [0, 1])
def test_outside_blocks_are_not_used(hjd, ctx, s, scale):
    import torch
    w, h = WS, HS
    gw, gh = hjd.scaled_size(w, h, scale)
    roi = (gw // 3 + 1, gh // 4, gw // 3, gh // 2)
    coefs, qt = _frame(w, h, s)
    pw, ph, bpm, _ = O.GEOM[s]
    mw, mh = pw // scale, ph // scale
    mcu_w = -(-w // pw)
    mcu = np.arange(coefs.shape[0]) // bpm
    mx, my = mcu % mcu_w, mcu // mcu_w
    x, y, rw, rh = roi
    inside = (mx >= x // mw) & (mx <= (x + rw - 1) // mw) & (my >= y // mh) & (my <= (y + rh - 1) // mh)
    assert inside.any() and not inside.all()
    noisy = np.array(coefs)
    rng = np.random.default_rng(11 + s + scale)
    noisy[~inside] = rng.integers(-32768, 32768, size=(int((~inside).sum()), 64), dtype=np.int64).astype(np.int16)
    for fmt_name in ("OUT_RGB_PLANAR", "OUT_BGRX"):
        got = _decode(hjd, ctx, torch.from_numpy(noisy).cuda(), qt, w, h, s, scale, fmt_name, roi)
        np.testing.assert_array_equal(got, _bytes_of(fmt_name, _slice(_full(w, h, s, scale), roi)))


# ---- the whole-frame ROI is the plan without -------------------------------------------
@pytest.mark.parametrize("fmt_name", FORMATS)
def test_whole_frame_roi_is_the_plain_plan(hjd, ctx, fmt_name):
    import torch
    w, h, s = 388, 33, 1
    coefs, qt = _frame(w, h, s)
    out_format = getattr(hjd, fmt_name)
    outs = []
    for roi in (None, (0, 0, w, h)):
        plan = hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_format=out_format, roi=roi)], 0, qtables=qt)
        assert plan.has_roi == (roi is not None)
        buf = torch.full((plan.out_bytes_needed + 64,), FILL, dtype=torch.uint8, device="cuda")
        plan.set_kernel(hjd.KERNEL_PERSISTENT)
        plan.launch(_dev_coefs(w, h, s), buf)
        torch.cuda.synchronize()
        outs.append((buf.cpu().numpy(), plan.tasks, plan.pixels, plan.coef_bytes))
        plan.close()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    assert outs[0][1:] == outs[1][1:]
    pitch = hjd.default_pitch(w, out_format)
    np.testing.assert_array_equal(_extract(fmt_name, outs[1][0], w, h, pitch, 0),
                                  _bytes_of(fmt_name, _full(w, h, s, 1)))


# ---- frames of different sizes into one batch tensor -----------------------------------
@pytest.mark.parametrize("s", [1, 0])
def test_mixed_batch_into_one_tensor(hjd, ctx, s):
    """Three frames of different sizes, each with its own 96x32 ROI (MCU
    aligned, x % 4 == 0, odd x), fill one (3, 3, 32, 96) planar tensor; at 1 and
    16 tasks per wave (waves cross frame boundaries)."""
    import torch
    frames = [((388, 49), (32, 16, 96, 32)), ((200, 120), (100, 9, 96, 32)), ((769, 40), (601, 3, 96, 32))]
    specs, coefs_all, blk, qt = [], [], 0, None
    for k, ((w, h), roi) in enumerate(frames):
        coefs, qt = _frame(w, h, s)
        specs.append(hjd.FrameSpec(w, h, s, coef_offset=blk, out_offset=k * 3 * 32 * 96, qt_index=(0, 1, 2),
                                   out_format=hjd.OUT_RGB_PLANAR, roi=roi))
        coefs_all.append(coefs)
        blk += coefs.shape[0]
    d_coefs = torch.from_numpy(np.concatenate(coefs_all)).cuda()
    plan = hjd.Plan(ctx, specs, 0, qtables=qt)
    assert plan.has_roi and plan.pixels == 3 * 96 * 32
    assert plan.tasks == sum(hjd.roi_geometry(w, h, s, 1, roi)[0] for (w, h), roi in frames)
    assert plan.coef_bytes == 128 * sum(hjd.roi_geometry(w, h, s, 1, roi)[1] for (w, h), roi in frames)
    exp = np.stack([_bytes_of("OUT_RGB_PLANAR", _slice(_full(w, h, s, 1), roi)) for (w, h), roi in frames])
    for chunk in (1, 16):
        plan.set_chunk(chunk)
        out = torch.full((3, 3, 32, 96), FILL, dtype=torch.uint8, device="cuda")
        assert plan.out_bytes_needed == out.numel()
        plan.launch(d_coefs, out)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg=f"chunk {chunk}")
    plan.close()


# ---- the G term's corrected path --------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("scale", [1, 2])
def test_g_flag_chroma_pairs(hjd, ctx, scale, s):
    """test_gpu_scaled's (U, V) = (-200, 200) | (-100, 100) frame through a ROI
    that cuts both halves."""
    import torch
    w, h = 96, 32
    pw, _, bpm, _ = O.GEOM[s]
    n = O.frame_blocks(w, h, s)
    mw = w // pw
    comp = O.block_components(s, n)
    left = ((np.arange(n) // bpm) % mw) < mw // 2
    coefs = np.zeros((n, 64), np.int16)
    luma = np.flatnonzero(comp == 0)
    coefs[luma, 0] = 8 * (52 + np.arange(luma.size) % 31)
    coefs[comp == 1, 0] = np.where(left, -1600, -800)[comp == 1]
    coefs[comp == 2, 0] = np.where(left, 1600, 800)[comp == 2]
    qt = np.ones((3, 64), np.int32)
    full = M.decode_scaled(coefs, qt, w, h, s, scale)
    roi = (40 // scale + 1, 5 // scale, 24 // scale, 20 // scale)
    assert roi[0] < (w // 2) // scale < roi[0] + roi[2]
    got = _decode(hjd, ctx, torch.from_numpy(coefs).cuda(), qt, w, h, s, scale, "OUT_BGRX", roi)
    np.testing.assert_array_equal(got, _bytes_of("OUT_BGRX", _slice(full, roi)))


# ---- autotune ------------------------------------------------------------------------
def test_autotune_on_a_roi_plan(hjd, ctx):
    import torch
    w, h, s = 388, 33, 1
    coefs, qt = _frame(w, h, s)
    roi = (0, 0, w, h)   # the same task count as the plain plan: only the ROI flag separates the cache keys

    def spec(r):
        return hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_format=hjd.OUT_RGB_PLANAR, roi=r)

    d = _dev_coefs(w, h, s)
    out = torch.full((3, h, w), FILL, dtype=torch.uint8, device="cuda")
    p = hjd.Plan(ctx, [spec(roi)], 0, qtables=qt)
    hjd.autotune_cache_clear()
    tpw, variant = p.autotune(d, out, rounds=1)
    assert variant == 0 and tpw >= 1 and p.launch_shape()["autotune_launches"] > 0
    p1 = hjd.Plan(ctx, [spec(None)], 0, qtables=qt)
    p1.set_kernel(hjd.KERNEL_PERSISTENT)
    assert p1.tasks == p.tasks
    p1.autotune(d, torch.empty((3, h, w), dtype=torch.uint8, device="cuda"), rounds=1)
    assert p1.launch_shape()["autotune_cached"] == 0
    p1.close()
    p2 = hjd.Plan(ctx, [spec(roi)], 0, qtables=qt)
    p2.autotune(d, out, rounds=1)
    assert p2.launch_shape()["autotune_cached"] == 1
    p2.close()
    out.fill_(FILL)
    p.launch(d, out)
    torch.cuda.synchronize()
    p.close()
    np.testing.assert_array_equal(out.cpu().numpy(), _bytes_of("OUT_RGB_PLANAR", _full(w, h, s, 1)))


# ---- refusals --------------------------------------------------------------------------
def test_refusals(hjd, ctx):
    import torch
    w, h = 100, 40
    qt = O.std_qtables()

    def plan(roi, s=1, in_fmt=0, scale=1, **kw):
        return hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), roi=roi, **kw)], in_fmt,
                        qtables=qt if in_fmt == 0 else None, scale=scale)

    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 101, 1), (0, 0, 1, 41), (100, 0, 1, 1),
                (0, 40, 1, 1), (1, 0, 100, 40)]:
        with _invalid("frame 0: roi"):
            plan(bad)
    for bad in [(0, 0, 51, 1), (0, 0, 1, 21), (50, 0, 1, 1), (0, 20, 1, 1)]:   # the scale-2 grid is 50 x 20
        with _invalid("frame 0: roi"):
            plan(bad, scale=2)
    plan((49, 19, 1, 1), scale=2).close()
    with _invalid("4:2:2, 4:1:1 or 4:4:0"):
        plan((0, 0, 1, 1), s=hjd.YUV422, scale=2)
    with _invalid("HJD_IN_I32_NATURAL"):
        plan((0, 0, 8, 8), in_fmt=hjd.IN_I32_NATURAL)
    with _invalid("pitch"):
        plan((4, 4, 9, 9), out_pitch=32)       # a 9-px BGRX row needs 36 bytes
    plan((4, 4, 8, 9), out_pitch=32).close()   # 8 px fit, though the frame is 100 px wide
    p = plan((17, 3, 8, 8))
    assert p.has_roi and (p.tasks, p.pixels) == (1, 64)
    with _invalid("variant"):
        p.set_variant(1)
    p.set_variant(0)
    with _invalid("latency"):
        p.set_kernel(hjd.KERNEL_LATENCY)
    p.set_kernel(hjd.KERNEL_PERSISTENT)
    p.set_kernel(hjd.KERNEL_AUTO)
    assert p.launch_shape()["kernel"] == "persistent"   # one task, and no latency kernel
    coefs = torch.zeros((O.frame_blocks(w, h, 1), 64), dtype=torch.int16, device="cuda")
    out = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    with _invalid("ROI"):
        p.launch_stages(4, coefs, out)
    p.close()


# ---- JPEG bytes -> ROI tensors ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _files():
    """q90 PIL files of different sizes: 4:2:0, 4:4:4 and gray, with their coefficients."""
    datas = (_pil(200, 120, 90, 2, seed=21), _pil(131, 77, 90, 0, seed=22), _pil(160, 90, 90, 0, seed=23, gray=True))
    return datas, tuple(_decode_coefs(d) for d in datas)


def _decode_coefs(data):
    import ocljpegdecoder_amd as hjd
    return hjd.decode_coefs(data)


def _expect(decoded, scale, roi=None):
    c, i = decoded
    full = (O.decode_q16(c, i.qt, i.width, i.height, i.sampling) if scale == 1 else
            M.decode_scaled(c, i.qt, i.width, i.height, i.sampling, scale))
    return full if roi is None else _slice(full, roi)


ROIS = {1: [(8, 16, 64, 48), (33, 7, 64, 48), (96, 42, 64, 48)],
        2: [(4, 8, 32, 24), (17, 3, 32, 24), (48, 21, 32, 24)]}


@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_decode_rgb_rois(hjd, ctx, layout):
    import torch
    fmt_name = "OUT_RGB_PLANAR" if layout == "chw" else "OUT_RGB24"
    datas, decoded = _files()
    datas = list(datas)
    assert [i.sampling for _, i in decoded] == [hjd.YUV420, hjd.YUV444, hjd.GRAY]
    with hjd.GpuDecoder(ctx, 3, 2 * sum(map(len, datas)), 2 * sum(i.nblocks for _, i in decoded)) as gd:
        for scale in (1, 2):
            rois = ROIS[scale]
            rw, rh = rois[0][2:]
            exps = [_bytes_of(fmt_name, _expect(d, scale, r)) for d, r in zip(decoded, rois)]
            outs = gd.decode_rgb(datas, layout=layout, scale=scale, rois=rois)
            gd.sync()
            assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX   # restored
            for o, e in zip(outs, exps):
                assert tuple(o.shape) == ((3, rh, rw) if chw_(layout) else (rh, rw, 3))
                np.testing.assert_array_equal(o.cpu().numpy(), e, err_msg=f"scale {scale}")
            batch = torch.full((3,) + exps[0].shape, FILL, dtype=torch.uint8, device="cuda")
            assert gd.decode_rgb(datas, layout=layout, out=batch, scale=scale, rois=rois) is batch
            gd.sync()
            np.testing.assert_array_equal(batch.cpu().numpy(), np.stack(exps), err_msg=f"scale {scale}, out=")
            with pytest.raises(ValueError):
                gd.decode_rgb(datas, layout=layout, out=batch, scale=scale, rois=[rois[0], rois[1], (0, 0, rw, rh - 1)])
            # without rois the call gives whole frames, and still refuses out= for files of different sizes
            outs = gd.decode_rgb(datas, layout=layout, scale=scale)
            gd.sync()
            for o, d in zip(outs, decoded):
                np.testing.assert_array_equal(o.cpu().numpy(), _bytes_of(fmt_name, _expect(d, scale)))
            with pytest.raises(ValueError):
                gd.decode_rgb(datas, layout=layout, out=batch, scale=scale)


def chw_(layout):
    return layout == "chw"


def test_decode_rois_to_bgrx(hjd, ctx):
    import torch
    datas, decoded = _files()
    rois = ROIS[1]
    with hjd.GpuDecoder(ctx, 3, 2 * sum(map(len, datas)), 2 * sum(i.nblocks for _, i in decoded)) as gd:
        outs = [torch.full((r[3], r[2]), -1, dtype=torch.int32, device="cuda") for r in rois]
        gd.decode(list(datas), outs, rois=rois)
        gd.sync()
        for o, d, r in zip(outs, decoded, rois):
            np.testing.assert_array_equal(o.cpu().numpy().view(np.uint32), _expect(d, 1, r))
        from ocljpegdecoder_amd._lib import HjdError
        with pytest.raises(HjdError, match="frame 1: roi") as e:
            gd.decode(list(datas), outs, rois=[rois[0], (100, 7, 64, 48), rois[2]])   # 131 px wide
        assert e.value.code == -1
        gd.decode(list(datas), outs, rois=rois)   # nothing was enqueued; the decoder still works
        gd.sync()
        np.testing.assert_array_equal(outs[1].cpu().numpy().view(np.uint32), _expect(decoded[1], 1, rois[1]))


def test_422_file_with_a_roi(hjd, ctx):
    from ocljpegdecoder_amd._lib import HjdError
    good, f422 = _pil(64, 48, 90, 2, seed=5), _pil(64, 48, 90, 1, seed=6)
    assert hjd.parse(f422).sampling == hjd.YUV422
    rois = [(3, 2, 40, 30), (21, 9, 40, 30)]
    dec = [hjd.decode_coefs(good), hjd.decode_coefs(f422)]
    with hjd.GpuDecoder(ctx, 2, 1 << 16, 1 << 10) as gd:
        outs = gd.decode_rgb([good, f422], rois=rois)
        gd.sync()
        for o, d, r in zip(outs, dec, rois):
            np.testing.assert_array_equal(o.cpu().numpy(), _bytes_of("OUT_RGB_PLANAR", _expect(d, 1, r)))
        with pytest.raises(HjdError, match="scaled decode") as e:
            gd.decode_rgb([good, f422], scale=2, rois=[(0, 0, 8, 8), (0, 0, 8, 8)])
        assert e.value.code == -1 and gd.scale == 1
        outs = gd.decode_rgb([good, f422], rois=rois)   # nothing was enqueued; the decoder still works
        gd.sync()
        np.testing.assert_array_equal(outs[1].cpu().numpy(), _bytes_of("OUT_RGB_PLANAR", _expect(dec[1], 1, rois[1])))


# ---- the C example -------------------------------------------------------------------
def test_c_example_roi_option(hjd):
    """examples/jpeg2bmp --roi x,y,w,h, alone and with --scale 2: a sequential
    file (hjd_gdec_decode_roi) and a progressive one (hjd_plan_create_roi) come
    out as the sliced model's BGRX."""
    import io
    import os
    import subprocess
    import tempfile
    from PIL import Image
    exe = os.path.join(O.REPO, "examples", "jpeg2bmp")
    assert os.access(exe, os.X_OK), "examples/jpeg2bmp not built (run __graft_entry__.build())"
    prog = io.BytesIO()
    Image.fromarray(np.random.default_rng(4).integers(0, 256, (150, 260, 3), dtype=np.uint8)).save(
        prog, format="JPEG", quality=80, subsampling=2, progressive=True)
    files = {"seq_420.jpg": _pil(250, 140, 90, 2, seed=9), "prog_420.jpg": prog.getvalue()}
    roi = (40, 20, 64, 32)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for name, data in files.items():
            open(os.path.join(d, name), "wb").write(data)
            paths.append(os.path.join(d, name))
        for scale in (1, 2):
            args = ["--roi", "40,20,64,32"] + (["--scale", "2"] if scale == 2 else [])
            p = subprocess.run([exe] + args + [d] + paths, capture_output=True, text=True, timeout=100)
            assert p.returncode == 0, p.stdout + p.stderr
            for name, data in files.items():
                raw = open(os.path.join(d, name + ".bmp"), "rb").read()
                assert len(raw) == 54 + 4 * 64 * 32
                got = np.frombuffer(raw[54:], dtype="<u4").reshape(32, 64)
                np.testing.assert_array_equal(got, _expect(hjd.decode_coefs(data), scale, roi), err_msg=f"{name} /{scale}")
        for bad in ("40,20,64", "240,20,64,32", "0,0,0,5"):
            r = subprocess.run([exe, "--roi", bad, d] + paths[:1], capture_output=True, text=True, timeout=100)
            assert r.returncode != 0 and "roi" in r.stderr, (bad, r.stderr)
