"""Scaled decode (1/2, 1/4, 1/8) in the fused kernel: hjd_plan_create_scaled,
Plan(scale=), GpuDecoder.decode_rgb(scale=).  The expectation is always the
numpy model of the definition (tests/scaled_model.py), built from the oracle's
IDCT and colour conversion; equality is exact, and no byte outside a frame's
payload may be written (0xA5-filled buffers with guard bands)."""
import functools

import numpy as np
import pytest

import oracle_py as O
import scaled_model as M
from test_entropy_emulation import _pil

pytestmark = pytest.mark.gpu

FILL = 0xA5
SCALES = [2, 4, 8]
SAMPLINGS = [0, 1, 4]   # HJD_YUV444, HJD_YUV420, HJD_GRAY
FORMATS = ["OUT_BGRX", "OUT_BGR24", "OUT_RGB24", "OUT_RGB_PLANAR"]
ROW_BYTES = {"OUT_BGRX": 4, "OUT_BGR24": 3, "OUT_RGB24": 3, "OUT_RGB_PLANAR": 1}


def _bytes_of(fmt_name, bgrx):
    """(H, W) BGRX words -> the format's payload: (H, W, 4), (H, W, 3) or (3, H, W) bytes."""
    b = np.ascontiguousarray(bgrx).view(np.uint8).reshape(bgrx.shape[0], bgrx.shape[1], 4)
    if fmt_name == "OUT_BGRX":
        return b
    if fmt_name == "OUT_BGR24":
        return np.ascontiguousarray(b[..., :3])
    rgb = np.ascontiguousarray(b[..., [2, 1, 0]])
    return rgb if fmt_name == "OUT_RGB24" else np.ascontiguousarray(rgb.transpose(2, 0, 1))


def _payload_index(fmt_name, w, h, pitch, offset):
    rows = 3 * h if fmt_name == "OUT_RGB_PLANAR" else h
    return offset + np.arange(rows)[:, None] * pitch + np.arange(w * ROW_BYTES[fmt_name])[None, :]


def _extract(fmt_name, full, w, h, pitch, offset):
    px = full[_payload_index(fmt_name, w, h, pitch, offset)]
    return px.reshape(3, h, w) if fmt_name == "OUT_RGB_PLANAR" else px.reshape(h, w, ROW_BYTES[fmt_name])


@functools.lru_cache(maxsize=None)
def _frame(w, h, s):
    coefs, qt = O.synthetic_coefs(w, h, s, seed=w + 7 * h + s)
    for a in (coefs, qt):
        a.setflags(write=False)
    return coefs, qt


@functools.lru_cache(maxsize=None)
def _model(w, h, s, scale):
    """The model's BGRX words of _frame(w, h, s), computed once per shape and scale."""
    coefs, qt = _frame(w, h, s)
    exp = M.decode_scaled(coefs, qt, w, h, s, scale)
    exp.setflags(write=False)
    return exp


def _decode(hjd, ctx, coefs, qt, w, h, s, scale, fmt_name, pad=0, guard=64, in_fmt=0):
    """One frame through a scaled Plan into a 0xA5-filled buffer with guard
    bands; returns the payload and asserts that no other byte was written."""
    import torch
    out_format = getattr(hjd, fmt_name)
    sw, sh = hjd.scaled_size(w, h, scale)
    pitch = hjd.default_pitch(sw, out_format) + pad
    rows = 3 * sh if fmt_name == "OUT_RGB_PLANAR" else sh
    total = guard + rows * pitch + 64
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    spec = hjd.FrameSpec(w, h, s, out_offset=guard, out_pitch=pitch if pad else 0, qt_index=(0, 1, 2),
                         out_format=out_format)
    plan = hjd.Plan(ctx, [spec], in_fmt, qtables=qt, scale=scale)
    assert plan.scale == scale
    assert plan.out_bytes_needed <= total
    assert plan.pixels == sw * sh
    plan.launch(torch.from_numpy(np.array(coefs)).cuda(), buf)
    torch.cuda.synchronize()
    plan.close()
    full = buf.cpu().numpy()
    outside = np.ones(total, bool)
    outside[_payload_index(fmt_name, sw, sh, pitch, guard).ravel()] = False
    assert (full[outside] == FILL).all(), "bytes outside the payload were written"
    return _extract(fmt_name, full, sw, sh, pitch, guard)


# (w, h, pitch pad)
SHAPES = [(1, 1, 0), (17, 9, 0), (129, 17, 0), (256, 32, 0), (385, 33, 0), (388, 33, 12), (769, 16, 0)]


@pytest.mark.parametrize("w,h,pad", SHAPES)
@pytest.mark.parametrize("fmt_name", FORMATS)
@pytest.mark.parametrize("s", SAMPLINGS)
@pytest.mark.parametrize("scale", SCALES)
def test_kernels_vs_model(hjd, ctx, scale, s, fmt_name, w, h, pad):
    coefs, qt = _frame(w, h, s)
    got = _decode(hjd, ctx, coefs, qt, w, h, s, scale, fmt_name, pad=pad)
    np.testing.assert_array_equal(got, _bytes_of(fmt_name, _model(w, h, s, scale)))


@pytest.mark.parametrize("fmt_name", ["OUT_RGB24", "OUT_RGB_PLANAR"])
@pytest.mark.parametrize("s", SAMPLINGS)
@pytest.mark.parametrize("scale", SCALES)
def test_byte_store_path_at_an_odd_offset(hjd, ctx, scale, s, fmt_name):
    w, h = 17, 9
    coefs, qt = _frame(w, h, s)
    got = _decode(hjd, ctx, coefs, qt, w, h, s, scale, fmt_name, guard=61)
    np.testing.assert_array_equal(got, _bytes_of(fmt_name, _model(w, h, s, scale)))


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("scale", SCALES)
def test_clamp_edge_blocks(hjd, ctx, scale, s):
    """The clamp-edge vectors (laid out as test_gpu_parity's
    test_extreme_legal_blocks_q16, all-ones qtables): a box mean of clamped
    samples differs from a clamp of the mean."""
    z = np.load(O.GOLDEN + "/idct_vectors.npz")
    bpm, mw = (6, 16) if s == 1 else (3, 8)
    n = (z["inp"].shape[0] // bpm) * bpm
    nat = np.ascontiguousarray(z["inp"][:n])
    assert np.abs(nat).max() < 32768
    coefs = np.ascontiguousarray(nat[:, O.ZIGZAG].astype(np.int16))   # natural -> zigzag, q = 1
    qt = np.ones((3, 64), np.int32)
    w, h = mw * (n // bpm), mw
    got = _decode(hjd, ctx, coefs, qt, w, h, s, scale, "OUT_BGRX")
    np.testing.assert_array_equal(got, _bytes_of("OUT_BGRX", M.decode_scaled(coefs, qt, w, h, s, scale)))


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("scale", SCALES)
def test_g_flag_chroma_pairs(hjd, ctx, scale, s):
    """(U, V) = (-200, 200) and (-100, 100), the two chroma pairs whose G term
    takes the kernel's corrected path, with Y + 128 running over 180..210
    (across the reference's rounding corner at (-200, 200)).  q = 1, DC-only
    blocks: by the reference's DC short-cut every sample is (dc + 4) >> 3."""
    w, h = 96, 32
    pw, _, bpm, _ = O.GEOM[s]
    n = O.frame_blocks(w, h, s)
    mw = w // pw
    comp = O.block_components(s, n)
    mx = (np.arange(n) // bpm) % mw
    left = mx < mw // 2
    coefs = np.zeros((n, 64), np.int16)
    luma = np.flatnonzero(comp == 0)
    coefs[luma, 0] = 8 * (52 + np.arange(luma.size) % 31)          # Y + 128 = 180..210
    coefs[comp == 1, 0] = np.where(left, -1600, -800)[comp == 1]   # U = -200 | -100
    coefs[comp == 2, 0] = np.where(left, 1600, 800)[comp == 2]     # V = 200 | 100
    qt = np.ones((3, 64), np.int32)
    y, u, v = M.scaled_planes(coefs, qt, w, h, s, scale)
    assert ((u == -200) & (v == 200)).any() and ((u == -100) & (v == 100)).any()
    assert y.min() == 52 and y.max() == 82
    got = _decode(hjd, ctx, coefs, qt, w, h, s, scale, "OUT_BGRX")
    np.testing.assert_array_equal(got, _bytes_of("OUT_BGRX", M.decode_scaled(coefs, qt, w, h, s, scale)))


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("scale", SCALES)
def test_mixed_batch_in_one_plan(hjd, ctx, scale, s):
    """Three frames of different sizes at distinct offsets of one buffer, one
    and sixteen tasks per wave (waves cross frame boundaries): each equals the
    model and nothing between them is written."""
    import torch
    fmt_name = "OUT_RGB_PLANAR"
    sizes = [(388, 33), (17, 9), (256, 32)]
    specs, coefs_all, off, blk = [], [], 128, 0
    qt = None
    for w, h in sizes:
        coefs, qt = _frame(w, h, s)
        sw, sh = hjd.scaled_size(w, h, scale)
        specs.append(hjd.FrameSpec(w, h, s, coef_offset=blk, out_offset=off, qt_index=(0, 1, 2),
                                   out_format=hjd.OUT_RGB_PLANAR))
        coefs_all.append(coefs)
        blk += coefs.shape[0]
        off += 3 * sw * sh + 100   # a gap the kernel must leave alone
    total = off + 64
    d_coefs = torch.from_numpy(np.concatenate(coefs_all)).cuda()
    plan = hjd.Plan(ctx, specs, hjd.IN_Q16_ZIGZAG, qtables=qt, scale=scale)
    assert plan.out_bytes_needed <= total
    for chunk in (1, 16):
        plan.set_chunk(chunk)
        assert plan.launch_shape()["kernel"] == "persistent"
        buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        plan.launch(d_coefs, buf)
        torch.cuda.synchronize()
        full = buf.cpu().numpy()
        inside = np.zeros(total, bool)
        for sp, (w, h) in zip(specs, sizes):
            sw, sh = hjd.scaled_size(w, h, scale)
            inside[_payload_index(fmt_name, sw, sh, sw, sp.out_offset).ravel()] = True
            np.testing.assert_array_equal(_extract(fmt_name, full, sw, sh, sw, sp.out_offset),
                                          _bytes_of(fmt_name, _model(w, h, s, scale)), err_msg=f"{w}x{h} chunk {chunk}")
        assert (full[~inside] == FILL).all()
    plan.close()


@pytest.mark.parametrize("fmt_name", FORMATS)
def test_scale_1_is_the_full_size_decode(hjd, ctx, fmt_name):
    import torch
    w, h, s = 388, 33, 1
    coefs, qt = _frame(w, h, s)
    out_format = getattr(hjd, fmt_name)
    d = torch.from_numpy(np.array(coefs)).cuda()
    outs = []
    for kw in ({}, {"scale": 1}):
        plan = hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_format=out_format)], 0, qtables=qt, **kw)
        assert plan.scale == 1
        buf = torch.full((plan.out_bytes_needed + 64,), FILL, dtype=torch.uint8, device="cuda")
        plan.launch(d, buf)
        torch.cuda.synchronize()
        plan.close()
        outs.append(buf.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    pitch = hjd.default_pitch(w, out_format)
    np.testing.assert_array_equal(_extract(fmt_name, outs[1], w, h, pitch, 0),
                                  _bytes_of(fmt_name, O.decode_q16(coefs, qt, w, h, s)))


def test_autotune_and_chunk_on_a_scaled_plan(hjd, ctx):
    import torch
    w, h, s, scale = 388, 33, 1, 4
    coefs, qt = _frame(w, h, s)
    sw, sh = hjd.scaled_size(w, h, scale)
    out = torch.full((3, sh, sw), FILL, dtype=torch.uint8, device="cuda")
    p = hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_format=hjd.OUT_RGB_PLANAR)], 0, qtables=qt,
                 scale=scale)
    d = torch.from_numpy(np.array(coefs)).cuda()
    hjd.autotune_cache_clear()
    tpw, variant = p.autotune(d, out, rounds=1)
    assert variant == 0 and tpw >= 1 and p.launch_shape()["autotune_launches"] > 0
    # the cache key holds the scale: a full-size plan of the same frame does not take this choice
    p1 = hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_format=hjd.OUT_RGB_PLANAR)], 0, qtables=qt)
    p1.set_kernel(hjd.KERNEL_PERSISTENT)
    out1 = torch.empty((3, h, w), dtype=torch.uint8, device="cuda")
    p1.autotune(d, out1, rounds=1)
    assert p1.launch_shape()["autotune_cached"] == 0
    p1.close()
    out.fill_(FILL)
    p.launch(d, out)
    torch.cuda.synchronize()
    p.close()
    np.testing.assert_array_equal(out.cpu().numpy(), _bytes_of("OUT_RGB_PLANAR", _model(w, h, s, scale)))


# ---- refusals -------------------------------------------------------------------
class _invalid:
    """The body must raise HjdError with status HJD_E_INVALID (-1) and a message naming the cause."""

    def __init__(self, match):
        from ocljpegdecoder_amd._lib import HjdError
        self.cm = pytest.raises(HjdError, match=match)

    def __enter__(self):
        self.info = self.cm.__enter__()

    def __exit__(self, *exc):
        r = self.cm.__exit__(*exc)
        assert self.info.value.code == -1, self.info.value
        return r


def test_refusals(hjd, ctx):
    import torch
    w, h = 17, 9
    qt = O.std_qtables()

    def plan(s=1, in_fmt=0, scale=2, **kw):
        return hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), **kw)], in_fmt,
                        qtables=qt if in_fmt == 0 else None, scale=scale)

    for bad in (0, 3, 16, -1):
        with _invalid("scale"):
            plan(scale=bad)
    for s in (hjd.YUV422, hjd.YUV411_H4V1, hjd.YUV440):
        with _invalid("4:2:2, 4:1:1 or 4:4:0"):
            plan(s=s)
        plan(s=s, scale=1).close()   # full size still serves them
    with _invalid("HJD_IN_I32_NATURAL"):
        plan(in_fmt=hjd.IN_I32_NATURAL)
    with _invalid("pitch"):
        plan(out_pitch=4 * 8)        # W' = 9 needs 36 bytes
    p = plan()
    assert (p.scale, p.pixels) == (2, 9 * 5)
    with _invalid("variant"):
        p.set_variant(1)
    p.set_variant(0)
    with _invalid("latency"):
        p.set_kernel(hjd.KERNEL_LATENCY)
    p.set_kernel(hjd.KERNEL_PERSISTENT)
    p.set_kernel(hjd.KERNEL_AUTO)
    assert p.launch_shape()["kernel"] == "persistent"   # however few tasks
    coefs = torch.zeros((O.frame_blocks(w, h, 1), 64), dtype=torch.int16, device="cuda")
    out = torch.zeros((5, 9), dtype=torch.int32, device="cuda")
    with _invalid("scaled"):
        p.launch_stages(4, coefs, out)
    p.close()
    with hjd.GpuDecoder(ctx, 1, 1 << 16, 1 << 10) as gd:
        with _invalid("scale"):
            gd.set_scale(3)
        assert gd.scale == 1


# ---- JPEG bytes -> scaled RGB tensors ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _jpegs(w, h):
    """q90 PIL files of one size: 4:2:0, 4:4:4 and L."""
    return (_pil(w, h, 90, 2, seed=w), _pil(w, h, 90, 0, seed=w + 1), _pil(w, h, 90, 0, seed=w + 2, gray=True))


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("w,h", [(200, 120), (131, 77)])
def test_decode_rgb_scaled(hjd, ctx, w, h, layout):
    import torch
    fmt_name = "OUT_RGB_PLANAR" if layout == "chw" else "OUT_RGB24"
    datas = list(_jpegs(w, h))
    decoded = [hjd.decode_coefs(d) for d in datas]
    assert [i.sampling for _, i in decoded] == [hjd.YUV420, hjd.YUV444, hjd.GRAY]
    with hjd.GpuDecoder(ctx, len(datas), 2 * sum(map(len, datas)), 2 * sum(i.nblocks for _, i in decoded)) as gd:
        for scale in SCALES:
            sw, sh = hjd.scaled_size(w, h, scale)
            exps = [_bytes_of(fmt_name, M.decode_scaled(c, i.qt, w, h, i.sampling, scale)) for c, i in decoded]
            outs = gd.decode_rgb(datas, layout=layout, scale=scale)
            gd.sync()
            assert gd.scale == 1   # restored
            for o, e in zip(outs, exps):
                assert o.dtype == torch.uint8 and tuple(o.shape) == ((3, sh, sw) if layout == "chw" else (sh, sw, 3))
                np.testing.assert_array_equal(o.cpu().numpy(), e, err_msg=f"scale {scale}")
            batch = torch.full((len(datas),) + exps[0].shape, FILL, dtype=torch.uint8, device="cuda")
            assert gd.decode_rgb(datas, layout=layout, out=batch, scale=scale) is batch
            gd.sync()
            np.testing.assert_array_equal(batch.cpu().numpy(), np.stack(exps), err_msg=f"scale {scale}, out=")
            with pytest.raises(ValueError):
                gd.decode_rgb(datas, layout=layout, out=batch, scale=1)   # out has the scaled size
        # the decoder carries no scale over: a scale-1 decode is the oracle's
        outs = gd.decode_rgb(datas, layout=layout)
        gd.sync()
        for o, (c, i) in zip(outs, decoded):
            np.testing.assert_array_equal(o.cpu().numpy(),
                                          _bytes_of(fmt_name, O.decode_q16(c, i.qt, w, h, i.sampling)))


def test_decode_rgb_scaled_refuses_422(hjd, ctx):
    from ocljpegdecoder_amd._lib import HjdError
    good, bad = _pil(64, 48, 90, 2, seed=5), _pil(64, 48, 90, 1, seed=6)
    assert hjd.parse(bad).sampling == hjd.YUV422
    with hjd.GpuDecoder(ctx, 2, 1 << 16, 1 << 10) as gd:
        with pytest.raises(HjdError, match="scaled decode") as e:
            gd.decode_rgb([good, bad], scale=2)
        assert e.value.code == -1
        assert gd.scale == 1
        outs = gd.decode_rgb([good, bad])   # nothing was enqueued; the decoder still works
        gd.sync()
        c, i = hjd.decode_coefs(bad)
        np.testing.assert_array_equal(outs[1].cpu().numpy(),
                                      _bytes_of("OUT_RGB_PLANAR", O.decode_q16(c, i.qt, 64, 48, i.sampling)))


# ---- the C example ---------------------------------------------------------------
def test_c_example_scale_option(hjd):
    """examples/jpeg2bmp --scale N: a sequential file (hjd_gdec_set_scale) and a
    progressive one (hjd_plan_create_scaled) come out as the model's BGRX."""
    import io
    import os
    import subprocess
    import tempfile
    from PIL import Image
    exe = os.path.join(O.REPO, "examples", "jpeg2bmp")
    assert os.access(exe, os.X_OK), "examples/jpeg2bmp not built (run __graft_entry__.build())"
    prog = io.BytesIO()
    Image.fromarray(np.random.default_rng(4).integers(0, 256, (77, 133, 3), dtype=np.uint8)).save(
        prog, format="JPEG", quality=80, subsampling=2, progressive=True)
    files = {"seq_420.jpg": _pil(131, 77, 90, 2, seed=9), "prog_420.jpg": prog.getvalue()}
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for name, data in files.items():
            open(os.path.join(d, name), "wb").write(data)
            paths.append(os.path.join(d, name))
        p = subprocess.run([exe, "--scale", "4", d] + paths, capture_output=True, text=True, timeout=100)
        assert p.returncode == 0, p.stdout + p.stderr
        for name, data in files.items():
            coefs, info = hjd.decode_coefs(data)
            sw, sh = hjd.scaled_size(info.width, info.height, 4)
            raw = open(os.path.join(d, name + ".bmp"), "rb").read()
            assert len(raw) == 54 + 4 * sw * sh
            got = np.frombuffer(raw[54:], dtype="<u4").reshape(sh, sw)
            np.testing.assert_array_equal(got, M.decode_scaled(coefs, info.qt, info.width, info.height, info.sampling, 4),
                                          err_msg=name)
        bad = subprocess.run([exe, "--scale", "3", d] + paths[:1], capture_output=True, text=True, timeout=100)
        assert bad.returncode != 0 and "scale" in bad.stderr
