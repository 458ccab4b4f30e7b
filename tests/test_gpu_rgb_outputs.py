"""HJD_OUT_RGB24 (H, W, 3) and HJD_OUT_RGB_PLANAR (3, H, W) outputs of the fused
kernel.  The expectation is always the oracle's BGRX words (O.decode_q16, or
the golden files' stored bgrx) permuted in numpy; equality is exact."""
import functools
import os

import numpy as np
import pytest

import oracle_py as O
from test_entropy_emulation import _pil

pytestmark = pytest.mark.gpu

SAMPLINGS = [0, 1, 3, 4, 5, 6]
FILL = 0xA5


def _hwc(bgrx):
    """(H, W) BGRX words -> (H, W, 3) bytes R, G, B."""
    b = np.ascontiguousarray(bgrx).view(np.uint8).reshape(bgrx.shape[0], bgrx.shape[1], 4)
    return np.ascontiguousarray(b[..., [2, 1, 0]])


def _chw(bgrx):
    """(H, W) BGRX words -> (3, H, W) bytes: planes R, G, B."""
    return np.ascontiguousarray(_hwc(bgrx).transpose(2, 0, 1))


def _expect(hjd, out_format, bgrx):
    return _chw(bgrx) if out_format == hjd.OUT_RGB_PLANAR else _hwc(bgrx)


@functools.lru_cache(maxsize=None)
def _frame(w, h, s):
    """Synthetic coefficients and the oracle's pixels, computed once per shape."""
    coefs, qt = O.synthetic_coefs(w, h, s, seed=w + 7 * h + s)
    exp = O.decode_q16(coefs, qt, w, h, s)
    for a in (coefs, qt, exp):
        a.setflags(write=False)
    return coefs, qt, exp


def _payload_mask(hjd, total, out_format, w, h, pitch, offset):
    """True where a frame's payload bytes lie in a buffer of `total` bytes."""
    m = np.zeros(total, bool)
    rows = 3 * h if out_format == hjd.OUT_RGB_PLANAR else h
    rb = w if out_format == hjd.OUT_RGB_PLANAR else 3 * w
    idx = offset + np.arange(rows)[:, None] * pitch + np.arange(rb)[None, :]
    m[idx.ravel()] = True
    return m


def _extract(hjd, full, out_format, w, h, pitch, offset):
    rows = 3 * h if out_format == hjd.OUT_RGB_PLANAR else h
    rb = w if out_format == hjd.OUT_RGB_PLANAR else 3 * w
    idx = offset + np.arange(rows)[:, None] * pitch + np.arange(rb)[None, :]
    px = full[idx]
    return px.reshape(3, h, w) if out_format == hjd.OUT_RGB_PLANAR else px.reshape(h, w, 3)


def _decode(hjd, ctx, coefs, qt, w, h, s, out_format, pitch, guard=64, in_fmt=0, kernel=None):
    """One frame through a Plan into a 0xA5-filled buffer with guard bands;
    returns the payload and asserts that no other byte was written."""
    import torch
    rows = 3 * h if out_format == hjd.OUT_RGB_PLANAR else h
    total = guard + rows * pitch + 64
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    spec = hjd.FrameSpec(w, h, s, out_offset=guard, out_pitch=pitch, qt_index=(0, 1, 2), out_format=out_format)
    plan = hjd.Plan(ctx, [spec], in_fmt, qtables=qt if in_fmt == 0 else None)
    assert plan.out_bytes_needed <= total
    if kernel is not None:
        plan.set_kernel(kernel)
    plan.launch(torch.from_numpy(np.array(coefs)).cuda(), buf)
    torch.cuda.synchronize()
    plan.close()
    full = buf.cpu().numpy()
    outside = ~_payload_mask(hjd, total, out_format, w, h, pitch, guard)
    assert (full[outside] == FILL).all(), "bytes outside the payload were written"
    return _extract(hjd, full, out_format, w, h, pitch, guard)


# (w, h, pitch pad, guard): guard 61 puts the byte path at an odd out_offset
SHAPES = [(1, 1, 0, 64), (17, 9, 0, 61), (385, 16, 0, 64), (388, 33, 0, 64), (388, 33, 12, 64), (768, 16, 0, 64),
          (768, 16, 12, 64)]


@pytest.mark.parametrize("w,h,pad,guard", SHAPES)
@pytest.mark.parametrize("s", SAMPLINGS)
@pytest.mark.parametrize("fmt_name", ["OUT_RGB24", "OUT_RGB_PLANAR"])
def test_kernels_vs_oracle(hjd, ctx, fmt_name, s, w, h, pad, guard):
    out_format = getattr(hjd, fmt_name)
    coefs, qt, bgrx = _frame(w, h, s)
    pitch = hjd.default_pitch(w, out_format) + pad
    exp = _expect(hjd, out_format, bgrx)
    for kernel in (hjd.KERNEL_LATENCY, hjd.KERNEL_PERSISTENT):
        got = _decode(hjd, ctx, coefs, qt, w, h, s, out_format, pitch, guard=guard, kernel=kernel)
        np.testing.assert_array_equal(got, exp, err_msg=f"kernel mode {kernel}")


@pytest.mark.parametrize("fmt_name", ["OUT_RGB24", "OUT_RGB_PLANAR"])
def test_i32_natural_input_on_golden_cases(hjd, ctx, fmt_name):
    out_format = getattr(hjd, fmt_name)
    for name in O.golden_cases():
        c = O.load_case(name)
        w, h, s = int(c["width"]), int(c["height"]), int(c["sampling"])
        nat = O.dequant_natural(c["coefs_q16"], c["qt"], s)
        got = _decode(hjd, ctx, nat, None, w, h, s, out_format, hjd.default_pitch(w, out_format), in_fmt=1)
        np.testing.assert_array_equal(got, _expect(hjd, out_format, c["bgrx"]), err_msg=name)


def test_planar_batch_in_one_plan(hjd, ctx):
    """Three frames of different sizes (one at an unaligned pitch) at distinct
    offsets of one buffer, persistent kernel: each equals the oracle and
    nothing between them is written."""
    import torch
    s = 1
    sizes = [(388, 33), (131, 20), (768, 16)]
    specs, coefs_all, off, blk = [], [], 128, 0
    qt = None
    for w, h in sizes:
        coefs, qt, _ = _frame(w, h, s)
        specs.append(hjd.FrameSpec(w, h, s, coef_offset=blk, out_offset=off, out_pitch=w, qt_index=(0, 1, 2),
                                   out_format=hjd.OUT_RGB_PLANAR))
        coefs_all.append(coefs)
        blk += coefs.shape[0]
        off += 3 * w * h + 100   # a gap the kernel must leave alone
    total = off + 64
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    plan = hjd.Plan(ctx, specs, hjd.IN_Q16_ZIGZAG, qtables=qt)
    plan.set_kernel(hjd.KERNEL_PERSISTENT)
    plan.launch(torch.from_numpy(np.concatenate(coefs_all)).cuda(), buf)
    torch.cuda.synchronize()
    plan.close()
    full = buf.cpu().numpy()
    inside = np.zeros(total, bool)
    for sp, (w, h) in zip(specs, sizes):
        inside |= _payload_mask(hjd, total, hjd.OUT_RGB_PLANAR, w, h, w, sp.out_offset)
        np.testing.assert_array_equal(_extract(hjd, full, hjd.OUT_RGB_PLANAR, w, h, w, sp.out_offset),
                                      _chw(_frame(w, h, s)[2]), err_msg=f"{w}x{h}")
    assert (full[~inside] == FILL).all()


def test_planar_equal_frames_form_nchw(hjd, ctx):
    import torch
    w, h = 388, 33
    frames = [(_frame(w, h, 0)), O.synthetic_coefs(w, h, 0, seed=99)]
    exp1 = O.decode_q16(frames[1][0], frames[1][1], w, h, 0)
    nb = frames[0][0].shape[0]
    qts = np.concatenate([frames[0][1], frames[1][1]])
    specs = [hjd.FrameSpec(w, h, 0, coef_offset=k * nb, out_offset=k * 3 * w * h, out_pitch=w,
                           qt_index=(3 * k, 3 * k + 1, 3 * k + 2), out_format=hjd.OUT_RGB_PLANAR) for k in range(2)]
    out = torch.full((2, 3, h, w), FILL, dtype=torch.uint8, device="cuda")
    plan = hjd.Plan(ctx, specs, hjd.IN_Q16_ZIGZAG, qtables=qts)
    plan.set_kernel(hjd.KERNEL_PERSISTENT)
    assert plan.out_bytes_needed == out.numel()
    plan.launch(torch.from_numpy(np.concatenate([frames[0][0], frames[1][0]])).cuda(), out)
    torch.cuda.synchronize()
    plan.close()
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([_chw(frames[0][2]), _chw(exp1)]))


@pytest.mark.parametrize("w,h", [(17, 9), (388, 33)])
def test_gray_planes_are_identical(hjd, ctx, w, h):
    coefs, qt, bgrx = _frame(w, h, 4)
    got = _decode(hjd, ctx, coefs, qt, w, h, 4, hjd.OUT_RGB_PLANAR, w, kernel=hjd.KERNEL_PERSISTENT)
    b = (bgrx & 0xFF).astype(np.uint8)
    for c in range(3):
        np.testing.assert_array_equal(got[c], b)


# ---- JPEG entry points --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _jpegs():
    golden = open(os.path.join(O.GOLDEN, "JPEG_example_JPG_RIP_050.jpg"), "rb").read()
    return (golden, _pil(333, 77, 85, 1, seed=41), _pil(200, 120, 80, 0, seed=42, gray=True))


@pytest.fixture(scope="module")
def jpeg_cases(hjd, ctx):
    """(data, info, BGRX words of decode_jpeg) per file."""
    out = []
    for d in _jpegs():
        info = hjd.parse(d)
        bgrx = hjd.decode_jpeg(ctx, d).cpu().numpy().view(np.uint32)
        bgrx.setflags(write=False)
        out.append((d, info, bgrx))
    assert [i.sampling for _, i, _ in out] == [hjd.YUV420, hjd.YUV422, hjd.GRAY]
    return out


def _shape(hjd, out_format, info):
    return (3, info.height, info.width) if out_format == hjd.OUT_RGB_PLANAR else (info.height, info.width, 3)


@pytest.mark.parametrize("fmt_name", ["OUT_RGB24", "OUT_RGB_PLANAR"])
def test_decode_jpeg_and_gpu_decoder(hjd, ctx, jpeg_cases, fmt_name):
    import torch
    out_format = getattr(hjd, fmt_name)
    datas = [d for d, _, _ in jpeg_cases]
    infos = [i for _, i, _ in jpeg_cases]
    for d, info, bgrx in jpeg_cases:
        out = hjd.decode_jpeg(ctx, d, out_format=out_format)
        assert out.dtype == torch.uint8 and tuple(out.shape) == _shape(hjd, out_format, info)
        assert out.is_contiguous()
        np.testing.assert_array_equal(out.cpu().numpy(), _expect(hjd, out_format, bgrx))
    outs = [torch.full(_shape(hjd, out_format, i), FILL, dtype=torch.uint8, device="cuda") for i in infos]
    with hjd.GpuDecoder(ctx, len(datas), sum(map(len, datas)), sum(i.nblocks for i in infos)) as gd:
        gd.set_output_format(out_format)
        gd.decode(datas, outs)
        gd.sync()
    for o, (_, _, bgrx) in zip(outs, jpeg_cases):
        np.testing.assert_array_equal(o.cpu().numpy(), _expect(hjd, out_format, bgrx))


@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_decode_rgb(hjd, ctx, jpeg_cases, layout):
    import torch
    out_format = hjd.OUT_RGB_PLANAR if layout == "chw" else hjd.OUT_RGB24
    datas = [d for d, _, _ in jpeg_cases]
    infos = [i for _, i, _ in jpeg_cases]
    with hjd.GpuDecoder(ctx, len(datas), 2 * sum(map(len, datas)), 2 * sum(i.nblocks for i in infos)) as gd:
        gd.set_output_format(hjd.OUT_BGR24)
        outs = gd.decode_rgb(datas, layout=layout)
        gd.sync()
        assert gd.out_format == hjd.OUT_BGR24   # restored
        assert isinstance(outs, list) and len(outs) == len(datas)
        for o, (_, info, bgrx) in zip(outs, jpeg_cases):
            assert o.dtype == torch.uint8 and tuple(o.shape) == _shape(hjd, out_format, info)
            np.testing.assert_array_equal(o.cpu().numpy(), _expect(hjd, out_format, bgrx))
        # two files of one size into a preallocated batch tensor
        pair = [_pil(150, 70, 90, 2, seed=51), _pil(150, 70, 85, 2, seed=52)]
        exps = [_expect(hjd, out_format, hjd.decode_jpeg(ctx, d).cpu().numpy().view(np.uint32)) for d in pair]
        batch = torch.full((2,) + exps[0].shape, FILL, dtype=torch.uint8, device="cuda")
        ret = gd.decode_rgb(pair, layout=layout, out=batch)
        gd.sync()
        assert ret is batch
        np.testing.assert_array_equal(batch.cpu().numpy(), np.stack(exps))
        with pytest.raises(ValueError):
            gd.decode_rgb([pair[0], datas[1]], layout=layout, out=batch)   # a size that differs from out
        with pytest.raises(ValueError):
            gd.decode_rgb(pair, layout="nchw")
        assert gd.out_format == hjd.OUT_BGR24


@pytest.mark.parametrize("fmt_name", ["OUT_RGB24", "OUT_RGB_PLANAR"])
def test_streams(hjd, ctx, jpeg_cases, fmt_name):
    """GpuJpegStream to device tensors and to host numpy arrays (D2H sink),
    and the host-Huffman JpegStream."""
    import torch
    out_format = getattr(hjd, fmt_name)
    datas = [d for d, _, _ in jpeg_cases]
    infos = [i for _, i, _ in jpeg_cases]
    dev = [torch.full(_shape(hjd, out_format, i), FILL, dtype=torch.uint8, device="cuda") for i in infos]
    host = [np.full(_shape(hjd, out_format, i), FILL, np.uint8) for i in infos]
    with hjd.GpuJpegStream(ctx, max_frames=4, max_scan_bytes=2 * sum(map(len, datas)),
                           max_blocks=2 * sum(i.nblocks for i in infos), out_format=out_format) as gs:
        for d, o, ho in zip(datas, dev, host):
            gs.submit(d, o)
            gs.submit(d, ho)
        gs.sync()
    for o, ho, (_, _, bgrx) in zip(dev, host, jpeg_cases):
        np.testing.assert_array_equal(o.cpu().numpy(), _expect(hjd, out_format, bgrx))
        np.testing.assert_array_equal(ho, _expect(hjd, out_format, bgrx))
    outs = [torch.full(_shape(hjd, out_format, i), FILL, dtype=torch.uint8, device="cuda") for i in infos]
    with hjd.JpegStream(ctx, max(i.nblocks for i in infos), nslots=2, nthreads=2, out_format=out_format) as st:
        for d, o in zip(datas, outs):
            st.submit(d, o)
        st.sync()
    for o, (_, _, bgrx) in zip(outs, jpeg_cases):
        np.testing.assert_array_equal(o.cpu().numpy(), _expect(hjd, out_format, bgrx))


# ---- misuse -------------------------------------------------------------------
class _invalid:
    """The body must raise the library's error with status HJD_E_INVALID (-1)."""

    def __init__(self, match):
        self.cm = pytest.raises(Exception, match=match)

    def __enter__(self):
        self.info = self.cm.__enter__()

    def __exit__(self, *exc):
        r = self.cm.__exit__(*exc)
        assert getattr(self.info.value, "code", None) == -1, self.info.value
        return r


def test_misuse_is_rejected(hjd, ctx):
    w, h, s = 17, 9, 1
    _, qt, _ = _frame(w, h, s)

    def plan(**kw):
        return hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), **kw)], hjd.IN_Q16_ZIGZAG, qtables=qt)

    with _invalid("pitch"):
        plan(out_format=hjd.OUT_RGB_PLANAR, out_pitch=w - 1)
    with _invalid("pitch"):
        plan(out_format=hjd.OUT_RGB24, out_pitch=3 * w - 1)
    with _invalid("output format"):
        f = hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_pitch=4 * w, out_format=4).to_c()
        import ctypes
        hp = ctypes.c_void_p()
        from ocljpegdecoder_amd._lib import HjdFrame, check, c_i32p
        q = np.ascontiguousarray(qt, np.int32)
        check(ctx.lib.hjd_plan_create(ctx.handle, (HjdFrame * 1)(f), 1, 0, q.ctypes.data_as(c_i32p), 3,
                                      ctypes.byref(hp)), "hjd_plan_create")
    with _invalid("mixed output formats"):
        hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_format=hjd.OUT_RGB24),
                       hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_offset=4096, out_format=hjd.OUT_RGB_PLANAR)],
                 hjd.IN_Q16_ZIGZAG, qtables=qt)
    for fmt in (hjd.OUT_RGB24, hjd.OUT_RGB_PLANAR):
        p = plan(out_format=fmt)
        with _invalid("BGRX-only"):
            p.set_variant(1)
        p.close()
    # existing behaviour kept: a BGR24 pitch that is not a multiple of 4 is still refused
    with _invalid("pitch"):
        plan(out_format=hjd.OUT_BGR24, out_pitch=3 * w + 3)
    with hjd.GpuDecoder(ctx, 1, 1 << 16, 1 << 10) as gd:
        with _invalid("output format"):
            gd.set_output_format(4)


def test_autotune_on_a_planar_plan(hjd, ctx):
    import torch
    w, h, s = 388, 33, 1
    coefs, qt, bgrx = _frame(w, h, s)
    out = torch.full((3, h, w), FILL, dtype=torch.uint8, device="cuda")
    p = hjd.Plan(ctx, [hjd.FrameSpec(w, h, s, qt_index=(0, 1, 2), out_format=hjd.OUT_RGB_PLANAR)],
                 hjd.IN_Q16_ZIGZAG, qtables=qt)
    p.set_kernel(hjd.KERNEL_PERSISTENT)
    d = torch.from_numpy(np.array(coefs)).cuda()
    tpw, variant = p.autotune(d, out, rounds=1)
    assert variant == 0 and tpw >= 1
    out.fill_(FILL)
    p.launch(d, out)
    torch.cuda.synchronize()
    p.close()
    np.testing.assert_array_equal(out.cpu().numpy(), _chw(bgrx))
