"""The antialiased resize on the GPU: Resize(antialias=True) alone on seeded
random planes, and GpuDecoder.decode_rgb_resized(antialias=True) from JPEG
bytes.  The expectation is tests/resize_aa_model.py, the numpy model of the
definition in include/hjd.h; payloads are compared bit for bit (the float
planes on their bit patterns), no byte outside a payload may be written
(0xA5-filled buffers with guard bands and pitch padding), and the sources must
come back unchanged."""
import functools

import numpy as np
import pytest

import norm_model as N
import resize_aa_model as A
import resize_model as R
from test_entropy_emulation import _pil

pytestmark = pytest.mark.gpu

FILL = 0xA5
DTYPES = ["uint8", "float16", "float32"]
BITS = {"uint8": np.uint8, "float16": np.uint16, "float32": np.uint32}
# not ImageNet's: every channel its own, none trivial
MEAN, STD = (0.31, 0.52, 0.47), (0.27, 0.19, 0.33)

# (w, h) -> (wo, ho), destination row padding in elements, guard bytes in front
CASES = {
    "vector_stores": ((37, 29), (24, 16), 0, 64),
    "guarded_stores_odd_offset_and_pitch": ((37, 29), (23, 15), 3, 61),
    "one_axis_only": ((9, 200), (9, 3), 0, 64),
    "enlargement": ((17, 33), (50, 40), 0, 64),
    "about_800_taps": ((64, 1000), (8, 5), 0, 64),
    "to_one_pixel": ((300, 7), (1, 1), 0, 64),
    "from_one_pixel": ((1, 1), (3, 3), 0, 64),
    "threads_loop": ((40, 30), (1024, 300), 0, 64),   # 76800 quads against 256 groups x 256 threads
}


@functools.lru_cache(maxsize=None)
def _norm():
    import ocljpegdecoder_amd as hjd
    a, b = hjd.norm_constants(MEAN, STD)
    return tuple(float(v) for v in a), tuple(float(v) for v in b)


@functools.lru_cache(maxsize=None)
def _src(w, h):
    a = np.random.default_rng(1000 * w + h).integers(0, 256, (3, h, w), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _model_u8(w, h, wo, ho, flip):
    a = A.resize_u8(_src(w, h), wo, ho, flip)
    a.setflags(write=False)
    return a


def _expect(w, h, wo, ho, flip, dtype):
    u8 = _model_u8(w, h, wo, ho, bool(flip))
    return u8 if dtype == "uint8" else N.apply(u8, _norm()[0], _norm()[1], np.dtype(dtype))


def _guard_of(dtype, guard):
    """Guard bytes in front: as asked for bytes, rounded down to the element size for floats (still no multiple of 16)."""
    return guard - guard % np.dtype(dtype).itemsize


def _resize_aa(hjd, ctx, shapes, wo, ho, dtype, flips=None, row_pad=0, guard=64, src_offset=61, src_pad=3):
    """One Resize(antialias=True) over `shapes` -> (N, 3, ho, wo) inside a
    0xA5-filled buffer; returns the payload's bit patterns, having asserted
    that no other byte was written and that the sources are unchanged."""
    import torch
    n, elem = len(shapes), np.dtype(dtype).itemsize
    guard = _guard_of(dtype, guard)
    p = wo + row_pad
    nbytes = n * 3 * ho * p * elem
    total = guard + nbytes + 64
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[guard:guard + nbytes].view(getattr(torch, dtype)).view(n, 3, ho, p)[..., :wo]
    srcs, bufs, hosts = [], [], []
    for w, h in shapes:   # each source at an odd address, rows w + src_pad bytes apart
        sp = w + src_pad
        host = np.full(src_offset + 3 * h * sp + 64, 0x3C, np.uint8)
        host[src_offset:src_offset + 3 * h * sp].reshape(3, h, sp)[..., :w] = _src(w, h)
        b = torch.from_numpy(host).cuda()
        hosts.append(host)
        bufs.append(b)
        srcs.append(b[src_offset:src_offset + 3 * h * sp].view(3, h, sp)[..., :w])
    r = hjd.Resize(ctx, srcs, out, flips=flips, normalize=_norm() if dtype != "uint8" else None, antialias=True)
    assert r.filter == hjd.RESIZE_TRIANGLE_AA
    r.launch()
    torch.cuda.synchronize()
    r.close()
    for b, host in zip(bufs, hosts):
        np.testing.assert_array_equal(b.cpu().numpy(), host, err_msg="a source buffer was written")
    full = buf.cpu().numpy()
    idx = guard + np.arange(n * 3 * ho)[:, None] * (p * elem) + np.arange(wo * elem)[None, :]
    outside = np.ones(total, bool)
    outside[idx.ravel()] = False
    assert (full[outside] == FILL).all(), "bytes outside the payload were written"
    return np.ascontiguousarray(full[idx]).view(BITS[dtype]).reshape(n, 3, ho, wo)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_each_case_alone(hjd, ctx, case, dtype):
    (w, h), (wo, ho), row_pad, guard = CASES[case]
    for flip in (False, True):
        got = _resize_aa(hjd, ctx, [(w, h)], wo, ho, dtype, flips=[flip], row_pad=row_pad, guard=guard)
        np.testing.assert_array_equal(got[0], _expect(w, h, wo, ho, flip, dtype),
                                      err_msg=f"{case}: {w}x{h} -> {wo}x{ho} {dtype} flip {flip}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wo,ho,row_pad,guard", [(24, 16, 0, 64), (23, 15, 3, 61)])
def test_mixed_batch_in_one_launch(hjd, ctx, wo, ho, row_pad, guard, dtype):
    """Every case's source size as one item of one launch, every second one flipped:
    sources of 1 to 1000 rows share the horizontal launch's group count."""
    shapes = list(dict.fromkeys(c[0] for c in CASES.values()))
    assert len(shapes) >= 4
    flips = [k % 2 == 1 for k in range(len(shapes))]
    got = _resize_aa(hjd, ctx, shapes, wo, ho, dtype, flips=flips, row_pad=row_pad, guard=guard)
    for k, (w, h) in enumerate(shapes):
        np.testing.assert_array_equal(got[k], _expect(w, h, wo, ho, flips[k], dtype),
                                      err_msg=f"item {k}: {w}x{h} -> {wo}x{ho} {dtype}")


def test_relaunch_and_set_normalize(hjd, ctx):
    """A filter-1 object launches again (same intermediate, same stream) with other constants."""
    import torch
    w, h, wo, ho = 37, 29, 10, 7
    src = torch.from_numpy(np.array(_src(w, h))).cuda()
    out = torch.zeros((1, 3, ho, wo), dtype=torch.float32, device="cuda")
    r = hjd.Resize(ctx, [src], out, normalize=_norm(), antialias=True)
    r.launch()
    other = ((2.0, 0.5, 1.0 / 255.0), (-1.0, 0.0, 0.25))
    r.set_normalize(*other)
    r.launch()
    torch.cuda.synchronize()
    r.close()
    np.testing.assert_array_equal(out[0].cpu().numpy().view(np.uint32),
                                  N.apply(_model_u8(w, h, wo, ho, False), other[0], other[1], np.dtype("float32")))


def test_resize_refusals_write_nothing(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    wide = torch.zeros((3, 2, 1449), dtype=torch.uint8, device="cuda")
    tall = torch.zeros((3, 1449, 2), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3, 1, 1), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(HjdError, match="src_w 1449 -> out_w 1") as e:
        hjd.Resize(ctx, [wide], out, antialias=True)
    assert e.value.code == -1
    with pytest.raises(HjdError, match="src_h 1449 -> out_h 1"):
        hjd.Resize(ctx, [tall], out, antialias=True)
    torch.cuda.synchronize()
    assert int(out.min()) == FILL and int(out.max()) == FILL
    r = hjd.Resize(ctx, [wide], out)          # plain bilinear takes it
    r.close()
    r = hjd.Resize(ctx, [wide[..., :1448]], out, antialias=True)   # the edge itself
    r.launch()
    torch.cuda.synchronize()
    r.close()
    assert int(out.max()) == 0


# ---- from JPEG bytes ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _files():
    """q90 PIL files: 4:2:0 64x48, 4:4:4 200x120, gray 64x48, 4:2:0 200x120."""
    return (_pil(64, 48, 90, 2, seed=41), _pil(200, 120, 90, 0, seed=42), _pil(64, 48, 90, 0, seed=43, gray=True),
            _pil(200, 120, 90, 2, seed=44))


def _decoder(hjd, ctx, datas):
    return hjd.GpuDecoder(ctx, len(datas), 2 * sum(map(len, datas)), 2 * sum(hjd.parse(d).nblocks for d in datas))


def _kw(dtype):
    import torch
    if dtype == "uint8":
        return {"dtype": torch.uint8}
    return {"dtype": getattr(torch, dtype), "mean": MEAN, "std": STD}


def _bits(t, dtype):
    return t.cpu().numpy().view(BITS[dtype])


def _model_of_crops(crops, size, flips, dtype):
    a, b = _norm()
    return [A.resize(c.cpu().numpy(), size[1], size[0], bool(f), np.dtype(dtype), a, b) for c, f in zip(crops, flips)]


# on the grid of scale 2 (32x24 and 100x60): odd origins, a 3.3x and a 2x reduction, an enlargement, one pixel
ROIS_2 = [(3, 1, 20, 23), (10, 5, 80, 50), (31, 23, 1, 1), (1, 0, 48, 32)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_from_jpeg_bytes_equals_resize_of_the_crops_and_the_model(hjd, ctx, dtype):
    import torch
    datas = list(_files())
    size, flips = (16, 24), [True, False, False, True]
    with _decoder(hjd, ctx, datas) as gd:
        for rois in (ROIS_2, None):
            crops = gd.decode_rgb(datas, scale=2, rois=rois)
            gd.sync()
            nbytes = 4 * 3 * size[0] * size[1] * np.dtype(dtype).itemsize
            buf = torch.full((64 + nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
            out = buf[64:64 + nbytes].view(getattr(torch, dtype)).view(4, 3, *size)
            got = gd.decode_rgb_resized(datas, size, flips=flips, out=out, scale=2, rois=rois, antialias=True,
                                        **_kw(dtype))
            gd.sync()
            assert got is out and gd.scale == 1 and gd.out_format == hjd.OUT_BGRX
            full = buf.cpu().numpy()
            assert (full[:64] == FILL).all() and (full[64 + nbytes:] == FILL).all()
            alone = torch.empty_like(out)
            r = hjd.Resize(ctx, crops, alone, flips=flips, normalize=_norm() if dtype != "uint8" else None,
                           antialias=True)
            r.launch()
            torch.cuda.synchronize()
            r.close()
            expect = _model_of_crops(crops, size, flips, dtype)
            for k in range(4):
                np.testing.assert_array_equal(_bits(out[k], dtype), expect[k], err_msg=f"file {k}, rois {rois}")
                np.testing.assert_array_equal(_bits(alone[k], dtype), expect[k], err_msg=f"file {k}, Resize alone")


def test_growing_scratch_then_plain_bilinear(hjd, ctx):
    """Three antialiased calls on one decoder, not synchronised in between:
    small crops, whole frames (the scratch grows behind the first call), the
    small crops again; then the same decoder without antialias, which is the
    bilinear result."""
    datas = list(_files())
    size = (16, 24)
    small = [(1, 1, 9, 7), (7, 5, 40, 30), (63, 47, 1, 1), (9, 9, 30, 50)]
    with _decoder(hjd, ctx, datas) as gd:
        crops_small = gd.decode_rgb(datas, rois=small)
        crops_whole = gd.decode_rgb(datas)
        first = gd.decode_rgb_resized(datas, size, rois=small, antialias=True)
        second = gd.decode_rgb_resized(datas, size, antialias=True)
        third = gd.decode_rgb_resized(datas, size, rois=small, antialias=True)
        plain = gd.decode_rgb_resized(datas, size, rois=small)
        gd.sync()
        none = [False] * 4
        exp_small = _model_of_crops(crops_small, size, none, "uint8")
        exp_whole = _model_of_crops(crops_whole, size, none, "uint8")
        for k in range(4):
            np.testing.assert_array_equal(_bits(first[k], "uint8"), exp_small[k])
            np.testing.assert_array_equal(_bits(second[k], "uint8"), exp_whole[k])
            np.testing.assert_array_equal(_bits(third[k], "uint8"), _bits(first[k], "uint8"))
            np.testing.assert_array_equal(_bits(plain[k], "uint8"),
                                          R.resize_u8(crops_small[k].cpu().numpy(), size[1], size[0]))
        assert any(not np.array_equal(_bits(plain[k], "uint8"), _bits(first[k], "uint8")) for k in range(4))


def test_refused_calls_enqueue_nothing_and_leave_the_decoder_usable(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    datas = list(_files())
    long_file = _pil(1456, 8, 90, 0, seed=45)   # 1456^2 > 2^21 * 1
    size = (7, 10)
    with _decoder(hjd, ctx, datas + [long_file]) as gd:
        out = torch.full((5, 3, 1, 1), FILL, dtype=torch.uint8, device="cuda")
        with pytest.raises(HjdError, match="frame 4: .*src_w 1456 -> out_w 1") as e:
            gd.decode_rgb_resized(datas + [long_file], (1, 1), out=out, antialias=True)
        assert e.value.code == -1
        gd.set_output_format(hjd.OUT_RGB24)
        with pytest.raises(HjdError, match="output format"):
            gd.decode_resized(datas + [long_file], out, antialias=True)
        gd.set_output_format(hjd.OUT_BGRX)
        gd.sync()
        torch.cuda.synchronize()
        assert int(out.min()) == FILL and int(out.max()) == FILL
        assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX
        crops = gd.decode_rgb(datas)
        got = gd.decode_rgb_resized(datas, size, antialias=True)
        gd.sync()
        expect = _model_of_crops(crops, size, [False] * 4, "uint8")
        for k in range(4):
            np.testing.assert_array_equal(_bits(got[k], "uint8"), expect[k])
