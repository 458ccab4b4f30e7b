"""The colour kernels alone (hjd_color_*, backend.Color) on seeded random uint8
planes.  The expectation is tests/color_model.py, the numpy model of the
definition in include/hjd.h; everything is compared bit for bit (the float
planes on their bit patterns through norm_model.apply), and no byte outside a
payload may be written: all outputs of a launch lie in one 0xA5-filled buffer,
which is compared as a whole."""
import functools
import itertools

import numpy as np
import pytest

import color_model as C
import norm_model as N
from test_gpu_resize import BITS, DTYPES, FILL, _imagenet, _src

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (3, 2), (5, 1), (7, 3), (64, 4), (257, 5)]
LARGE = (1028, 257)          # 257 * 257 quads > 256 groups * 256 threads: the threads loop, the table of sums is full
CELLS = list(itertools.product(range(4), (0, 1, 3)))   # source pointer offset, row pad
LARGE_CELL = {"uint8": (1, 3), "float16": (0, 0), "float32": (2, 1)}
LIM, TLIM = C.MAX_COEF, C.MAX_OFFSET


def _up(x, a):
    return (x + a - 1) // a * a


@functools.lru_cache(maxsize=None)
def _records():
    """name -> record: the laws, every sign pattern of the limits, random ones without and with p."""
    rng = np.random.default_rng(21)
    recs = {"identity": C.IDENTITY, "inverse": C.INVERSE}
    for sm, sp, st in itertools.product((1, -1), repeat=3):
        recs[f"limits{sm:+d}{sp:+d}{st:+d}"] = tuple([sm * LIM] * 9 + [sp * LIM] * 9 + [st * TLIM] * 3)
    for k in range(2):
        recs[f"random_m{k}"] = tuple(int(v) for v in rng.integers(-LIM, LIM + 1, 9)) + (0,) * 9 + \
            tuple(int(v) for v in rng.integers(-TLIM, TLIM + 1, 3))
    for k in range(3):   # mild, so that the result is not all clamped: m near I, p a few tenths, t a few grey levels
        m = (np.eye(3) * 4096 + rng.integers(-1500, 1500, (3, 3))).astype(int).ravel()
        recs[f"random_p{k}"] = tuple(int(v) for v in m) + tuple(int(v) for v in rng.integers(-1200, 1200, 9)) + \
            tuple(int(v) for v in rng.integers(-40 * 4096, 40 * 4096, 3))
    return recs


def _run(hjd, ctx, items, dtype, norm, in_place=False):
    """items: (src (3, h, w) uint8, record, source offset 0..3, source row pad, output offset in
    elements 0..3, output row pad in elements).  One Color object over all of them, launched once;
    the whole output buffer is compared with FILL + the model's payloads.  in_place (uint8): every
    output is its source."""
    import torch
    elem = np.dtype(dtype).itemsize
    splace, dplace, soff, doff = [], [], 64, 64
    for src, _, so, sp, do, dp in items:
        _, h, w = src.shape
        splace.append((soff + so, w + sp))
        soff = _up(soff + so + 3 * h * (w + sp) + 64, 64)
        dplace.append((doff + do * elem, (w + dp) * elem))
        doff = _up(doff + do * elem + 3 * h * (w + dp) * elem + 64, 64)
    host = np.full(soff, 0x3C, np.uint8)
    expect = np.full(doff, FILL, np.uint8)
    for (src, rec, *_), (sa, spitch), (da, dpitch) in zip(items, splace, dplace):
        _, h, w = src.shape
        host[sa:sa + 3 * h * spitch].reshape(3 * h, spitch)[:, :w] = src.reshape(3 * h, w)
        u8 = C.color_u8(src, rec)
        bits = (u8 if dtype == "uint8" else N.apply(u8, norm[0], norm[1], np.dtype(dtype))).astype(BITS[dtype])
        expect[da:da + 3 * h * dpitch].reshape(3 * h, dpitch)[:, :w * elem] = bits.reshape(3 * h, w).view(np.uint8)
    sbuf = torch.from_numpy(host).cuda()
    if in_place:
        assert dtype == "uint8"
        out, dplace = sbuf, splace
        expect = host.copy()
        for (src, rec, *_), (sa, spitch) in zip(items, splace):
            _, h, w = src.shape
            expect[sa:sa + 3 * h * spitch].reshape(3 * h, spitch)[:, :w] = C.color_u8(src, rec).reshape(3 * h, w)
    else:
        out = torch.full((doff,), FILL, dtype=torch.uint8, device="cuda")
    srcs, outs = [], []
    for (src, *_), (sa, spitch), (da, dpitch) in zip(items, splace, dplace):
        _, h, w = src.shape
        srcs.append((sbuf[sa:sa + 3 * h * w].view(3, h, w), spitch))
        outs.append((out[da:da + 3 * h * w * elem].view(getattr(torch, dtype)).view(3, h, w), dpitch))
    op = hjd.Color(ctx, srcs, outs, [rec for _, rec, *_ in items], normalize=norm if dtype != "uint8" else None)
    op.launch()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    op.close()
    for k, ((src, rec, *cell), (da, dpitch)) in enumerate(zip(items, dplace)):
        lo, hi = da, da + 3 * src.shape[1] * dpitch
        assert np.array_equal(got[lo:hi], expect[lo:hi]), \
            f"item {k}: {src.shape[2]}x{src.shape[1]} {dtype} cell {cell} record {rec}"
    assert np.array_equal(got, expect), "bytes outside the outputs were written"
    if not in_place:
        np.testing.assert_array_equal(sbuf.cpu().numpy(), host, err_msg="a source was written")


def _cell_item(src, rec, off, pad):
    # the output: its source's offset and pad, but a row pad of 1 gives aligned, unpadded output rows
    # (a byte-loading source with vector stores) at an offset two elements on
    return (src, rec, off, pad, off if pad != 1 else (off + 2) % 4, pad if pad != 1 else 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_sizes_every_cell_every_record(hjd, ctx, dtype):
    items = [_cell_item(_src(w, h), rec, off, pad)
             for (w, h) in SMALL for off, pad in CELLS for rec in _records().values()]
    _run(hjd, ctx, items, dtype, _imagenet())


@pytest.mark.parametrize("dtype", DTYPES)
def test_largest_size_loops_and_fills_the_table(hjd, ctx, dtype):
    w, h = LARGE
    quads = -(-w // 4) * h
    print(f"{w}x{h}: {quads} quads, {min(256, -(-quads // 256))} groups")
    assert quads > 256 * 256
    off, pad = LARGE_CELL[dtype]
    recs = _records()
    items = [_cell_item(_src(w, h), recs[name], off, pad) for name in ("random_p0", "limits+1-1+1", "random_m0")]
    _run(hjd, ctx, items, dtype, _imagenet())


def _boundary_images():
    """Images whose 256 S / N lies exactly on, or next to, a rounding boundary of mq."""
    out = []
    for vals in ([0, 1], [254, 255], [7, 8]):                       # N = 2, an odd sum
        out.append(np.array([[vals]] * 3, np.uint8))
    a = np.zeros((3, 16, 32), np.uint8)                             # N = 512: S = 3 -> 1.5 in Q8, a tie
    a[:, 0, 0] = 3
    out.append(a)
    b = np.full((3, 16, 32), 255, np.uint8)                         # N = 512: S = 512 * 255 - 1 -> 65279.5
    b[:, 15, 31] = 254
    out.append(b)
    c = np.zeros((3, 1, 3), np.uint8)                               # N = 3: thirds, per channel 1/3, 2/3, 3/3
    c[0, 0, 2] = c[1, 0, 1] = c[1, 0, 2] = 1
    c[2] = 1
    out.append(c)
    return out


def _on_the_edge(im, below):
    """A record whose bytes sit on a rounding edge of the last shift, so that one step of mq in either
    direction moves them: p = 32767 I (a step of mq moves T by 128) and t such that T + 2048 is
    100 * 4096 exactly (u8 = 100; a smaller mq gives 99), or with below one less (u8 = 99; a larger mq gives 100)."""
    p = [LIM, 0, 0, 0, LIM, 0, 0, 0, LIM]
    T = C.offsets([0] * 9 + p + [0] * 3, im)
    t = [int(100 * 4096 - 2048 - v) - (1 if below else 0) for v in T]
    rec = tuple([0] * 9 + p + t)
    assert (C.color_u8(im, rec) == (99 if below else 100)).all()
    return rec


def test_sums_on_the_rounding_boundaries_of_the_mean(hjd, ctx):
    imgs = _boundary_images()
    assert C.means_q8(imgs[0]).tolist() == [128] * 3 and C.means_q8(imgs[3]).tolist() == [2] * 3
    assert C.means_q8(imgs[4]).tolist() == [65280] * 3 and C.means_q8(imgs[5]).tolist() == [85, 171, 256]
    recs = [tuple([0] * 9 + [4096] * 9 + [0] * 3),                                   # the sum of the means
            tuple([4096, 0, 0, 0, 4096, 0, 0, 0, 4096] + [-2048] * 9 + [1 << 11] * 3),
            tuple([0] * 9 + [1, -1, 1, 128, 0, 0, 0, 0, -128] + [100 * 4096, 0, 200 * 4096])]
    pairs = list(itertools.product(imgs, recs)) + [(im, _on_the_edge(im, below)) for im in imgs for below in (False, True)]
    items = [(im, rec, k % 4, (0, 1, 3)[k % 3], k % 4, 0) for k, (im, rec) in enumerate(pairs)]
    for dtype in ("uint8", "float32"):
        _run(hjd, ctx, items, dtype, _imagenet())


def test_one_object_three_sizes_one_with_sums(hjd, ctx):
    recs = _records()
    for order in (("random_m0", "random_p1", "inverse"), ("random_p2", "identity", "random_m1")):
        items = [(_src(w, h), recs[name], 0, 0, 0, 0) for (w, h), name in zip([(257, 5), (64, 4), (3, 2)], order)]
        assert sum(any(rec[9:18]) for _, rec, *_ in items) == 1
        for dtype in DTYPES:
            _run(hjd, ctx, items, dtype, _imagenet())


def test_in_place_uint8(hjd, ctx):
    recs = _records()
    items = [(_src(w, h), recs[name], off, pad, off, pad)
             for (w, h), name, off, pad in [((64, 4), "random_p0", 0, 0), ((257, 5), "inverse", 0, 3), ((7, 3), "random_p1", 1, 1),
                                            (LARGE, "random_p2", 0, 0), ((5, 1), "identity", 2, 0)]]
    _run(hjd, ctx, items, "uint8", None, in_place=True)


def test_one_batch_tensor_and_refusals(hjd, ctx):
    """outs as one (N, 3, h, w) tensor; what Python and the library refuse leaves nothing written."""
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    src = torch.from_numpy(np.stack([_src(64, 4), _src(64, 4)[:, ::-1].copy()])).cuda()
    out = torch.full((2 * 3 * 4 * 64 * 2,), FILL, dtype=torch.uint8, device="cuda").view(torch.float16).view(2, 3, 4, 64)
    recs = [_records()["random_p0"], _records()["inverse"]]
    norm = _imagenet()
    bad = list(C.IDENTITY)
    bad[4] = 32768
    with pytest.raises(HjdError, match=r"color item 1: m\[4\] = 32768"):
        hjd.Color(ctx, [src[0], src[1]], out, [recs[0], bad])
    with pytest.raises(ValueError, match="21 integers"):
        hjd.Color(ctx, [src[0], src[1]], out, [recs[0], recs[1][:20]])
    with pytest.raises(ValueError, match="one output and one colour record"):
        hjd.Color(ctx, [src[0], src[1]], out, recs[:1])
    with pytest.raises(ValueError, match="its source"):
        hjd.Color(ctx, [src[0], src[1]], [out[0], out[1][..., :63]], recs)
    with pytest.raises(HjdError, match="HJD_OUT_RGB_PLANAR_F16"):
        hjd.Color(ctx, [src[0]], torch.empty((1, 3, 4, 64), dtype=torch.uint8, device="cuda"), recs[:1], normalize=norm)
    torch.cuda.synchronize()
    assert int(out.view(torch.uint8).min()) == FILL and int(out.view(torch.uint8).max()) == FILL
    op = hjd.Color(ctx, [src[0], src[1]], out, recs, normalize=norm)
    op.launch()
    torch.cuda.synchronize()
    op.close()
    for k in range(2):
        np.testing.assert_array_equal(out[k].cpu().numpy().view(np.uint16),
                                      C.color(src[k].cpu().numpy(), recs[k], np.float16, norm[0], norm[1]))
