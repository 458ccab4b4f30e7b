"""The tone kernels alone (hjd_tone_*, backend.Tone) on uint8 planes.  The
expectation is tests/tone_model.py, the numpy model of the definition in
include/hjd.h; everything is compared bit for bit (the float planes on their
bit patterns through norm_model.table), and no byte outside a payload may be
written: all outputs of a launch lie in one 0xA5-filled buffer, which is
compared as a whole.  The sources lie in a buffer filled with 0x3C, so a
histogram that counted padding would see that value."""
import functools
import itertools

import numpy as np
import pytest

import norm_model as N
import tone_model as T
from test_gpu_resize import BITS, DTYPES, FILL, _imagenet, _src

pytestmark = pytest.mark.gpu

MODES = (T.TABLE, T.AUTOCONTRAST, T.EQUALIZE)
SMALL = list(itertools.product((1, 3, 4, 5, 8, 13), (1, 2, 7)))
CELLS = list(itertools.product(range(4), (0, 1, 3)))   # source pointer offset, row pad
LOOPS = (300, 200)   # 75 * 200 quads > 16 groups * 256 threads: the histogram's threads loop (and 59 groups of tone_kernel)


def _up(x, a):
    return (x + a - 1) // a * a


@functools.lru_cache(maxsize=None)
def _tables():
    rng = np.random.default_rng(31)
    v = np.arange(256)
    t = {"identity": T.IDENTITY,
         "solarize": np.tile(np.where(v < 128, v, 255 - v).astype(np.uint8), (3, 1)),
         "random": rng.integers(0, 256, (3, 256), dtype=np.uint8)}
    for a in t.values():
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _narrow(w, h):
    """A seeded image whose channels span 30..199, 0..255 and 100..102: data curves that are not the identity."""
    rng = np.random.default_rng(7000 * w + h)
    a = np.stack([rng.integers(30, 200, (h, w)), rng.integers(0, 256, (h, w)), rng.integers(100, 103, (h, w))]).astype(np.uint8)
    a.setflags(write=False)
    return a


def _run(hjd, ctx, items, dtype, norm, in_place=False, launches=1):
    """items: (src (3, h, w) uint8, mode, table, source offset 0..3, source row pad, output offset in
    elements 0..3, output row pad in elements).  One Tone object over all of them; after each of its
    launches the whole output buffer is compared with FILL + the model's payloads.  in_place
    (uint8): every output is its source."""
    import torch
    elem = np.dtype(dtype).itemsize
    splace, dplace, soff, doff = [], [], 64, 64
    for src, _, _, so, sp, do, dp in items:
        _, h, w = src.shape
        splace.append((soff + so, w + sp))
        soff = _up(soff + so + 3 * h * (w + sp) + 64, 64)
        dplace.append((doff + do * elem, (w + dp) * elem))
        doff = _up(doff + do * elem + 3 * h * (w + dp) * elem + 64, 64)
    host = np.full(soff, 0x3C, np.uint8)
    expect = np.full(doff, FILL, np.uint8)
    table = None if dtype == "uint8" else N.table(norm[0], norm[1], np.dtype(dtype))   # norm_model.apply's, made once
    for (src, mode, lut, *_), (sa, spitch), (da, dpitch) in zip(items, splace, dplace):
        _, h, w = src.shape
        host[sa:sa + 3 * h * spitch].reshape(3 * h, spitch)[:, :w] = src.reshape(3 * h, w)
        u8 = T.tone_u8(src, mode, lut)
        bits = (u8 if table is None else np.stack([table[c][u8[c]] for c in range(3)])).astype(BITS[dtype])
        expect[da:da + 3 * h * dpitch].reshape(3 * h, dpitch)[:, :w * elem] = bits.reshape(3 * h, w).view(np.uint8)
    sbuf = torch.from_numpy(host).cuda()
    if in_place:
        assert dtype == "uint8" and launches == 1
        out, dplace = sbuf, splace
        expect = host.copy()
        for (src, mode, lut, *_), (sa, spitch) in zip(items, splace):
            _, h, w = src.shape
            expect[sa:sa + 3 * h * spitch].reshape(3 * h, spitch)[:, :w] = T.tone_u8(src, mode, lut).reshape(3 * h, w)
    else:
        out = torch.full((doff,), FILL, dtype=torch.uint8, device="cuda")
    srcs, outs = [], []
    for (src, *_), (sa, spitch), (da, dpitch) in zip(items, splace, dplace):
        _, h, w = src.shape
        srcs.append((sbuf[sa:sa + 3 * h * w].view(3, h, w), spitch))
        outs.append((out[da:da + 3 * h * w * elem].view(getattr(torch, dtype)).view(3, h, w), dpitch))
    op = hjd.Tone(ctx, srcs, outs, curves=[lut for _, _, lut, *_ in items], modes=[mode for _, mode, *_ in items],
                  normalize=norm if dtype != "uint8" else None)
    for launch in range(launches):
        if launch:
            out.fill_(FILL)
        op.launch()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for k, ((src, mode, _, *cell), (da, dpitch)) in enumerate(zip(items, dplace)):
            lo, hi = da, da + 3 * src.shape[1] * dpitch
            assert np.array_equal(got[lo:hi], expect[lo:hi]), \
                f"launch {launch} item {k}: {src.shape[2]}x{src.shape[1]} {dtype} cell {cell} mode {mode}"
        assert np.array_equal(got, expect), "bytes outside the outputs were written"
    op.close()
    if not in_place:
        assert np.array_equal(sbuf.cpu().numpy(), host), "a source was written"


def _cell_item(src, mode, lut, off, pad):
    # the output: its source's offset and pad, but a row pad of 1 gives aligned, unpadded output rows
    # (a byte-loading source with vector stores) at an offset two elements on
    return (src, mode, lut, off, pad, off if pad != 1 else (off + 2) % 4, pad if pad != 1 else 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_sizes_every_cell_every_mode(hjd, ctx, dtype):
    luts = list(_tables().values())
    items = [_cell_item(_narrow(w, h) if k % 2 else _src(w, h), mode, luts[(k + mode) % 3], off, pad)
             for k, ((w, h), (off, pad), mode) in enumerate(itertools.product(SMALL, CELLS, MODES))]
    _run(hjd, ctx, items, dtype, _imagenet())


def test_constant_image_padding_is_not_counted(hjd, ctx):
    """5 x 3 of constant 200: one non-empty bin, so both data curves are the identity.  Counting the
    zeros a guarded quad load returns past column 5 (bin 0), or the 0x3C of the padding, makes two."""
    src = np.full((3, 3, 5), 200, np.uint8)
    assert (T.tone_u8(src, T.AUTOCONTRAST) == 200).all() and (T.tone_u8(src, T.EQUALIZE) == 200).all()
    items = [(src, mode, T.IDENTITY, off, pad, 0, 0) for mode in (T.AUTOCONTRAST, T.EQUALIZE)
             for off, pad in ((0, 3), (0, 0), (1, 2), (0, 7))]   # dword loads with padding, byte loads, ...
    for dtype in ("uint8", "float32"):
        _run(hjd, ctx, items, dtype, _imagenet())


def test_flat_and_two_valued_images(hjd, ctx):
    """64 x 64 of one value: every lane of a wave adds to one bin.  Two values: autocontrast sends them
    to 0 and 255, equalize by their counts."""
    rng = np.random.default_rng(12)
    flat = np.stack([np.full((64, 64), v, np.uint8) for v in (0, 131, 255)])
    two = np.where(rng.random((3, 64, 64)) < 0.3, 90, 160).astype(np.uint8)
    few = np.where(rng.random((3, 16, 16)) < 0.01, 7, 250).astype(np.uint8)   # step 0 or 1 in equalize
    assert set(np.unique(T.tone_u8(two, T.AUTOCONTRAST))) == {0, 255}
    assert not np.array_equal(T.tone_u8(two, T.EQUALIZE), two)
    items = [(im, mode, lut, 0, 0, 0, 0) for im in (flat, two, few) for mode in (T.AUTOCONTRAST, T.EQUALIZE)
             for lut in (T.IDENTITY, _tables()["random"])]
    for dtype in ("uint8", "float16"):
        _run(hjd, ctx, items, dtype, _imagenet())


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_quads_than_the_histogram_groups_hold(hjd, ctx, dtype):
    w, h = LOOPS
    assert -(-w // 4) * h > 16 * 256
    off, pad = {"uint8": (1, 3), "float16": (0, 0), "float32": (2, 1)}[dtype]
    items = [_cell_item(_narrow(w, h), mode, _tables()[name], off, pad)
             for mode, name in ((T.EQUALIZE, "identity"), (T.AUTOCONTRAST, "random"), (T.TABLE, "solarize"))]
    _run(hjd, ctx, items, dtype, _imagenet())


def test_one_object_three_sizes_mixed_modes_launched_twice(hjd, ctx):
    """1 x 1, 224 x 224 and 300 x 200 in one object: groups without work write zeros (the histogram's)
    or return (tone_kernel's); the second launch reuses the tables of the first."""
    sizes = [(1, 1), (224, 224), LOOPS]
    for modes in ((T.EQUALIZE, T.TABLE, T.AUTOCONTRAST), (T.AUTOCONTRAST, T.EQUALIZE, T.EQUALIZE), (T.TABLE, T.TABLE, T.EQUALIZE)):
        items = [(_narrow(w, h), mode, _tables()["random" if mode else "solarize"], 0, 0, 0, 0)
                 for (w, h), mode in zip(sizes, modes)]
        for dtype in DTYPES:
            _run(hjd, ctx, items, dtype, _imagenet(), launches=2)


def test_a_bin_above_2_to_the_24(hjd, ctx):
    """4100 x 4096 of one value: 16,793,600 pixels in one bin, more than 24 bits or a float count.
    Channel R is flat altogether (one bin: the identity); G and B carry a ramp in their first row, so
    their curves depend on the large count (a count taken modulo 2^24 would leave 4,084 + the ramp)."""
    w, h = 4100, 4096
    src = np.full((3, h, w), 40, np.uint8)
    src[1:, 0, :] = np.arange(w) % 256
    assert T.histogram(src)[1].max() > 2 ** 24
    for mode in (T.EQUALIZE, T.AUTOCONTRAST):
        _run(hjd, ctx, [(src, mode, T.IDENTITY, 0, 0, 0, 0)], "uint8", None)


def test_equalize_then_a_solarize_table(hjd, ctx):
    """The data curve runs first, the table second; on this image the other order gives other bytes."""
    src, sol = _narrow(64, 48), _tables()["solarize"]
    other = T.tone_u8(T.tone_u8(src, T.TABLE, sol), T.EQUALIZE)
    assert not np.array_equal(T.tone_u8(src, T.EQUALIZE, sol), other)
    assert np.array_equal(T.tone_u8(src, T.EQUALIZE, sol), T.tone_u8(T.tone_u8(src, T.EQUALIZE), T.TABLE, sol))
    for dtype in DTYPES:
        _run(hjd, ctx, [(src, T.EQUALIZE, sol, 0, 0, 0, 0)], dtype, _imagenet())


def test_in_place_uint8(hjd, ctx):
    t = _tables()
    items = [(_narrow(w, h), mode, t[name], off, pad, off, pad)
             for (w, h), mode, name, off, pad in [((64, 4), T.EQUALIZE, "identity", 0, 0), ((13, 7), T.AUTOCONTRAST, "random", 0, 3),
                                                  ((7, 3), T.TABLE, "solarize", 1, 1), (LOOPS, T.EQUALIZE, "random", 0, 0),
                                                  ((5, 1), T.TABLE, "identity", 2, 0)]]
    _run(hjd, ctx, items, "uint8", None, in_place=True)


def test_one_batch_tensor_defaults_and_refusals(hjd, ctx):
    """outs as one (N, 3, h, w) tensor, curves and modes by default and one for all; what Python and
    the library refuse leaves nothing written."""
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    imgs = np.stack([_narrow(64, 4), _narrow(64, 4)[:, ::-1].copy()])
    src = torch.from_numpy(imgs).cuda()
    out = torch.full((2 * 3 * 4 * 64 * 2,), FILL, dtype=torch.uint8, device="cuda").view(torch.float16).view(2, 3, 4, 64)
    norm = _imagenet()
    with pytest.raises(HjdError, match=r"tone item 1: mode 3 is outside 0..2"):
        hjd.Tone(ctx, [src[0], src[1]], out, modes=[0, 3])
    with pytest.raises(ValueError, match="one tone table"):
        hjd.Tone(ctx, [src[0], src[1]], out, curves=[T.IDENTITY])
    with pytest.raises(ValueError, match="one mode"):
        hjd.Tone(ctx, [src[0], src[1]], out, modes=[1])
    with pytest.raises(ValueError, match="its source"):
        hjd.Tone(ctx, [src[0], src[1]], [out[0], out[1][..., :63]])
    with pytest.raises(HjdError, match="HJD_OUT_RGB_PLANAR_F16"):
        hjd.Tone(ctx, [src[0]], torch.empty((1, 3, 4, 64), dtype=torch.uint8, device="cuda"), normalize=norm)
    torch.cuda.synchronize()
    assert int(out.view(torch.uint8).min()) == FILL and int(out.view(torch.uint8).max()) == FILL
    for kw, mode, lut in (({}, T.TABLE, T.IDENTITY), ({"modes": hjd.TONE_EQUALIZE}, T.EQUALIZE, T.IDENTITY),
                          ({"curves": hjd.tone_curve(solarize=128), "modes": [hjd.TONE_AUTOCONTRAST] * 2}, T.AUTOCONTRAST,
                           _tables()["solarize"])):
        op = hjd.Tone(ctx, [src[0], src[1]], out, normalize=norm, **kw)
        op.launch()
        torch.cuda.synchronize()
        op.close()
        for k in range(2):
            assert np.array_equal(out[k].cpu().numpy().view(np.uint16), T.tone(imgs[k], mode, lut, np.float16, norm[0], norm[1]))
