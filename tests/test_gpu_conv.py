"""The filter kernel alone (hjd_conv_*, backend.Conv) on uint8 planes.  The
expectation is tests/conv_model.py, the numpy model of the definition in
include/hjd.h; everything is compared bit for bit (the float planes on their
bit patterns through norm_model.table), and no byte outside a payload may be
written: all outputs of a launch lie in one 0xA5-filled buffer, which is
compared as a whole.  The sources lie in a buffer filled with 0x3C, so a
window that read padding would see that value."""
import functools
import itertools

import numpy as np
import pytest

import conv_model as C
import norm_model as N
from test_gpu_resize import BITS, DTYPES, FILL, _imagenet, _src

pytestmark = pytest.mark.gpu

BORDERS = (C.KEEP, C.REFLECT, C.REPLICATE)
RADII = ((0, 0), (1, 1), (3, 0), (0, 5), (11, 1), (11, 11))
# the tile edges at 64 and 32, the quad edges at 4
SHAPES = list(itertools.product((1, 2, 3, 4, 5, 8, 13, 63, 64, 65, 67), (1, 2, 7, 31, 32, 33)))
CELLS = list(itertools.product(range(4), (1, 3, 0)))   # source pointer offset, row pad (odd pitches for even widths and back)
GAINS = ((0, 4096), (6932, -2836), (-4096, 8192), (9000, -4904))
HALO = (300, 200)   # 5 x 7 tiles: interior tiles whose halo at radius 11 spans the four neighbours and the diagonals


def _up(x, a):
    return (x + a - 1) // a * a


def _taps(rng, r, total=4096):
    k = rng.integers(1, 400, 2 * r + 1)
    k = (k * (total - (2 * r + 1)) // k.sum()) + 1
    k[r] += total - k.sum()
    assert k.sum() == total and k.min() >= 1
    return [int(v) for v in k]


@functools.lru_cache(maxsize=None)
def _filter(rx, ry, border, gain=0, seed=0):
    """A seeded record of radius (rx, ry): random taps, kh summing to 4096 and kv to 4096 or 3000."""
    rng = np.random.default_rng(1000 * rx + 10 * ry + seed)
    a, b = GAINS[gain % len(GAINS)]
    return C.record(_taps(rng, rx), _taps(rng, ry, 3000 if seed % 2 else 4096), a, b, border)


def _numpy_filter(hjd, f):
    return hjd.conv_filter(f["kh"], f["kv"], f["a"], f["b"], f["border"])


def _key(f):
    return (tuple(f["kh"]), tuple(f["kv"]), f["a"], f["b"], f["border"])


@functools.lru_cache(maxsize=None)
def _model(w, h, key, seed=None):
    """The model's bytes of _src(w, h) (or of a flat image of value `seed`) under the record of `key`; made once."""
    src = _src(w, h) if seed is None else np.full((3, h, w), seed, np.uint8)
    out = C.conv_u8(src, C.record(*key))
    out.setflags(write=False)
    return out


def _run(hjd, ctx, items, dtype, norm, launches=1):
    """items: (src (3, h, w) uint8, record, expected (3, h, w) uint8, source offset 0..3, source row pad, output
    offset in elements 0..3, output row pad in elements).  One Conv object over all of them; after each
    of its launches the whole output buffer is compared with FILL + the expected payloads."""
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
    for (src, f, u8, *_), (sa, spitch), (da, dpitch) in zip(items, splace, dplace):
        _, h, w = src.shape
        host[sa:sa + 3 * h * spitch].reshape(3 * h, spitch)[:, :w] = src.reshape(3 * h, w)
        bits = (u8 if table is None else np.stack([table[c][u8[c]] for c in range(3)])).astype(BITS[dtype])
        expect[da:da + 3 * h * dpitch].reshape(3 * h, dpitch)[:, :w * elem] = bits.reshape(3 * h, w).view(np.uint8)
    sbuf = torch.from_numpy(host).cuda()
    out = torch.full((doff,), FILL, dtype=torch.uint8, device="cuda")
    srcs, outs = [], []
    for (src, *_), (sa, spitch), (da, dpitch) in zip(items, splace, dplace):
        _, h, w = src.shape
        srcs.append((sbuf[sa:sa + 3 * h * w].view(3, h, w), spitch))
        outs.append((out[da:da + 3 * h * w * elem].view(getattr(torch, dtype)).view(3, h, w), dpitch))
    op = hjd.Conv(ctx, srcs, outs, filters=[_numpy_filter(hjd, f) for _, f, *_ in items],
                  normalize=norm if dtype != "uint8" else None)
    for launch in range(launches):
        if launch:
            out.fill_(FILL)
        op.launch()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for k, ((src, f, _, *cell), (da, dpitch)) in enumerate(zip(items, dplace)):
            lo, hi = da, da + 3 * src.shape[1] * dpitch
            assert np.array_equal(got[lo:hi], expect[lo:hi]), \
                f"launch {launch} item {k}: {src.shape[2]}x{src.shape[1]} {dtype} cell {cell} radius ({f['rx']}, {f['ry']}) " \
                f"border {f['border']} gains ({f['a']}, {f['b']})"
        assert np.array_equal(got, expect), "bytes outside the outputs were written"
    op.close()
    assert np.array_equal(sbuf.cpu().numpy(), host), "a source was written"


def _item(w, h, f, off=0, pad=0):
    # the output: its source's offset and pad, but a row pad of 1 gives aligned, unpadded output rows
    # (a byte-loading source with vector stores) at an offset two elements on
    return (_src(w, h), f, _model(w, h, _key(f)), off, pad, off if pad != 1 else (off + 2) % 4, pad if pad != 1 else 0)


def _every_shape(border):
    """Every shape x radius that is legal for the shape under `border`, each in every alignment cell (source
    pointer offset 0..3 x row pad: odd and even pitches); the gains and the taps' sums go round with the items."""
    k = 0
    for (w, h), (rx, ry) in itertools.product(SHAPES, RADII):
        if border == C.REFLECT and (rx >= w or ry >= h):
            continue
        f = _filter(rx, ry, border, gain=k, seed=k % 2)
        for off, pad in CELLS:
            yield _item(w, h, f, off, pad)
        k += 1


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_shape_cell_and_radius(hjd, ctx, dtype, border):
    items = list(_every_shape(border))
    legal = sum(1 for (w, h), (rx, ry) in itertools.product(SHAPES, RADII) if border != C.REFLECT or (rx < w and ry < h))
    assert len(items) == legal * len(CELLS) and legal >= (200 if border == C.REFLECT else len(SHAPES) * len(RADII))
    _run(hjd, ctx, items, dtype, _imagenet())


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_cell_at_the_tile_edges(hjd, ctx, dtype):
    """The shapes around the tile's corner in every alignment cell, radius 11 and the sharpness radius."""
    items = [_item(w, h, _filter(rx, ry, border, gain=k), off, pad)
             for k, ((w, h), (off, pad), border, (rx, ry)) in enumerate(itertools.product(
                 ((63, 31), (64, 32), (65, 33), (67, 33), (13, 33)), CELLS, BORDERS, ((11, 11), (1, 1))))]
    _run(hjd, ctx, items, dtype, _imagenet())


def test_flat_255_and_gain_extremes(hjd, ctx):
    """S = 255 << 24 does not fit int32; a = 2^20 with b = -2^20 cancel products of 2^52; a negative T shifts arithmetically."""
    spread = [178] * 22 + [180]
    w, h = 70, 40
    pins = [(255, C.record(spread, spread, 0, 4096, C.REFLECT), 255),
            (255, C.record(spread, spread, 1 << 20, -(1 << 20), C.REFLECT), 0),
            (255, C.record(spread, spread, -(1 << 20), 1 << 20, C.REPLICATE), 0),
            (1, C.record([4096], [4096], 1 << 20, 0, C.KEEP), 255),
            (255, C.record(spread, [4096], 0, -(1 << 20), C.REPLICATE), 0),
            (200, C.record([4096], [4096], 0, -11, C.KEEP), 0),
            (200, C.record([1000, 2096, 1000], [4096], 0, -11, C.REPLICATE), 0),
            (200, C.record([4096], [4096], 0, -2048, C.KEEP), 0)]
    items = []
    for v, f, want in pins:
        u8 = _model(w, h, _key(f), seed=v)
        assert (u8 == want).all()
        items.append((np.full((3, h, w), v, np.uint8), f, u8, 0, 0, 0, 0))
    for dtype in ("uint8", "float32"):
        _run(hjd, ctx, items, dtype, _imagenet())


@pytest.mark.parametrize("dtype", DTYPES)
def test_interior_tiles_at_radius_11(hjd, ctx, dtype):
    w, h = HALO
    assert w > 3 * 64 and h > 3 * 32
    off, pad = {"uint8": (1, 3), "float16": (0, 0), "float32": (2, 1)}[dtype]
    items = [_item(w, h, _filter(11, 11, border, gain=k, seed=k), off, pad) for k, border in enumerate(BORDERS)]
    items.append(_item(w, h, _filter(1, 1, C.KEEP, gain=1), off, pad))
    _run(hjd, ctx, items, dtype, _imagenet())


def test_one_object_three_sizes_launched_twice(hjd, ctx):
    """1 x 1, 224 x 224 and 300 x 200 in one object: the groups find their image by its tile prefix."""
    sizes = [(1, 1), (224, 224), HALO]
    for radii, borders in ((((0, 0), (11, 11), (1, 1)), (C.KEEP, C.REFLECT, C.KEEP)),
                           (((0, 5), (3, 0), (11, 1)), (C.REPLICATE, C.REFLECT, C.REPLICATE))):
        items = [_item(w, h, _filter(rx, ry, border, gain=k + 1, seed=k)) for k, ((w, h), (rx, ry), border) in
                 enumerate(zip(sizes, radii, borders))]
        for dtype in DTYPES:
            _run(hjd, ctx, items, dtype, _imagenet(), launches=2)


def test_the_identity_record_is_a_copy(hjd, ctx):
    items = [(_src(w, h), C.IDENTITY, _src(w, h), off, pad, off, pad)
             for (w, h), (off, pad) in zip(((1, 1), (5, 3), (64, 32), (67, 33), (300, 200)), CELLS)]
    for dtype in DTYPES:
        _run(hjd, ctx, items, dtype, _imagenet())


def test_one_batch_tensor_defaults_and_refusals(hjd, ctx):
    """outs as one (N, 3, h, w) tensor, filters by default and one for all, the float formats against
    norm_model; what Python and the library refuse leaves nothing written."""
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    imgs = np.stack([_src(64, 8), _src(64, 8)[:, ::-1].copy()])
    src = torch.from_numpy(imgs).cuda()
    out = torch.full((2 * 3 * 8 * 64 * 2,), FILL, dtype=torch.uint8, device="cuda").view(torch.float16).view(2, 3, 8, 64)
    norm = _imagenet()
    blur = hjd.conv_gaussian(1.0)
    with pytest.raises(HjdError, match=r"conv item 1: border 3 is outside 0..2"):
        hjd.Conv(ctx, [src[0], src[1]], out, filters=[blur, hjd.conv_filter([4096], [4096], 4096, 0, 3)])
    with pytest.raises(HjdError, match=r"conv item 0: HJD_CONV_REFLECT needs radius"):
        hjd.Conv(ctx, [src[0], src[1]], out, filters=hjd.conv_gaussian(3.0))   # radius 9 on 8 rows
    with pytest.raises(HjdError, match="dst == src"):
        hjd.Conv(ctx, [src[0]], [src[0]])
    with pytest.raises(ValueError, match="one filter record"):
        hjd.Conv(ctx, [src[0], src[1]], out, filters=[blur])
    with pytest.raises(ValueError, match="its source"):
        hjd.Conv(ctx, [src[0], src[1]], [out[0], out[1][..., :63]])
    with pytest.raises(HjdError, match="HJD_OUT_RGB_PLANAR_F16"):
        hjd.Conv(ctx, [src[0]], torch.empty((1, 3, 8, 64), dtype=torch.uint8, device="cuda"), normalize=norm)
    torch.cuda.synchronize()
    assert int(out.view(torch.uint8).min()) == FILL and int(out.view(torch.uint8).max()) == FILL
    for kw in ({}, {"filters": blur}, {"filters": [hjd.conv_sharpness(1.7), hjd.conv_unsharp(0.8, 1.5)]}):
        op = hjd.Conv(ctx, [src[0], src[1]], out, normalize=norm, **kw)
        op.launch()
        torch.cuda.synchronize()
        op.close()
        fs = kw.get("filters", hjd.CONV_IDENTITY)
        for k in range(2):
            f = C.from_numpy(fs[k] if isinstance(fs, list) else fs)
            assert np.array_equal(out[k].cpu().numpy().view(np.uint16), C.conv(imgs[k], f, np.float16, norm[0], norm[1]))
