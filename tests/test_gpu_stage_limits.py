"""The stage kernels (resize, antialiased resize, orient, warp) where their
32-bit arithmetic and their 64-bit offsets are at their limits:

  1  dimensions of 16384 (include/hjd.h: "all four dimensions lie in 1..16384"),
     the antialiased filter's legality edge src^2 = 2^21 * out, and warp matrices
     of INT32_MIN / INT32_MAX;
  2  source and destination pitches of 2^30 bytes, so that row and plane offsets
     inside ONE image pass 2^31 and 2^32;
  3  the float stores on the constants where rounding goes wrong (half
     subnormals, +0, half overflow, two roundings) and on fp32-subnormal results,
     the fused kernels' included.

Every comparison is bit for bit against the numpy models (resize_model,
resize_aa_model, orient_model, warp_model, norm_model), the float planes on
their bit patterns; every output lies in a 0xA5-filled buffer of which no byte
outside the payload may change (parts 1 and 3 compare the buffer on the host,
part 2 counts on the device).  Each test first asserts, from the kernel's own
formula, that its shape reaches the range it is there for, and prints the value."""
import functools

import numpy as np
import pytest

import norm_model as N
import orient_model as OM
import resize_aa_model as A
import resize_model as R
import warp_model as W
from test_gpu_resize import BITS, _imagenet, _src

pytestmark = pytest.mark.gpu

FILL = 0xA5
MAX = 16384
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


# ---- buffers ------------------------------------------------------------------------------------
def count_not_fill(buf):
    """Bytes of a device uint8 buffer that differ from FILL, counted on the
    device over int64 words, 1 GiB at a time (the temporaries stay at 128 MiB)."""
    import torch
    assert buf.dtype == torch.uint8 and buf.is_contiguous() and buf.numel() % 8 == 0 and buf.data_ptr() % 8 == 0
    words = buf.view(torch.int64)
    fill = int.from_bytes(bytes([FILL] * 8), "little", signed=True)
    n, chunk = 0, 1 << 27
    for lo in range(0, words.numel(), chunk):
        part = words[lo:lo + chunk]
        idx = (part != fill).nonzero().flatten()
        if idx.numel():
            n += int((part[idx].view(torch.uint8) != FILL).sum())
    return n


def rows_of(buf, offset, rows, pitch, row_bytes):
    """`rows` rows of row_bytes bytes, pitch bytes apart from `offset` of a device byte buffer, on the host."""
    import torch
    return torch.as_strided(buf, (rows, row_bytes), (pitch, 1), offset).cpu().numpy()


def _dev_source(src, offset=64, pad=0):
    """(3, h, w) bytes on the device at `offset` of a buffer of their own, rows w + pad apart, as a [..., :w] view."""
    import torch
    _, h, w = src.shape
    sp = w + pad
    host = np.full(offset + 3 * h * sp + 64, 0x3C, np.uint8)
    host[offset:offset + 3 * h * sp].reshape(3, h, sp)[..., :w] = src
    buf = torch.from_numpy(host).cuda()
    return buf[offset:offset + 3 * h * sp].view(3, h, sp)[..., :w]


def _batch(make, srcs, wo, ho, dtype, row_pad=0, guard=64, form=None):
    """make(srcs, out) -> a Resize or Warp object over the device sources,
    launched into an (N, 3, ho, wo) view of a FILL-filled buffer (guard bytes
    in front, rows wo + row_pad elements apart).  Returns the payload's bit
    patterns, having asserted that no other byte of the buffer changed."""
    import torch
    n, elem = len(srcs), np.dtype(dtype).itemsize
    p = wo + row_pad
    nbytes = n * 3 * ho * p * elem
    buf = torch.full((guard + nbytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[guard:guard + nbytes].view(getattr(torch, dtype)).view(n, 3, ho, p)[..., :wo]
    r = make(srcs, out)
    if form is None:
        r.launch()
    else:
        r.launch_form(form)
    torch.cuda.synchronize()
    r.close()
    full = buf.cpu().numpy()
    rows = full[guard:guard + nbytes].reshape(n * 3 * ho, p * elem)
    assert (full[:guard] == FILL).all() and (full[guard + nbytes:] == FILL).all() and \
        (rows[:, wo * elem:] == FILL).all(), "bytes outside the payload were written"
    return np.ascontiguousarray(rows[:, :wo * elem]).view(BITS[dtype]).reshape(n, 3, ho, wo)


def _bits(u8, dtype, norm):
    return u8 if dtype == "uint8" else N.apply(u8, norm[0], norm[1], np.dtype(dtype))


def _norm_of(dtype, norm):
    return norm if dtype != "uint8" else None


# =================================================================================================
# 1  dimension limits
# =================================================================================================
# ---- bilinear resize ----------------------------------------------------------------------------
RESIZE_SHAPES = [((16384, 3), (16384, 2)), ((16384, 3), (5, 2)), ((16384, 2), (1, 1)), ((2, 2), (16384, 3)),
                 ((3, 16384), (2, 16384)), ((3, 16384), (2, 5)), ((2, 2), (3, 16384)),
                 ((16383, 3), (16383, 2))]      # the last: guarded stores
ALL_DTYPES_AT = (0, 3)


@functools.lru_cache(maxsize=None)
def _resize_model(w, h, wo, ho, flip):
    return R.resize_u8(_src(w, h), wo, ho, flip)


def _resize_peak(size, out):
    """The largest (2j + 1) * size and (rem << 11) that resize_tap forms on one axis."""
    j = np.arange(out, dtype=np.int64)
    n = np.maximum((2 * j + 1) * size - out, 0)
    return int(((2 * j + 1) * size).max()), int(((n % (2 * out)) << 11).max())


@pytest.mark.parametrize("k", range(len(RESIZE_SHAPES)))
def test_bilinear_at_the_dimension_limits(hjd, ctx, k):
    (w, h), (wo, ho) = RESIZE_SHAPES[k]
    peaks = [_resize_peak(w, wo), _resize_peak(h, ho)]
    print(f"resize {w}x{h} -> {wo}x{ho}: max (2j+1)*size {max(p[0] for p in peaks)}, max rem<<11 {max(p[1] for p in peaks)}")
    assert max(w, h, wo, ho) >= MAX - 1 and all(p[0] < 2 ** 31 and p[1] < 2 ** 31 for p in peaks)
    if (w, wo) == (MAX, MAX):
        assert peaks[0][0] == (2 * MAX - 1) * MAX >= 2 ** 29 - 2 ** 14   # the most that sizes up to 16384 can form
    src = _dev_source(_src(w, h))
    norm = _imagenet()
    for dtype in (["uint8", "float16", "float32"] if k in ALL_DTYPES_AT else ["uint8"]):
        got = _batch(lambda s, o: hjd.Resize(ctx, s, o, flips=[False, True], normalize=_norm_of(dtype, norm)),
                     [src, src], wo, ho, dtype)
        for item, flip in enumerate((False, True)):
            np.testing.assert_array_equal(got[item], _bits(_resize_model(w, h, wo, ho, flip), dtype, norm),
                                          err_msg=f"{w}x{h} -> {wo}x{ho} {dtype} flip {flip}")


# ---- antialiased resize -------------------------------------------------------------------------
AA_EDGE = [((16384, 2), (128, 1)), ((2, 16384), (2, 128)), ((1448, 2), (1, 2)), ((2, 1448), (2, 1))]
AA_OTHER = [((2, 2), (16384, 3)), ((2, 2), (3, 16384)), ((16384, 3), (16384, 2)), ((16384, 2), (16383, 2))]
AA_F16_AT = [((16384, 2), (128, 1)), ((2, 2), (16384, 3))]


@functools.lru_cache(maxsize=None)
def _aa_source(kind, w, h):
    if kind == "random":
        return _src(w, h)
    a = np.full((3, h, w), 255, np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _aa_model(kind, w, h, wo, ho):
    """(not flipped, flipped): resize_aa_model.resize_u8 with the horizontal
    pass, which the two share, computed once."""
    mid = A.axis_pass(_aa_source(kind, w, h).astype(np.int64), wo)
    return tuple(np.ascontiguousarray(A.axis_pass(m.swapaxes(1, 2), ho).swapaxes(1, 2).astype(np.uint8))
                 for m in (mid, mid[:, :, ::-1]))


def _aa_peak(size, out):
    """The largest weight sum T of one axis and the accumulator's peak 255 T + T / 2."""
    t = max(int(t.sum()) for _, t in A.axis_weights(size, out))
    return t, 255 * t + t // 2


def _aa_check(hjd, ctx, kind, w, h, wo, ho, dtypes):
    src = _dev_source(_aa_source(kind, w, h), offset=61, pad=3)   # an odd address and pitch: byte loads anyway
    norm = _imagenet()
    for dtype in dtypes:
        got = _batch(lambda s, o: hjd.Resize(ctx, s, o, flips=[False, True], normalize=_norm_of(dtype, norm),
                                             antialias=True), [src, src], wo, ho, dtype)
        for item in range(2):
            np.testing.assert_array_equal(got[item], _bits(_aa_model(kind, w, h, wo, ho)[item], dtype, norm),
                                          err_msg=f"{kind} {w}x{h} -> {wo}x{ho} {dtype} flip {bool(item)}")


@pytest.mark.parametrize("kind", ["random", "255"])
@pytest.mark.parametrize("k", range(len(AA_EDGE)))
def test_antialiased_at_the_legality_edge(hjd, ctx, k, kind):
    (w, h), (wo, ho) = AA_EDGE[k]
    size, out = (w, wo) if max(w, wo) > max(h, ho) else (h, ho)
    t, acc = _aa_peak(size, out)
    print(f"aa {size} -> {out}: T {t}, accumulator peak {acc} = 2^{np.log2(acc):.4f}")
    # src^2 <= 2^21 out caps T at 2 src^2 / out + 2 src, the accumulator near 255.5 * 2^22 = 2^30 - 2^21
    assert A.legal(size, out) and not A.legal(size + 1, out) and 2 ** 29 <= acc < 2 ** 31
    if size == MAX:
        assert acc >= 2 ** 30 - 2 ** 22
    if kind == "255":
        assert (_aa_model(kind, w, h, wo, ho)[0] == 255).all()     # the peak is reached and divides back exactly
    if k == 0:
        assert np.array_equal(_aa_model(kind, w, h, wo, ho)[1], A.resize_u8(_aa_source(kind, w, h), wo, ho, True))
    _aa_check(hjd, ctx, kind, w, h, wo, ho, ["uint8", "float16"] if AA_EDGE[k] in AA_F16_AT else ["uint8"])


@pytest.mark.parametrize("k", range(len(AA_OTHER)))
def test_antialiased_at_the_dimension_limits(hjd, ctx, k):
    (w, h), (wo, ho) = AA_OTHER[k]
    peak = max((2 * o - 1) * s + 2 * max(s, o) for s, o in ((w, wo), (h, ho)))   # c + s2 of resize_aa_first
    print(f"aa {w}x{h} -> {wo}x{ho}: max (2j+1)*size + 2 max(size, out) {peak}")
    assert max(wo, ho) >= MAX - 1 and peak < 2 ** 31
    if min(w, wo) >= MAX - 1:
        assert peak >= 2 ** 29 - 2 ** 16
    _aa_check(hjd, ctx, "random", w, h, wo, ho, ["uint8", "float16"] if AA_OTHER[k] in AA_F16_AT else ["uint8"])


def test_antialiased_refuses_one_past_the_edge(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    wide = torch.zeros((3, 2, MAX), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 3, 1, 127), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(HjdError, match="src_w 16384 -> out_w 127"):
        hjd.Resize(ctx, [wide], out, antialias=True)
    with pytest.raises(HjdError, match="src_w 1449 -> out_w 1"):
        hjd.Resize(ctx, [wide[..., :1449]], out[..., :1], antialias=True)
    with pytest.raises(HjdError, match="src_h 1449 -> out_h 1"):
        hjd.Resize(ctx, [torch.zeros((3, 1449, 2), dtype=torch.uint8, device="cuda")], out[..., :1], antialias=True)
    torch.cuda.synchronize()
    assert int(out.min()) == FILL and int(out.max()) == FILL


# ---- orient -------------------------------------------------------------------------------------
ORIENT_SIZES = [(16384, 1), (1, 16384), (16384, 5), (5, 16384), (16383, 3)]
T = 128   # hjd::kOrientTile


def _up(x, a):
    return (x + a - 1) // a * a


def _orient_all(hjd, ctx, S, dtype, odd, norm):
    """All eight orientations of S (3, h, w) as eight items of one launch, each
    into its own place of one FILL-filled buffer, which is compared as a whole.
    odd: source pitch + 1 byte and output pitches + 1 element (the byte paths)."""
    import torch
    _, h, w = S.shape
    elem = np.dtype(dtype).itemsize
    src = _dev_source(S, pad=(_up(w, 4) - w) + (1 if odd else 0))
    places, off = [], 64
    for o in range(1, 9):
        dw, dh = OM.oriented_size(w, h, o)
        dpitch = (_up(dw, 4) + (1 if odd else 0)) * elem
        places.append((off, dpitch, dw, dh))
        off = _up(off + 3 * dh * dpitch + 64, 64)
    expect = np.full(off, FILL, np.uint8)
    out = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
    outs = []
    for o, (base, dpitch, dw, dh) in zip(range(1, 9), places):
        bits = _bits(OM.orient(S, o), dtype, norm).astype(BITS[dtype])
        expect[base:base + 3 * dh * dpitch].reshape(3 * dh, dpitch)[:, :dw * elem] = bits.reshape(3 * dh, dw).view(np.uint8)
        outs.append((out[base:base + 3 * dh * dw * elem].view(getattr(torch, dtype)).view(3, dh, dw), dpitch))
    op = hjd.Orient(ctx, [src] * 8, outs, list(range(1, 9)), normalize=_norm_of(dtype, norm))
    op.launch()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    op.close()
    for o, (base, dpitch, dw, dh) in zip(range(1, 9), places):
        lo, hi = base, base + 3 * dh * dpitch
        assert np.array_equal(got[lo:hi], expect[lo:hi]), f"{w}x{h} orientation {o} {dtype} odd {odd}"
    assert np.array_equal(got, expect), "bytes outside the outputs were written"


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("w,h", ORIENT_SIZES)
def test_orient_at_the_dimension_limits(hjd, ctx, w, h, odd):
    tiles = -(-w // T) * -(-h // T)
    print(f"orient {w}x{h}: {tiles} tiles per plane, {8 * 3 * tiles} in the launch")
    assert tiles == 128 and max(w, h) >= MAX - 1      # 8 items x 3 planes x 128 tiles: the bisection over tile_begin
    for dtype in (["uint8", "float32"] if (w, h) == (16384, 5) else ["uint8"]):
        _orient_all(hjd, ctx, _src(w, h), dtype, odd, _imagenet())


# ---- warp ---------------------------------------------------------------------------------------
WARP_FILL = 0xC0FFEE
WARP_MATRICES = {
    "identity": W.IDENTITY,
    "mirrored_crop": (-65536, 0, 16383 << 16, 0, 65536, 1 << 15),
    "transpose": (0, 65536, 0, 65536, 0, 0),
    "near_identity": (65535, 7, -3, 1, 65533, -65536),
}
WARP_EXTREME = [(INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN),
                (INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX)]


def _warp_items(hjd, ctx, S, matrices, wo, ho, forms=(None,)):
    """Every matrix with the fill colour and with replicate, as items of one launch over one source."""
    items = [(m, rep) for m in matrices for rep in (False, True)]
    src = _dev_source(S)
    exp = [W.warp_u8(S, m, wo, ho, WARP_FILL, W.REPLICATE if rep else 0) for m, rep in items]
    for form in forms:
        got = _batch(lambda s, o: hjd.Warp(ctx, s, o, [m for m, _ in items], fills=[WARP_FILL] * len(items),
                                           replicate=[rep for _, rep in items]),
                     [src] * len(items), wo, ho, "uint8", form=form)
        for k, (m, rep) in enumerate(items):
            np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{S.shape[2]}x{S.shape[1]} -> {wo}x{ho} {m} "
                                                                  f"replicate {rep} form {form}")
    return exp


@pytest.mark.parametrize("wo,ho", [(16384, 2), (2, 16384)])
@pytest.mark.parametrize("w,h", [(16384, 3), (3, 16384)])
def test_warp_at_the_dimension_limits(hjd, ctx, w, h, wo, ho):
    peak = max(int(np.abs(np.stack(W.positions(m, wo, ho))).max()) for m in WARP_MATRICES.values())
    print(f"warp {w}x{h} -> {wo}x{ho}: max |X| {peak} = 2^{np.log2(peak):.3f}")
    assert peak >= 16383 << 16 and peak >> 16 < 2 ** 31          # m * index up to 2^30 - 2^16
    both_forms = (w, h, wo, ho) == (16384, 3, 16384, 2)
    exp = _warp_items(hjd, ctx, _src(w, h), list(WARP_MATRICES.values()), wo, ho,
                      forms=(None, False, True) if both_forms else (None,))
    if (w, h, wo, ho) == (16384, 3, 16384, 2):
        np.testing.assert_array_equal(exp[0], _src(w, h)[:, :2])           # the identity is the crop
    if (w, h, wo, ho) == (3, 16384, 16384, 2):
        np.testing.assert_array_equal(exp[4], _src(w, h)[:, :, :2].transpose(0, 2, 1))


@pytest.mark.parametrize("wo,ho", [(16384, 2), (2, 16384)])
def test_warp_extreme_matrices(hjd, ctx, wo, ho):
    """Coordinates near +-2^45: X >> 16 still fits int32 and every tap is clamped."""
    for m in WARP_EXTREME:
        X, Y = W.positions(m, wo, ho)
        peak = int(max(np.abs(X).max(), np.abs(Y).max()))
        print(f"warp {m[0]:+d}.. -> {wo}x{ho}: max |X| {peak} = 2^{np.log2(peak):.3f}")
        assert 2 ** 44 <= peak < 2 ** 46 and peak >> 16 < 2 ** 31 - 1
        x0, y0 = X >> 16, Y >> 16
        assert (((x0 < -1) | (x0 > 37)) | ((y0 < -1) | (y0 > 29))).mean() > 0.99   # (almost) every tap outside 37 x 29
    _warp_items(hjd, ctx, _src(37, 29), WARP_EXTREME, wo, ho)


# =================================================================================================
# 2  pitches and planes past 2^31 and 2^32 inside one image
# =================================================================================================
KINDS = ["resize", "resize_aa", "orient", "warp"]
PITCH = 1 << 30
SW, SH = 40, 3
ROT180 = (-65536, 0, (SW - 1) << 16, 0, -65536, (SH - 1) << 16)


@functools.lru_cache(maxsize=None)
def _small(w=SW, h=SH):
    """(3, h, w) bytes, all 256 values present."""
    rng = np.random.default_rng(77)
    a = np.concatenate([rng.permutation(256), rng.integers(0, 256, 3 * h * w - 256)]).astype(np.uint8)
    a = rng.permutation(a).reshape(3, h, w)
    assert len(np.unique(a)) == 256
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("pitch", [PITCH, PITCH + 1])
@pytest.mark.parametrize("kind", KINDS)
def test_source_pitch_of_1gib(hjd, ctx, kind, pitch):
    """Rows 2^30 (+ 1: the byte path) bytes apart: row 2 lies at 2^31, the plane
    stride is 3 * 2^30 and plane B lies at 6 * 2^30.  Only the nine rows are written."""
    import torch
    S = _small()
    print(f"{kind}: source row 2 at {2 * pitch}, plane stride {SH * pitch}, plane B at {2 * SH * pitch}")
    assert (SH - 1) * pitch >= 2 ** 31 and 2 * SH * pitch >= 2 ** 32
    torch.cuda.reset_peak_memory_stats()
    big = torch.empty((3, SH, pitch), dtype=torch.uint8, device="cuda")
    src = big[..., :SW]
    src.copy_(torch.from_numpy(np.array(S)))
    if kind == "resize":
        got = _batch(lambda s, o: hjd.Resize(ctx, s, o, flips=[False, True]), [src, src], 23, 5, "uint8")
        exp = [R.resize_u8(S, 23, 5, f) for f in (False, True)]
    elif kind == "resize_aa":
        got = _batch(lambda s, o: hjd.Resize(ctx, s, o, flips=[False, True], antialias=True), [src, src], 23, 2, "uint8")
        exp = [A.resize_u8(S, 23, 2, f) for f in (False, True)]
    elif kind == "warp":
        got = _batch(lambda s, o: hjd.Warp(ctx, s, o, [W.IDENTITY, ROT180]), [src, src], SW, SH, "uint8")
        exp = [W.warp_u8(S, W.IDENTITY, SW, SH), W.warp_u8(S, ROT180, SW, SH)]
        assert np.array_equal(exp[0], S) and np.array_equal(exp[1], S[:, ::-1, ::-1])
    else:
        outs = [torch.full((3,) + OM.oriented_size(SW, SH, o)[::-1], FILL, dtype=torch.uint8, device="cuda")
                for o in range(1, 9)]
        op = hjd.Orient(ctx, [src] * 8, outs, list(range(1, 9)))
        op.launch()
        torch.cuda.synchronize()
        op.close()
        got, exp = [t.cpu().numpy() for t in outs], [OM.orient(S, o) for o in range(1, 9)]
    for k, e in enumerate(exp):
        np.testing.assert_array_equal(got[k], e, err_msg=f"{kind} item {k}")
    np.testing.assert_array_equal(src.cpu().numpy(), S, err_msg="the source was written")
    print(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    del big, src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("kind", KINDS)
def test_destination_pitch_of_1gib(hjd, ctx, kind, dtype):
    """Output rows 2^30 bytes apart (2^28 float elements), three rows per
    plane: i * out_pitch reaches 2^31 and c * dplane 6 * 2^30.  The payload is
    compared on the host, the rest of the 9 GiB buffer counted on the device."""
    import torch
    S, norm = _small(), _imagenet()
    elem, guard = np.dtype(dtype).itemsize, 64
    print(f"{kind} {dtype}: output row 2 at {2 * PITCH}, plane stride {SH * PITCH}, plane B at {2 * SH * PITCH}")
    assert (SH - 1) * PITCH >= 2 ** 31 and 2 * SH * PITCH >= 2 ** 32
    torch.cuda.reset_peak_memory_stats()
    buf = torch.empty((guard + 3 * SH * PITCH + 64,), dtype=torch.uint8, device="cuda")
    body = buf[guard:guard + 3 * SH * PITCH].view(getattr(torch, dtype)).view(1, 3, SH, PITCH // elem)
    small = _dev_source(S)

    def run(make, wo, exp_u8, what):
        buf.fill_(FILL)
        op = make()
        op.launch()
        torch.cuda.synchronize()
        op.close()
        got = rows_of(buf, guard, 3 * SH, PITCH, wo * elem)
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(BITS[dtype]).reshape(3, SH, wo),
                                      _bits(exp_u8, dtype, norm), err_msg=what)
        assert count_not_fill(buf) == int((got != FILL).sum()), f"bytes outside the payload were written: {what}"

    nk = _norm_of(dtype, norm)
    if kind == "orient":
        tall = _dev_source(_small(SH, SW))          # 3 wide, 40 tall: orientations 5..8 give 40 x 3
        for o in range(1, 9):
            s_np, s_dev = (S, small) if o < 5 else (_small(SH, SW), tall)
            carrier = buf[guard:guard + 3 * SH * SW * elem].view(getattr(torch, dtype)).view(3, SH, SW)
            run(lambda: hjd.Orient(ctx, [s_dev], [(carrier, PITCH)], [o], normalize=nk), SW, OM.orient(s_np, o),
                f"orientation {o}")
    else:
        for wo in (24, 23):                         # the vector stores, the per-element stores
            out = body[..., :wo]
            if kind == "resize":
                run(lambda: hjd.Resize(ctx, [small], out, flips=[True], normalize=nk), wo,
                    R.resize_u8(S, wo, SH, True), f"wo {wo}")
            elif kind == "resize_aa":
                run(lambda: hjd.Resize(ctx, [small], out, normalize=nk, antialias=True), wo,
                    A.resize_u8(S, wo, SH), f"wo {wo}")
            else:
                m = (65536, 300, 5 << 16, -200, 65536, 1 << 14)
                run(lambda: hjd.Warp(ctx, [small], out, [m], fills=[WARP_FILL], normalize=nk), wo,
                    W.warp_u8(S, m, wo, SH, WARP_FILL), f"wo {wo}")
    print(f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    del buf, body, run
    torch.cuda.empty_cache()


# =================================================================================================
# 3  the float stores on the constants where rounding goes wrong
# =================================================================================================
FW, FH = 32, 8
# fp32-subnormal results: a itself subnormal; and a normal a
# with a b that cancels bytes 77 / 128 / 255 of R / G / B into the subnormal
# range, exactly: (v - 77) * 2^-120 + v * 2^-143
SUB_A = ((2.0 ** -140,) * 3, (0.0, 0.0, 0.0))
SUB_CANCEL = (((1 + 2.0 ** -23) * 2.0 ** -120,) * 3, (-77 * 2.0 ** -120, -128 * 2.0 ** -120, -255 * 2.0 ** -120))


@functools.lru_cache(maxsize=None)
def _all_bytes():
    """(3, 8, 32): every plane holds all 256 bytes, each in an order of its own."""
    rng = np.random.default_rng(256)
    a = np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8).reshape(3, FH, FW)
    a.setflags(write=False)
    return a


def _constants(name):
    from test_gpu_norm_outputs import EDGE, _two_roundings
    return {"edge": EDGE, "two_roundings": _two_roundings()[0], "sub_a": SUB_A, "sub_cancel": SUB_CANCEL}[name]


def _subnormal_premise(name, norm):
    f32 = N.table(norm[0], norm[1], np.float32)
    sub = ((f32 & 0x7f800000) == 0) & ((f32 & 0x007fffff) != 0)
    print(f"{name}: fp32-subnormal results per channel {sub.sum(axis=1).tolist()}")
    if name == "sub_a":
        assert (sub[:, 1:]).all()                         # every byte but 0
    if name == "sub_cancel":
        assert sub[0, 77] and sub[1, 128] and sub[2, 255] and sub.sum() == 3
        assert f32[0, 77] == 77 * 64                      # 77 * 2^-143 on the 2^-149 grid


@pytest.mark.parametrize("path", ["vector", "per_element"])
@pytest.mark.parametrize("name,dtype", [("edge", "float16"), ("edge", "float32"), ("two_roundings", "float16"),
                                        ("sub_a", "float16"), ("sub_a", "float32"), ("sub_cancel", "float16"),
                                        ("sub_cancel", "float32")])
def test_stage_kernels_float_stores(hjd, ctx, name, dtype, path):
    """An identity Resize, a same-size antialiased Resize, Orient 1 and 6 and an
    identity Warp of a source with all 256 bytes in every plane reproduce
    norm_model.apply.  per_element: rows one element longer than 32."""
    norm = _constants(name)
    S = _all_bytes()
    if name.startswith("sub"):
        _subnormal_premise(name, norm)
    if name == "edge":
        t = N.table(norm[0], norm[1], np.float16)
        half_sub = ((t[0] & 0x7c00) == 0) & ((t[0] & 0x03ff) != 0)
        print(f"edge: {half_sub.sum()} half-subnormal R results, G[128] {t[1][128]:#06x}, {(t[2] == 0x7c00).sum()} B overflows")
        assert half_sub.sum() >= 32 and t[1][128] == 0 and (t[2] == 0x7c00).any() and (t[2] != 0x7c00).any()
    if name == "two_roundings":
        t = N.table(norm[0], norm[1], np.float16)
        exact = np.array([[np.float16(float(np.float32(a)) * v) for v in range(256)] for a in norm[0]]).view(np.uint16)
        assert (t != exact).any()                         # one rounding would differ on bytes the source holds
    pad = 0 if path == "vector" else 1
    src = _dev_source(S)
    exp = N.apply(S, norm[0], norm[1], np.dtype(dtype))
    makers = {
        "resize": lambda s, o: hjd.Resize(ctx, s, o, normalize=norm),
        "resize_aa": lambda s, o: hjd.Resize(ctx, s, o, normalize=norm, antialias=True),
        "warp": lambda s, o: hjd.Warp(ctx, s, o, [W.IDENTITY], normalize=norm),
    }
    for kind, make in makers.items():
        got = _batch(make, [src], FW, FH, dtype, row_pad=pad)
        bad = np.argwhere(got[0] != exp)
        assert bad.size == 0, (f"{kind}: {len(bad)} elements differ; first (c, y, x) = {bad[0]}: byte "
                               f"{S[tuple(bad[0])]}, got {got[0][tuple(bad[0])]:#x}, expected {exp[tuple(bad[0])]:#x}")
    _orient_floats(hjd, ctx, S, dtype, norm, pad)


def _orient_floats(hjd, ctx, S, dtype, norm, pad):
    import torch
    elem = np.dtype(dtype).itemsize
    src = _dev_source(S)
    for o in (1, 6):
        dw, dh = OM.oriented_size(FW, FH, o)
        dpitch = (dw + pad) * elem
        total = 64 + 3 * dh * dpitch + 64
        buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        carrier = buf[64:64 + 3 * dh * dw * elem].view(getattr(torch, dtype)).view(3, dh, dw)
        op = hjd.Orient(ctx, [src], [(carrier, dpitch)], [o], normalize=norm)
        op.launch()
        torch.cuda.synchronize()
        op.close()
        expect = np.full(total, FILL, np.uint8)
        bits = N.apply(OM.orient(S, o), norm[0], norm[1], np.dtype(dtype)).astype(BITS[dtype])
        expect[64:64 + 3 * dh * dpitch].reshape(3 * dh, dpitch)[:, :dw * elem] = bits.reshape(3 * dh, dw).view(np.uint8)
        got = buf.cpu().numpy()
        bad = np.flatnonzero(got != expect)
        assert bad.size == 0, f"orient {o}: {bad.size} bytes differ, first at {bad[0]}: {got[bad[0]]:#x} != {expect[bad[0]]:#x}"


@pytest.mark.parametrize("kernel", ["persistent", "latency"])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("name", ["sub_a", "sub_cancel"])
def test_fused_kernels_keep_fp32_subnormals(hjd, ctx, name, dtype, kernel):
    """The case DESIGN.md s3.7 documented without a test: the fused kernels'
    float stores of fp32-subnormal results (vector and per-element stores)."""
    from test_gpu_norm_outputs import H1, W1, _check
    norm = _constants(name)
    _subnormal_premise(name, norm)
    for pad in (0, 1):
        u8 = _check(hjd, ctx, W1, H1, 1, dtype, norm, pad=pad,
                    kernel=hjd.KERNEL_LATENCY if kernel == "latency" else hjd.KERNEL_PERSISTENT)
    if name == "sub_cancel":
        assert (u8[0] == 77).any() or (u8[1] == 128).any() or (u8[2] == 255).any()   # the frame holds a cancelling byte
    else:
        assert (u8 > 0).any()
