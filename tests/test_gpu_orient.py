"""Orient (hjd_orient_*) alone against the numpy model (tests/orient_model.py),
bit for bit: all eight orientations on random bytes at the sizes where a tiled
transpose goes wrong, aligned and unaligned sources and outputs independently,
the three output formats (the floats through tests/norm_model.py), every case
one launch over items of all orientations and sizes, into a filled buffer that
is compared as a whole -- so no byte outside an output, its row padding
included, may change."""
import functools

import numpy as np
import pytest

import norm_model as N
import orient_model as M

pytestmark = pytest.mark.gpu

T = 128   # hjd::kOrientTile
FILL = 0xA5
# (w, h): single pixels and lines, around one tile, more than one tile with ragged
# edges, one with no dword straddling an edge (both multiples of 4) and partial tiles
SIZES = [(1, 1), (1, 9), (9, 1), (T - 1, T + 1), (T, T), (T + 1, 2 * T + 2), (2 * T + 3, T - 1), (130, 67), (136, 132)]
DTYPES = ["uint8", "float16", "float32"]
BITS = {"uint8": np.uint8, "float16": np.uint16, "float32": np.uint32}
SRC_CASES = ["aligned", "base+1", "pitch+1"]
DST_CASES = ["aligned", "base+1", "pitch+1"]   # in elements


def _up(x, a):
    return (x + a - 1) // a * a


@functools.lru_cache(maxsize=None)
def _norm_table(a, b, dtype):
    """norm_model's (3, 256) table of bit patterns, built once per dtype."""
    return N.table(a, b, np.dtype(dtype))


def _norm_bits(D, a, b, dtype):
    """norm_model.apply through the cached table."""
    t = _norm_table(tuple(float(v) for v in a), tuple(float(v) for v in b), dtype)
    return np.stack([t[c][D[c]] for c in range(3)])


@functools.lru_cache(maxsize=None)
def _sources(case):
    """One byte buffer with every (size, orientation) item's source planes in it:
    (buffer, [(offset, pitch, w, h, o, S)])."""
    rng = np.random.default_rng(7)
    items, off = [], 0
    for w, h in SIZES:
        for o in range(1, 9):
            pitch = _up(w, 4) if case != "pitch+1" else _up(w, 4) + 1
            base = _up(off, 64) + (1 if case == "base+1" else 0)
            items.append((base, pitch, w, h, o))
            off = base + 3 * h * pitch
    buf = rng.integers(0, 256, off + 64, dtype=np.uint8)
    out = []
    for base, pitch, w, h, o in items:
        S = buf[base:base + 3 * h * pitch].reshape(3, h, pitch)[:, :, :w].copy()
        out.append((base, pitch, w, h, o, S))
    buf.setflags(write=False)
    return buf, out


@pytest.mark.parametrize("dst_case", DST_CASES)
@pytest.mark.parametrize("src_case", SRC_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_orientations_one_launch(hjd, ctx, dtype, src_case, dst_case):
    import torch
    elem = np.dtype(dtype).itemsize
    src_np, items = _sources(src_case)
    src = torch.from_numpy(src_np.copy()).cuda()
    a, b = hjd.norm_constants(N.IMAGENET_MEAN, N.IMAGENET_STD)
    # the outputs' places: 64 bytes of guard band before, between and after them
    places, off = [], 64
    for base, pitch, w, h, o, S in items:
        dw, dh = M.oriented_size(w, h, o)
        dpitch = _up(dw, 4) * elem + (elem if dst_case == "pitch+1" else 0)
        dbase = _up(off, 64) + (elem if dst_case == "base+1" else 0)
        places.append((dbase, dpitch, dw, dh))
        off = dbase + 3 * dh * dpitch + 64
    expect = np.full(off, FILL, np.uint8)
    out = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
    srcs, outs = [], []
    for (base, pitch, w, h, o, S), (dbase, dpitch, dw, dh) in zip(items, places):
        D = M.orient(S, o)
        bits = D if dtype == "uint8" else _norm_bits(D, a, b, dtype)
        rows = bits.astype(BITS[dtype]).reshape(3 * dh, dw).view(np.uint8)          # (3 dh, dw * elem)
        view = expect[dbase:dbase + 3 * dh * dpitch].reshape(3 * dh, dpitch)
        view[:, :dw * elem] = rows
        srcs.append((src[base:base + 3 * h * w].view(3, h, w), pitch))
        carrier = out[dbase:dbase + 3 * dh * dw * elem].view(getattr(torch, dtype)).view(3, dh, dw)
        outs.append((carrier, dpitch))
    orientations = [it[4] for it in items]
    with_norm = None if dtype == "uint8" else (a, b)
    op = hjd.Orient(ctx, srcs, outs, orientations, normalize=with_norm)
    op.launch()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    op.close()
    if not np.array_equal(got, expect):   # name the first item that differs, or the guard band
        for k, ((base, pitch, w, h, o, S), (dbase, dpitch, dw, dh)) in enumerate(zip(items, places)):
            lo, hi = dbase, dbase + 3 * dh * dpitch
            assert np.array_equal(got[lo:hi], expect[lo:hi]), f"item {k}: {w}x{h} orientation {o}"
        raise AssertionError("bytes outside the outputs were written")


def test_default_constants_and_contiguous_tensors(hjd, ctx):
    """Plain (3, h, w) tensors on both sides; floats without normalize are float(u8)."""
    import torch
    rng = np.random.default_rng(3)
    S = rng.integers(0, 256, (3, 67, 130), dtype=np.uint8)
    src = torch.from_numpy(S).cuda()
    for dtype in DTYPES:
        outs = [torch.zeros((3,) + M.oriented_size(130, 67, o)[::-1], dtype=getattr(torch, dtype), device="cuda")
                for o in range(1, 9)]
        op = hjd.Orient(ctx, [src] * 8, outs, list(range(1, 9)))
        op.launch()
        torch.cuda.synchronize()
        op.close()
        for o in range(1, 9):
            np.testing.assert_array_equal(outs[o - 1].cpu().numpy(), M.orient(S, o).astype(dtype), err_msg=f"{dtype} {o}")


def test_python_refusals(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    src = torch.zeros((3, 5, 7), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="oriented image"):
        hjd.Orient(ctx, [src], [torch.zeros((3, 5, 7), dtype=torch.uint8, device="cuda")], [6])
    with pytest.raises(HjdError, match="orientation 9"):
        hjd.Orient(ctx, [src], [torch.zeros((3, 5, 7), dtype=torch.uint8, device="cuda")], [9])
    with pytest.raises(HjdError, match="overlaps"):
        hjd.Orient(ctx, [src], [src], [1])
    with pytest.raises(ValueError, match="one output"):
        hjd.Orient(ctx, [src], [], [1])
    op = hjd.Orient(ctx, [src], [torch.zeros((3, 7, 5), dtype=torch.uint8, device="cuda")], [5])
    with pytest.raises(HjdError, match="output format"):
        op.set_normalize((1.0,) * 3, (0.0,) * 3)   # a byte-format object
    op.close()
