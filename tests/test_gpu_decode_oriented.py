"""JPEG bytes -> oriented tensors: GpuDecoder.decode / decode_rgb_oriented /
decode_rgb_resized with apply_exif_orientation= and orientations=
(hjd_gdec_decode_oriented, hjd_gdec_decode_resized_oriented).  The expectation
is the numpy model (tests/orient_model.py) applied to the plain decode of the
same decoder -- whose bytes the other suites pin -- so every comparison is bit
for bit (the float planes on their bit patterns), and the resized results are
the resize models applied to the oriented plain decode."""
import functools

import numpy as np
import pytest

import norm_model as N
import orient_model as M
import resize_aa_model as RA
import resize_model as R

pytestmark = pytest.mark.gpu

BITS = {"uint8": np.uint8, "float16": np.uint16, "float32": np.uint32}
# (w, h, Pillow subsampling, gray): 4:2:0 with ragged MCUs, 4:4:4, gray, 4:2:2
SPECS = [(83, 61, 2, False), (64, 48, 0, False), (64, 48, 0, True), (80, 40, 1, False)]


@functools.lru_cache(maxsize=None)
def _files(o):
    """The four files with EXIF orientation o (None: no EXIF block); the same pixels for every o."""
    return tuple(M.pil_jpeg(w, h, sub, seed=40 + k, orientation=o, gray=gray) for k, (w, h, sub, gray) in enumerate(SPECS))


def _decoder(hjd, ctx, n=4):
    datas = _files(6)
    infos = [hjd.parse(d) for d in datas]
    return hjd.GpuDecoder(ctx, n, 2 * n * max(map(len, datas)), 2 * n * max(i.nblocks for i in infos))


def _kw(dtype):
    import torch
    if dtype == "uint8":
        return {"dtype": torch.uint8}
    return {"dtype": getattr(torch, dtype), "mean": N.IMAGENET_MEAN, "std": N.IMAGENET_STD}


def _bits(t, dtype="uint8"):
    return t.cpu().numpy().view(BITS[dtype])


def _plain(gd, dtype="uint8", scale=1, pick=range(4)):
    """The plain decode's bit patterns, one (3, H, W) array per picked file."""
    outs = gd.decode_rgb([_files(None)[k] for k in pick], scale=scale, **_kw(dtype))
    gd.sync()
    return [_bits(t, dtype) for t in outs]


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_exif_orientation_applied(hjd, ctx, dtype):
    with _decoder(hjd, ctx) as gd:
        plain = _plain(gd, dtype)
        assert [p.shape for p in plain] == [(3, h, w) for w, h, _, _ in SPECS]
        for o in range(1, 9):
            assert [hjd.exif_orientation(d) for d in _files(o)] == [o] * 4
            outs = gd.decode_rgb_oriented(list(_files(o)), apply_exif_orientation=True, **_kw(dtype))
            gd.sync()
            assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX and gd.normalize == ((1.0,) * 3, (0.0,) * 3)
            for k in range(4):
                np.testing.assert_array_equal(_bits(outs[k], dtype), M.orient(plain[k], o), err_msg=f"file {k}, o {o}")


@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_scale_2(hjd, ctx, dtype):
    pick = [0, 1, 2]   # 4:2:0, 4:4:4, gray (the scaled kernels' samplings)
    with _decoder(hjd, ctx) as gd:
        plain = _plain(gd, dtype, scale=2, pick=pick)
        assert plain[0].shape == (3, 31, 42)
        for o in range(1, 9):
            outs = gd.decode_rgb_oriented([_files(o)[k] for k in pick], scale=2, apply_exif_orientation=True, **_kw(dtype))
            gd.sync()
            for j in range(3):
                np.testing.assert_array_equal(_bits(outs[j], dtype), M.orient(plain[j], o), err_msg=f"file {pick[j]}, o {o}")


def _display_rois(o):
    """One rectangle per file on its displayed image: odd origins, the whole
    image, one pixel in the last row and column, and one touching both the
    last row and the last column."""
    sizes = [M.oriented_size(w, h, o) for w, h, _, _ in SPECS]
    (w0, h0), (w1, h1), (w2, h2), (w3, h3) = sizes
    return [(w0 - 30, h0 - 17, 30, 17), (0, 0, w1, h1), (w2 - 1, h2 - 1, 1, 1), (5, 3, 21, 30)]


@pytest.mark.parametrize("o", range(1, 9))
def test_rois_are_display_coordinates(hjd, ctx, o):
    rois = _display_rois(o)
    with _decoder(hjd, ctx) as gd:
        plain = _plain(gd)
        for dtype in ("uint8", "float32"):
            ref = plain if dtype == "uint8" else _plain(gd, dtype)
            outs = gd.decode_rgb_oriented(list(_files(o)), rois=rois, apply_exif_orientation=True, **_kw(dtype))
            gd.sync()
            for k, (x, y, w, h) in enumerate(rois):
                assert tuple(outs[k].shape) == (3, h, w)
                np.testing.assert_array_equal(_bits(outs[k], dtype), M.orient(ref[k], o)[:, y:y + h, x:x + w],
                                              err_msg=f"file {k}, o {o}, {dtype}")


def test_mixed_batch_through_decode(hjd, ctx):
    """decode() with a list of outputs; frames of orientation 1 in a mixed
    batch go through the orient kernel too (a copy) and come out as ever."""
    import torch
    orients = [1, 6, 1, 3]
    with _decoder(hjd, ctx) as gd:
        plain = _plain(gd)
        gd.set_output_format(hjd.OUT_RGB_PLANAR)
        outs = [torch.full((3,) + M.oriented_size(w, h, o)[::-1], 0xA5, dtype=torch.uint8, device="cuda")
                for (w, h, _, _), o in zip(SPECS, orients)]
        gd.decode(list(_files(None)), outs, orientations=orients)
        gd.sync()
        for k in range(4):
            np.testing.assert_array_equal(_bits(outs[k]), M.orient(plain[k], orients[k]), err_msg=f"file {k}")


def test_all_1_is_the_plain_call_and_explicit_orientations_win(hjd, ctx):
    import torch
    with _decoder(hjd, ctx) as gd:
        plain = _plain(gd)
        same = gd.decode_rgb_oriented(list(_files(1)), apply_exif_orientation=True)
        none = gd.decode_rgb_oriented(list(_files(None)), apply_exif_orientation=True)   # no EXIF block at all
        gd.sync()
        for k in range(4):
            np.testing.assert_array_equal(_bits(same[k]), plain[k])
            np.testing.assert_array_equal(_bits(none[k]), plain[k])
        # the all-1 call takes hjd_gdec_decode itself: the interleaved formats' refusal is the only difference
        gd.set_output_format(hjd.OUT_BGRX)
        from ocljpegdecoder_amd._lib import HjdError
        with pytest.raises(HjdError, match="output format"):
            gd.decode(list(_files(1)), [torch.empty((h, w), dtype=torch.int32, device="cuda") for w, h, _, _ in SPECS],
                      apply_exif_orientation=True)
        # explicit orientations override the files' tags, with and without apply_exif_orientation
        for kw in ({}, {"apply_exif_orientation": True}):
            outs = gd.decode_rgb_oriented(list(_files(6)), orientations=[8, 1, 2, 5], **kw)
            gd.sync()
            for k, o in enumerate([8, 1, 2, 5]):
                np.testing.assert_array_equal(_bits(outs[k]), M.orient(plain[k], o), err_msg=f"file {k}")
        # the equal-size rule looks at display sizes: 64x48 turned is 48x64
        out = torch.empty((2, 3, 64, 48), dtype=torch.uint8, device="cuda")
        pair = [_files(6)[1], _files(8)[2]]
        assert gd.decode_rgb_oriented(pair, out=out, apply_exif_orientation=True) is out
        gd.sync()
        np.testing.assert_array_equal(_bits(out[0]), M.orient(plain[1], 6))
        np.testing.assert_array_equal(_bits(out[1]), M.orient(plain[2], 8))


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
def test_resized_is_resize_of_orient_of_decode(hjd, ctx, dtype, antialias):
    model = RA if antialias else R
    size = (16, 24)   # (h, w)
    flips = [True, False, False, True]
    a, b = hjd.norm_constants(N.IMAGENET_MEAN, N.IMAGENET_STD)
    a, b = tuple(float(v) for v in a), tuple(float(v) for v in b)
    with _decoder(hjd, ctx) as gd:
        plain = _plain(gd)
        for o, with_rois in ((6, False), (7, True), (2, True), (5, False)):
            rois = _display_rois(o) if with_rois else None
            out = gd.decode_rgb_resized(list(_files(o)), size, flips=flips, rois=rois, antialias=antialias,
                                        apply_exif_orientation=True, **_kw(dtype))
            gd.sync()
            assert tuple(out.shape) == (4, 3) + size
            for k in range(4):
                D = M.orient(plain[k], o)
                if rois:
                    x, y, w, h = rois[k]
                    D = np.ascontiguousarray(D[:, y:y + h, x:x + w])
                np.testing.assert_array_equal(_bits(out[k], dtype),
                                              model.resize(D, size[1], size[0], flips[k], np.dtype(dtype), a, b),
                                              err_msg=f"file {k}, o {o}, rois {with_rois}")
        # a mixed batch by explicit orientations, and the all-1 batch (the plain resized call)
        for orients in ([1, 8, 3, 1], [1, 1, 1, 1]):
            out = gd.decode_rgb_resized(list(_files(None)), size, orientations=orients, antialias=antialias, **_kw(dtype))
            gd.sync()
            for k in range(4):
                np.testing.assert_array_equal(_bits(out[k], dtype),
                                              model.resize(M.orient(plain[k], orients[k]), size[1], size[0], False,
                                                           np.dtype(dtype), a, b), err_msg=f"file {k}, {orients}")


def test_growing_scratch_and_a_plain_call_in_between(hjd, ctx):
    """Oriented calls on one decoder, the later with larger crops (the scratch
    grows behind the earlier, which is not synchronised here), a plain call in
    between, and a resized oriented call (two scratch regions) after them."""
    small = [(1, 1, 3, 2), (7, 5, 4, 4), (0, 0, 1, 1), (9, 9, 2, 3)]
    size = (7, 10)
    with _decoder(hjd, ctx) as gd:
        ref = _plain(gd)
        first = gd.decode_rgb_oriented(list(_files(6)), rois=small, apply_exif_orientation=True)
        plain = gd.decode_rgb(list(_files(6)))                                  # the tag is ignored without the argument
        second = gd.decode_rgb_oriented(list(_files(6)), apply_exif_orientation=True)    # whole frames: more scratch
        third = gd.decode_rgb_resized(list(_files(7)), size, apply_exif_orientation=True)
        fourth = gd.decode_rgb_oriented(list(_files(3)), rois=small, apply_exif_orientation=True)   # fits again
        gd.sync()
        for k in range(4):
            x, y, w, h = small[k]
            np.testing.assert_array_equal(_bits(first[k]), M.orient(ref[k], 6)[:, y:y + h, x:x + w])
            np.testing.assert_array_equal(_bits(plain[k]), ref[k])
            np.testing.assert_array_equal(_bits(second[k]), M.orient(ref[k], 6))
            np.testing.assert_array_equal(_bits(third[k]), R.resize(M.orient(ref[k], 7), size[1], size[0]))
            np.testing.assert_array_equal(_bits(fourth[k]), M.orient(ref[k], 3)[:, y:y + h, x:x + w])


def test_refusals_leave_the_decoder_usable(hjd, ctx):
    import torch
    from ocljpegdecoder_amd._lib import HjdError
    with _decoder(hjd, ctx) as gd:
        ref = _plain(gd)
        datas = list(_files(6))
        for kw in ({"apply_exif_orientation": True}, {"orientations": [1, 1, 1, 1]}):
            with pytest.raises(ValueError, match="chw"):
                gd.decode_rgb_oriented(datas, layout="hwc", **kw)
            with pytest.raises(ValueError, match="chw"):
                gd.decode_rgb_resized(datas, (8, 8), layout="hwc", **kw)
        with pytest.raises(ValueError, match="orientation 9"):
            gd.decode_rgb_oriented(datas, orientations=[1, 9, 1, 1])
        with pytest.raises(ValueError, match="one orientation"):
            gd.decode_rgb_oriented(datas, orientations=[1, 6])
        gd.set_output_format(hjd.OUT_RGB_PLANAR)
        outs = [torch.empty((3, w, h), dtype=torch.uint8, device="cuda") for w, h, _, _ in SPECS]
        with pytest.raises(HjdError, match="frame 1: orientation 9") as e:
            gd.decode(datas, outs, orientations=[6, 9, 6, 6])          # refused by the library, nothing enqueued
        assert e.value.code == -1
        with pytest.raises(HjdError, match="frame 2: orientation 0"):
            gd.decode_resized(datas, torch.empty((4, 3, 8, 8), dtype=torch.uint8, device="cuda"), orientations=[6, 6, 0, 6])
        gd.set_output_format(hjd.OUT_BGRX)
        # a display rectangle outside D: 83x61 turned is 61 wide
        with pytest.raises(HjdError, match="frame 0: .*outside the 61 x 83") as e:
            gd.decode_rgb_oriented(datas, rois=[(0, 0, 62, 8)] + [(0, 0, 8, 8)] * 3, apply_exif_orientation=True)
        assert e.value.code == -1
        with pytest.raises(HjdError, match="frame 3: .*outside"):
            gd.decode_rgb_resized(datas, (8, 8), rois=[(0, 0, 8, 8)] * 3 + [(0, 73, 8, 8)], apply_exif_orientation=True)
        # the equal-size rule on display shapes: a (64, 48) batch no longer takes the turned 64x48 files
        out = torch.empty((2, 3, 48, 64), dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="image 0 is 48x64"):
            gd.decode_rgb_oriented(datas[1:3], out=out, apply_exif_orientation=True)
        with pytest.raises(HjdError, match="scaled decode"):
            gd.decode_rgb_oriented(datas, scale=2, apply_exif_orientation=True)   # the 4:2:2 file
        assert gd.scale == 1 and gd.out_format == hjd.OUT_BGRX
        outs = gd.decode_rgb_oriented(datas, apply_exif_orientation=True)
        gd.sync()
        for k in range(4):
            np.testing.assert_array_equal(_bits(outs[k]), M.orient(ref[k], 6))
