"""Host JPEG front end + streaming decode (include/hjd_host.h).

    info = parse(data)                        # headers only
    coefs, info = decode_coefs(data)          # host Huffman -> int16 zigzag coefficients
    pixels = decode_jpeg(ctx, data)           # host Huffman + fused HIP kernel, BGRX on the device
    with JpegStream(ctx, max_blocks) as st:   # Huffman workers || H2D || kernel
        st.submit(data, out_tensor); st.sync()
    gd = GpuDecoder(ctx, max_frames, max_scan_bytes, max_blocks)   # Huffman decode ON the GPU
        gd.decode([data, ...], [out_tensor, ...]); gd.sync()
    with GpuJpegStream(ctx, 32, 32 << 22, 32 * 194400) as st:      # destuff workers || H2D || GPU Huffman + pixels
        st.submit(data, out_tensor); st.sync()
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import HjdJpegInfo, HjdRect, check

_u8p = ctypes.POINTER(ctypes.c_uint8)
_i16p = ctypes.POINTER(ctypes.c_int16)

try:   # decode_rgb's default dtype (the package has loaded torch already where it is installed)
    import torch as _torch
    _UINT8 = _torch.uint8
except ImportError:
    _UINT8 = None


@dataclass
class JpegInfo:
    width: int
    height: int
    sampling: int
    restart_interval: int
    mcu_w: int
    mcu_h: int
    nblocks: int
    qt: np.ndarray            # [3][64] file (zigzag) order, per component
    qt_precision: tuple
    scan_offset: int
    process: int = 0          # 0 baseline, 1 extended sequential, 2 progressive
    single_scan: bool = True  # one interleaved sequential scan (GPU entropy decodable)

    @classmethod
    def from_c(cls, c: HjdJpegInfo) -> "JpegInfo":
        return cls(c.width, c.height, c.sampling, c.restart_interval, c.mcu_w, c.mcu_h, c.nblocks,
                   np.array(c.qt, dtype=np.int32), tuple(c.qt_precision), c.scan_offset,
                   c.process, bool(c.single_scan))


def _src(data):
    """(uint8 pointer, size, object to keep alive) of JPEG bytes, without a copy:
    bytes / bytearray / memoryview / uint8 numpy array / ctypes array.  (A copy
    per call cost a 1 MB FHD JPEG ~0.1 ms of allocation, page faults and memcpy
    on the latency path.)  The library only reads the bytes (const uint8_t*)."""
    if isinstance(data, bytes):   # the object's own buffer (c_char_p does not copy): ~1 us
        return ctypes.cast(ctypes.c_char_p(data), _u8p), len(data), data
    if isinstance(data, ctypes.Array):
        return ctypes.cast(data, _u8p), len(data), data
    a = data if isinstance(data, np.ndarray) else np.frombuffer(data, np.uint8)
    if a.dtype != np.uint8 or not a.flags.c_contiguous:
        raise ValueError("JPEG bytes must be contiguous uint8")
    return a.ctypes.data_as(_u8p), a.nbytes, a


def _buf(data):
    """The bytes' address as a uint8 pointer that keeps them alive (_src)."""
    return _src(data)[0]


def parse(data: bytes) -> JpegInfo:
    lib = _lib.load()
    info = HjdJpegInfo()
    check(lib.hjd_jpeg_parse(_buf(data), len(data), ctypes.byref(info)), "hjd_jpeg_parse")
    return JpegInfo.from_c(info)


def exif_orientation(data) -> int:
    """hjd_jpeg_orientation: the file's EXIF Orientation, 1..8 (include/hjd.h
    says what each does); 1 where the file has none or its EXIF block is
    broken.  HjdError only for bytes that are no JPEG."""
    lib = _lib.load()
    addr, size, _keep = _ptr_size(data)
    o = ctypes.c_int32(1)
    check(lib.hjd_jpeg_orientation(ctypes.cast(addr, _u8p), size, ctypes.byref(o)), "hjd_jpeg_orientation")
    return int(o.value)


def decode_coefs(data: bytes):
    """Host Huffman decode -> (int16 [nblocks][64] zigzag coefficients, JpegInfo)."""
    lib = _lib.load()
    buf = _buf(data)
    info = HjdJpegInfo()
    check(lib.hjd_jpeg_parse(buf, len(data), ctypes.byref(info)), "hjd_jpeg_parse")
    coefs = np.empty((info.nblocks, 64), np.int16)
    check(lib.hjd_jpeg_decode_coefs(buf, len(data), ctypes.byref(info), coefs.ctypes.data_as(_i16p), info.nblocks),
          "hjd_jpeg_decode_coefs")
    return coefs, JpegInfo.from_c(info)


def decode_coefs_into(data: bytes, out: np.ndarray) -> JpegInfo:
    """Host Huffman decode into a caller-provided int16 [>= nblocks][64] array
    (e.g. a pinned host tensor's numpy view, for an H2D copy straight after)."""
    lib = _lib.load()
    buf = _buf(data)
    info = HjdJpegInfo()
    check(lib.hjd_jpeg_parse(buf, len(data), ctypes.byref(info)), "hjd_jpeg_parse")
    if out.dtype != np.int16 or out.ndim != 2 or out.shape[1] != 64 or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous int16 [blocks][64] array")
    check(lib.hjd_jpeg_decode_coefs(buf, len(data), ctypes.byref(info), out.ctypes.data_as(_i16p), out.shape[0]),
          "hjd_jpeg_decode_coefs")
    return JpegInfo.from_c(info)


def decode_coefs_batch(datas: Sequence[bytes], nthreads: int = 0,
                       outs: Optional[Sequence[np.ndarray]] = None) -> List[np.ndarray]:
    """Decode many files on a host thread pool.  `outs`: one C-contiguous
    (>= nblocks, 64) int16 array per file to decode into (reused buffers: no
    allocation or first-touch page faults in the call), else new arrays."""
    lib = _lib.load()
    infos = [parse(d) for d in datas]
    if outs is None:
        outs = [np.empty((i.nblocks, 64), np.int16) for i in infos]
    else:
        outs = list(outs)
        if len(outs) != len(datas) or any(o.dtype != np.int16 or o.ndim != 2 or o.shape[1] != 64
                                          or not o.flags.c_contiguous for o in outs):
            raise ValueError("outs: one C-contiguous (n, 64) int16 array per file")
    cap = max([i.nblocks for i in infos] or [0])
    srcs = [_src(d) for d in datas]
    arr_d = (_u8p * len(srcs))(*[p for p, _, _ in srcs])
    arr_s = (ctypes.c_size_t * len(srcs))(*[n for _, n, _ in srcs])
    arr_o = (_i16p * len(outs))(*[o.ctypes.data_as(_i16p) for o in outs])
    status = (ctypes.c_int32 * len(datas))()
    # capacity checked per file (the library takes one capacity for the batch)
    for o, i in zip(outs, infos):
        if o.shape[0] < i.nblocks:
            raise ValueError(f"output of {o.shape[0]} blocks < {i.nblocks}")
    check(lib.hjd_jpeg_decode_batch(arr_d, arr_s, len(datas), arr_o, cap, nthreads, status),
          "hjd_jpeg_decode_batch")
    return outs


def _out_pitch(out, out_format: int) -> int:
    """Row pitch in bytes of an output array (tensor or numpy): its last
    dimension, except for an (..., W, 3) uint8 array taking OUT_RGB24 pixels,
    whose rows are its last two."""
    item = out.element_size() if hasattr(out, "element_size") else out.itemsize
    if out_format == 2 and out.ndim >= 3 and out.shape[-1] == 3 and item == 1:   # OUT_RGB24, (H, W, 3)
        return 3 * out.shape[-2]
    return out.shape[-1] * item


def decode_jpeg(ctx, data: bytes, stream=None, out_format: int = 0, normalize=None):
    """JPEG bytes -> device pixels (host Huffman, then the fused kernel on the
    device): an (H, W) int32 tensor of BGRX words, or with out_format=OUT_BGR24
    an (H, pitch) uint8 tensor of B,G,R bytes (pitch = (3W+3)&~3, the 24-bpp
    BMP row), with OUT_RGB24 an (H, W, 3) uint8 tensor and with OUT_RGB_PLANAR
    a (3, H, W) uint8 tensor (both contiguous); with OUT_RGB_PLANAR_F16 / _F32
    a (3, H, W) float16 / float32 tensor normalised with normalize = (a, b)
    (norm_constants(); None: a = 1, b = 0)."""
    import torch
    from .backend import (IN_Q16_ZIGZAG, OUT_BGR24, OUT_RGB24, OUT_RGB_PLANAR, OUT_RGB_PLANAR_F16, OUT_RGB_PLANAR_F32,
                          FrameSpec, Plan, default_pitch)
    if normalize is not None and out_format not in (OUT_RGB_PLANAR_F16, OUT_RGB_PLANAR_F32):
        raise ValueError("normalize needs out_format OUT_RGB_PLANAR_F16 or OUT_RGB_PLANAR_F32")
    coefs, info = decode_coefs(data)
    dev = torch.device("cuda", ctx.device)
    d_coefs = torch.from_numpy(coefs).to(dev)
    if out_format == OUT_BGR24:
        out = torch.empty((info.height, default_pitch(info.width, OUT_BGR24)), dtype=torch.uint8, device=dev)
    elif out_format == OUT_RGB24:
        out = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=dev)
    elif out_format == OUT_RGB_PLANAR:
        out = torch.empty((3, info.height, info.width), dtype=torch.uint8, device=dev)
    elif out_format in (OUT_RGB_PLANAR_F16, OUT_RGB_PLANAR_F32):
        out = torch.empty((3, info.height, info.width), device=dev,
                          dtype=torch.float16 if out_format == OUT_RGB_PLANAR_F16 else torch.float32)
    else:
        out = torch.empty((info.height, info.width), dtype=torch.int32, device=dev)
    plan = Plan(ctx, [FrameSpec(info.width, info.height, info.sampling, qt_index=(0, 1, 2), out_format=out_format)],
                IN_Q16_ZIGZAG, qtables=info.qt, normalize=normalize)
    plan.launch(d_coefs, out, stream)
    return out


class JpegStream:
    """hjd_stream: host Huffman workers -> pinned slots -> H2D -> fused kernel."""

    def __init__(self, ctx, max_blocks: int, nslots: int = 4, nthreads: int = 0, out_format: int = 0):
        self.lib = _lib.load()
        self.ctx = ctx
        h = ctypes.c_void_p()
        check(self.lib.hjd_stream_create(ctx.handle, int(max_blocks), int(nslots), int(nthreads), ctypes.byref(h)),
              "hjd_stream_create")
        self.handle = h
        self._keep = []   # bytes must stay alive until sync
        self.out_format = 0
        if out_format:
            self.set_output_format(out_format)

    def set_output_format(self, out_format: int):
        """OUT_BGRX, OUT_BGR24, OUT_RGB24 ((H, W, 3) uint8 outputs) or
        OUT_RGB_PLANAR ((3, H, W) uint8 outputs) for subsequent submits."""
        check(self.lib.hjd_stream_set_output_format(self.handle, int(out_format)), "hjd_stream_set_output_format")
        self.out_format = int(out_format)

    def submit(self, data: bytes, out, out_pitch: Optional[int] = None):
        src, size, keep = _src(data)
        self._keep.append(keep)
        if isinstance(out, int):
            ptr = out
            assert out_pitch, "out_pitch required with a raw pointer"
        else:
            if not (out.is_cuda and out.is_contiguous()):
                raise ValueError("out must be a contiguous device tensor")
            ptr = out.data_ptr()
            out_pitch = out_pitch or _out_pitch(out, self.out_format)
        check(self.lib.hjd_stream_submit(self.handle, src, size, ptr, int(out_pitch)), "hjd_stream_submit")

    def sync(self) -> dict:
        stats = (ctypes.c_int64 * 5)()
        rc = self.lib.hjd_stream_sync(self.handle, stats)
        self._keep.clear()
        check(rc, "hjd_stream_sync")
        h2d_ns, kernel_ns = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self.lib.hjd_stream_busy(self.handle, ctypes.byref(h2d_ns), ctypes.byref(kernel_ns)), "hjd_stream_busy")
        return {"images": stats[0], "pixels": stats[1], "host_decode_ns": stats[2], "h2d_bytes": stats[3],
                "kernel_launches": stats[4], "h2d_busy_ns": h2d_ns.value, "kernel_busy_ns": kernel_ns.value}

    def close(self):
        if self.handle:
            self.lib.hjd_stream_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pinned_bytes(data: bytes):
    """The bytes in a pinned (page-locked) host tensor: JPEGs submitted from
    pinned memory reach the GPU raw and are destuffed there (no host pass over
    the scan; include/hjd_host.h hjd_host_register).  Keep the tensor alive
    until the decoder's / stream's sync()."""
    import torch
    t = torch.empty(len(data), dtype=torch.uint8).pin_memory()
    t.numpy()[:] = np.frombuffer(data, np.uint8)
    return t


def _ptr_size(d):
    """(address, size) of bytes / ctypes array / (pinned) CPU uint8 tensor."""
    if isinstance(d, ctypes.Array):
        return ctypes.addressof(d), len(d), d
    if hasattr(d, "data_ptr") and hasattr(d, "is_cuda"):
        if d.is_cuda or not d.is_contiguous() or d.element_size() != 1:
            raise ValueError("JPEG tensors must be contiguous uint8 host tensors")
        return d.data_ptr(), d.numel(), d
    p, n, keep = _src(d)
    return ctypes.cast(p, ctypes.c_void_p).value or 0, n, keep


def _byte_arrays(datas):
    """(objects to keep alive, uint8* array, size_t array) of the inputs; bytes
    objects take the direct path (a decode call's Python cost is on the
    single-image latency path)."""
    ptrs, sizes, keep = [], [], []
    for d in datas:
        if isinstance(d, bytes):
            p, n, k = _src(d)
        else:
            a, n, k = _ptr_size(d)
            p = ctypes.cast(a, _u8p)
        ptrs.append(p)
        sizes.append(n)
        keep.append(k)
    return keep + ptrs, (_u8p * len(ptrs))(*ptrs), (ctypes.c_size_t * len(sizes))(*sizes)


def _stream_handle(stream):
    if stream is None:
        return None
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


class GpuDecoder:
    """hjd_gdec: JPEG bytes -> Huffman decode on the GPU -> fused pixel kernel.

    The host only parses headers and copies the scans (without byte stuffing)
    into pinned memory; the entropy decode is a verified parallel decode on
    the device, bit-identical to decode_coefs()."""

    def __init__(self, ctx, max_frames: int, max_scan_bytes: int, max_blocks: int, sub_bits: int = 0):
        self.lib = _lib.load()
        self.ctx = ctx
        h = ctypes.c_void_p()
        check(self.lib.hjd_gdec_create(ctx.handle, int(max_frames), int(max_scan_bytes), int(max_blocks),
                                       int(sub_bits), ctypes.byref(h)), "hjd_gdec_create")
        self.handle = h
        self._n = 0
        self.out_format = 0
        self.scale = 1
        self.normalize = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))   # the C default: out = float(u8)

    def set_output_format(self, out_format: int):
        """OUT_BGRX (default), OUT_BGR24, OUT_RGB24, OUT_RGB_PLANAR or the
        float planes OUT_RGB_PLANAR_F16 / _F32 (set_normalize) for the
        following decode() calls."""
        check(self.lib.hjd_gdec_set_output_format(self.handle, int(out_format)), "hjd_gdec_set_output_format")
        self.out_format = int(out_format)

    def set_normalize(self, a, b):
        """hjd_gdec_set_normalize: the constants (R, G, B triples, or scalars;
        norm_constants() makes them) of the float formats for the following
        decode() calls: out = fma(float(u8), a, b).  Default a = 1, b = 0."""
        from .backend import _norm_arrays
        ca, cb = _norm_arrays((a, b))
        check(self.lib.hjd_gdec_set_normalize(self.handle, ca, cb), "hjd_gdec_set_normalize")
        self.normalize = (tuple(ca), tuple(cb))

    def set_scale(self, scale: int):
        """Decode scale of the following decode() calls: 1 (default), 2, 4 or 8
        (hjd_gdec_set_scale): image i comes out scaled_size(W, H, scale), and
        the outputs are sized for that.  4:4:4, 4:2:0 and gray files only."""
        check(self.lib.hjd_gdec_set_scale(self.handle, int(scale)), "hjd_gdec_set_scale")
        self.scale = int(scale)

    @staticmethod
    def _orientations(datas, apply_exif_orientation, orientations):
        """The per-image orientations of a call, or None where it asks for
        none: the explicit list if given, else (apply_exif_orientation) the
        files' own tags."""
        if orientations is not None:
            if len(orientations) != len(datas):
                raise ValueError("one orientation per JPEG")
            return [int(o) for o in orientations]
        if apply_exif_orientation:
            return [exif_orientation(d) for d in datas]
        return None

    @staticmethod
    def _rects(rois, n):
        """The rois of a call as an HjdRect array, or None where it gives none."""
        if rois is None:
            return None
        if len(rois) != n:
            raise ValueError("one ROI per JPEG")
        return (HjdRect * n)(*[HjdRect(*[int(v) for v in r]) for r in rois])

    @staticmethod
    def _flips(flips, n):
        """The flips of a resized call as an int32 array, or None where it gives none."""
        if flips is None:
            return None
        if len(flips) != n:
            raise ValueError("one flip flag per JPEG")
        return (ctypes.c_int32 * n)(*[1 if f else 0 for f in flips])

    @staticmethod
    def _warp_arrays(xforms, fills, replicate, n):
        """(matrices, flags, fills or None) of a warped call as ctypes arrays."""
        from .backend import _warp_flags, _xform
        if len(xforms) != n:
            raise ValueError("one matrix per JPEG")
        mats = ((ctypes.c_int32 * 6) * n)(*[(ctypes.c_int32 * 6)(*_xform(x)) for x in xforms])
        fl = (ctypes.c_int32 * n)(*_warp_flags(replicate, n))
        fi = None
        if fills is not None:
            if len(fills) != n:
                raise ValueError("one fill colour per JPEG")
            if any(not 0 <= int(f) <= 0xFFFFFF for f in fills):
                raise ValueError("a fill colour is 0xRRGGBB")
            fi = (ctypes.c_uint32 * n)(*[int(f) for f in fills])
        return mats, fl, fi

    def _check_batch_out(self, out, n):
        """`out` of a resized or warped call: (n, 3, Ho, Wo) in the decoder's planar format."""
        if not (out.is_cuda and out.is_contiguous() and out.ndim == 4 and out.shape[0] == n and out.shape[1] == 3):
            raise ValueError(f"out must be a contiguous device tensor ({n}, 3, Ho, Wo)")
        elem = {3: 1, 5: 2, 6: 4}.get(self.out_format)   # the planar formats (any other: the library refuses)
        if elem is not None and out.element_size() != elem:
            raise ValueError(f"out's dtype {out.dtype} is not the decoder's output format ({self.out_format})")

    def decode(self, datas: Sequence[bytes], outs, stream=None, rois=None, apply_exif_orientation: bool = False,
               orientations: Optional[Sequence[int]] = None):
        """outs: contiguous device tensors, one row per image row: (H, W) int32
        (or (H, pitch/4)) for BGRX, (H, pitch) uint8 for BGR24, (H, W, 3)
        uint8 for RGB24, (3, H, W) uint8 for planar RGB, (3, H, W) float16 /
        float32 for the float planes.  rois: one (x, y, w, h)
        per image on the grid of the decoder's scale (hjd_gdec_decode_roi);
        outs are then sized (h, w).  apply_exif_orientation: every image
        comes out as displayed, permuted by its file's EXIF orientation
        (exif_orientation()); orientations: one value 1..8 per image instead,
        which wins over the files' tags (hjd_gdec_decode_oriented: the planar
        formats only; outs are sized for the oriented image, oriented_size(),
        and rois are rectangles on it).  With neither, nothing changes."""
        _keep, arr_d, arr_s = _byte_arrays(datas)
        n = len(datas)
        if len(outs) != n:
            raise ValueError("one output per JPEG")
        for o in outs:
            if not (o.is_cuda and o.is_contiguous()):
                raise ValueError("outputs must be contiguous device tensors")
        ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        pitches = (ctypes.c_int32 * n)(*[_out_pitch(o, self.out_format) for o in outs])
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        if orients is not None:
            check(self.lib.hjd_gdec_decode_oriented(self.handle, arr_d, arr_s, n, self._rects(rois, n),
                                                    (ctypes.c_int32 * n)(*orients), ptrs, pitches,
                                                    _stream_handle(stream)), "hjd_gdec_decode_oriented")
        elif rois is None:
            check(self.lib.hjd_gdec_decode(self.handle, arr_d, arr_s, n, ptrs, pitches, _stream_handle(stream)),
                  "hjd_gdec_decode")
        else:
            check(self.lib.hjd_gdec_decode_roi(self.handle, arr_d, arr_s, n, self._rects(rois, n), ptrs, pitches,
                                               _stream_handle(stream)), "hjd_gdec_decode_roi")
        self._n = n

    def decode_resized(self, datas: Sequence[bytes], out, stream=None, rois=None, flips=None,
                       apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None,
                       antialias=False):
        """hjd_gdec_decode_resized_filter: decode, crop (rois, one (x, y, w, h) per
        image on the grid of the decoder's scale, of any sizes; None: whole
        frames), resize every crop to out's (Ho, Wo) and flip where flips[i]
        is set, into `out`, a contiguous device tensor (N, 3, Ho, Wo) whose
        dtype is the decoder's current planar format's.  The crops pass
        through a scratch the decoder owns: a call that needs a larger one
        than any before waits for the previous call and reallocates.
        antialias: the exact triangle filter (RESIZE_TRIANGLE_AA) instead of
        plain bilinear; a crop dimension d going to o then needs
        d * d <= 2**21 * o.  apply_exif_orientation / orientations as
        decode(): the result is the resize of the oriented image
        (hjd_gdec_decode_resized_oriented), rois and flips applying to it."""
        _keep, arr_d, arr_s = _byte_arrays(datas)
        n = len(datas)
        self._check_batch_out(out, n)
        rects, fl = self._rects(rois, n), self._flips(flips, n)
        ho, wo = int(out.shape[2]), int(out.shape[3])
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        if orients is not None:
            check(self.lib.hjd_gdec_decode_resized_oriented(self.handle, arr_d, arr_s, n, rects,
                                                            (ctypes.c_int32 * n)(*orients), fl, out.data_ptr(), wo, ho,
                                                            wo * out.element_size(), 1 if antialias else 0,
                                                            _stream_handle(stream)),
                  "hjd_gdec_decode_resized_oriented")
        else:
            check(self.lib.hjd_gdec_decode_resized_filter(self.handle, arr_d, arr_s, n, rects, fl, out.data_ptr(), wo,
                                                          ho, wo * out.element_size(), 1 if antialias else 0,
                                                          _stream_handle(stream)),
                  "hjd_gdec_decode_resized_filter")
        self._n = n

    def decode_rgb(self, datas: Sequence[bytes], layout: str = "chw", out=None, stream=None, scale: int = 1,
                   rois=None, dtype=_UINT8, mean=None, std=None):
        """Decode to RGB tensors: layout "chw" gives (3, H, W) per image
        (OUT_RGB_PLANAR), "hwc" gives (H, W, 3) (OUT_RGB24).  dtype
        torch.uint8 (default), or torch.float16 / torch.float32
        ("chw" only): the network's input in the same launch,
        (u8 / 255 - mean) / std per channel, exactly fma(float(u8), a, b) with
        (a, b) = norm_constants(mean, std), for F16 then rounded to half
        (OUT_RGB_PLANAR_F16 / _F32); mean and std (scalars or R, G, B triples)
        default to 0 and 1, and need a float dtype.  scale 2, 4 or 8
        decodes at 1/scale (H and W below are then scaled_size's; the
        decoder's own scale is restored afterwards).  Without `out`,
        one new device tensor per image is returned as a list.  With `out`, a
        contiguous device tensor of that dtype (N, 3, H, W) ("chw") or (N, H, W, 3)
        ("hwc"), image i is decoded into out[i] and `out` is returned;
        ValueError if an image's size differs from it.  rois: one (x, y, w, h)
        per image on the (scaled) grid; tensors are sized per ROI, and with
        `out` every ROI's (h, w) must equal out's while the files' own sizes
        may differ.  Asynchronous like
        decode(): call sync() before reading.  The decoder's output format
        and constants are restored afterwards.  decode_rgb_resized() resizes
        images of different sizes into one batch, decode_rgb_oriented()
        applies the files' EXIF orientation."""
        return self._decode_rgb(datas, layout, out, stream, scale, rois, dtype, mean, std, None)

    def decode_rgb_oriented(self, datas: Sequence[bytes], layout: str = "chw", out=None, stream=None, scale: int = 1,
                            rois=None, dtype=_UINT8, mean=None, std=None, apply_exif_orientation: bool = True,
                            orientations: Optional[Sequence[int]] = None):
        """decode_rgb with every image as displayed: permuted on the GPU
        (hjd_gdec_decode_oriented) by its file's EXIF orientation
        (apply_exif_orientation, the default here), or by orientations, one
        value 1..8 per image, which wins over the files' tags (rot90-style
        augmentation).  H, W, the rois and the equal-size rule of `out` refer
        to the oriented image (oriented_size()).  layout "chw" only ("hwc"
        with either is a ValueError: oriented output is planar).  With
        apply_exif_orientation=False and no orientations it is decode_rgb.
        (decode_rgb itself keeps its parameter list; decode(),
        decode_resized() and decode_rgb_resized() take the two arguments
        directly.)"""
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        if orients is not None and layout == "hwc":
            raise ValueError('oriented output is planar: layout must be "chw"')
        return self._decode_rgb(datas, layout, out, stream, scale, rois, dtype, mean, std, orients)

    def _decode_rgb(self, datas, layout, out, stream, scale, rois, dtype, mean, std, orients):
        """decode_rgb / decode_rgb_oriented (orients: None, or one orientation per image)."""
        import torch
        from .backend import oriented_size, scaled_size
        chw, dtype, fmt, norm = self._rgb_format(layout, dtype, mean, std)
        infos = []
        for d in datas:   # headers only; any input decode() takes (bytes, arrays, pinned tensors)
            addr, size, _k = _ptr_size(d)
            c = HjdJpegInfo()
            check(self.lib.hjd_jpeg_parse(ctypes.cast(addr, _u8p), size, ctypes.byref(c)), "hjd_jpeg_parse")
            infos.append(JpegInfo.from_c(c))
        sizes = [scaled_size(i.width, i.height, scale) for i in infos]   # (W', H')
        if orients is not None:   # as displayed
            for k, o in enumerate(orients):
                if not 1 <= o <= 8:
                    raise ValueError(f"image {k}: orientation {o} is outside 1..8")
            sizes = [oriented_size(w, h, o) for (w, h), o in zip(sizes, orients)]
        if rois is not None:
            if len(rois) != len(infos):
                raise ValueError("one ROI per JPEG")
            sizes = [(int(r[2]), int(r[3])) for r in rois]
        if out is None:
            dev = torch.device("cuda", self.ctx.device)
            outs = [torch.empty((3, h, w) if chw else (h, w, 3), dtype=dtype, device=dev) for w, h in sizes]
        else:
            if not (out.is_cuda and out.is_contiguous() and out.dtype == dtype and out.ndim == 4
                    and out.shape[1 if chw else 3] == 3):
                raise ValueError(f"out must be a contiguous {dtype} device tensor (N, 3, H, W) or (N, H, W, 3)")
            if out.shape[0] != len(infos):
                raise ValueError(f"out holds {out.shape[0]} images, {len(infos)} JPEGs given")
            oh, ow = (out.shape[2], out.shape[3]) if chw else (out.shape[1], out.shape[2])
            for k, (w, h) in enumerate(sizes):
                if (h, w) != (oh, ow):
                    raise ValueError(f"image {k} is {w}x{h}" + (f" at scale {scale}" if scale != 1 else "") +
                                     f", out is {ow}x{oh}")
            outs = [out[k] for k in range(len(infos))]
        return self._with_settings(scale, fmt, norm,
                                   lambda: self.decode(datas, outs, stream, rois=rois, orientations=orients),
                                   outs if out is None else out)

    def _with_settings(self, scale, fmt, norm, call, result):
        """Run `call` at this scale, output format and constants (norm, or
        None: untouched), restore the decoder's own and return `result`."""
        prev, prev_scale, prev_norm = self.out_format, self.scale, self.normalize
        self.set_scale(scale)
        self.set_output_format(fmt)
        try:
            if norm is not None:
                self.set_normalize(*norm)
            call()
        finally:
            self.set_output_format(prev)
            self.set_scale(prev_scale)
            if norm is not None:
                self.set_normalize(*prev_norm)
        return result

    @staticmethod
    def _rgb_format(layout, dtype, mean, std):
        """(chw, dtype, output format, constants or None) of decode_rgb's arguments."""
        import torch
        from .backend import OUT_RGB24, OUT_RGB_PLANAR, OUT_RGB_PLANAR_F16, OUT_RGB_PLANAR_F32, norm_constants
        if layout not in ("chw", "hwc"):
            raise ValueError('layout must be "chw" or "hwc"')
        chw = layout == "chw"
        if dtype is None:
            dtype = torch.uint8
        if dtype not in (torch.uint8, torch.float16, torch.float32):
            raise ValueError("dtype must be torch.uint8, torch.float16 or torch.float32")
        if dtype == torch.uint8:
            if mean is not None or std is not None:
                raise ValueError("mean and std need dtype torch.float16 or torch.float32")
            return chw, dtype, (OUT_RGB_PLANAR if chw else OUT_RGB24), None
        if not chw:
            raise ValueError('the float dtypes are planar: layout must be "chw"')
        return chw, dtype, (OUT_RGB_PLANAR_F16 if dtype == torch.float16 else OUT_RGB_PLANAR_F32), \
            norm_constants(mean, std)

    def decode_rgb_resized(self, datas: Sequence[bytes], size, flips=None, layout: str = "chw", out=None, stream=None,
                           scale: int = 1, rois=None, dtype=_UINT8, mean=None, std=None,
                           apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None,
                           antialias=False):
        """decode_rgb with size = (h, w): every image -- its ROI, of any size,
        or its whole (scaled) frame -- is resized to h x w on the GPU
        (decode_resized: bilinear, no antialiasing, where resize_scale() gives
        the `scale` that keeps the reduction within 2x; with antialias=True
        the exact triangle filter of interpolate(antialias=True), for any
        reduction) and mirrored horizontally
        where flips[i] is set, and ONE (N, 3, h, w) tensor of the dtype comes
        back: `out` if given (a contiguous device tensor of exactly that shape
        and dtype), else a new one.  dtype, mean, std, scale and rois as
        decode_rgb; layout "chw" only ("hwc" is a ValueError: the batch is
        planar).  apply_exif_orientation / orientations as decode_rgb: the
        oriented image is what is cropped (rois), resized and flipped.
        Asynchronous; the decoder's format, scale and constants are
        restored afterwards."""
        import torch
        chw, dtype, fmt, norm = self._rgb_format(layout, dtype, mean, std)
        if not chw:
            raise ValueError('a resized batch is planar: layout must be "chw"')
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        out = self._batch_result(len(datas), size, dtype, out)
        return self._with_settings(scale, fmt, norm,
                                   lambda: self.decode_resized(datas, out, stream, rois=rois, flips=flips,
                                                               antialias=antialias, orientations=orients), out)

    def decode_warped(self, datas: Sequence[bytes], out, xforms, stream=None, fills=None, replicate=False,
                      apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None):
        """hjd_gdec_decode_warped: decode and sample every image through its
        own affine map xforms[i] (six Q16 ints, the inverse map output ->
        source pixel indices; warp_xform() makes them) into `out`, a
        contiguous device tensor (N, 3, Ho, Wo) whose dtype is the decoder's
        current planar format's.  The matrices address the grid of the
        decoder's scale, and the displayed image where apply_exif_orientation
        or orientations (as decode()) give an orientation: it is folded into
        the matrix, at no launch.  fills: one colour 0xRRGGBB per image for
        taps outside it (default 0); replicate (one value, or one per image):
        the nearest pixel of the image instead.  Only the rectangle of each
        frame the warp reads is decoded, into the scratch decode_resized()
        uses, under its growth rule."""
        _keep, arr_d, arr_s = _byte_arrays(datas)
        n = len(datas)
        self._check_batch_out(out, n)
        mats, fl, fi = self._warp_arrays(xforms, fills, replicate, n)
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        ho, wo = int(out.shape[2]), int(out.shape[3])
        check(self.lib.hjd_gdec_decode_warped(self.handle, arr_d, arr_s, n, mats,
                                              (ctypes.c_int32 * n)(*orients) if orients is not None else None, fl, fi,
                                              out.data_ptr(), wo, ho, wo * out.element_size(), _stream_handle(stream)),
              "hjd_gdec_decode_warped")
        self._n = n

    def decode_rgb_warped(self, datas: Sequence[bytes], size, xforms, fill=0, replicate=False, out=None, stream=None,
                          scale: int = 1, dtype=_UINT8, mean=None, std=None, apply_exif_orientation: bool = False,
                          orientations: Optional[Sequence[int]] = None):
        """decode_rgb with size = (h, w) and one affine map per image
        (decode_warped): rotation, shear, zoom, flips and translation on the
        GPU, and ONE (N, 3, h, w) tensor of the dtype comes back: `out` if
        given (a contiguous device tensor of exactly that shape and dtype),
        else a new one.  xforms[i]: six Q16 ints as warp_xform(W, H, w, h,
        angle, zoom, ...) returns them for the image's size (W, H) at `scale`
        -- as displayed, where an orientation applies.  fill: one colour
        0xRRGGBB, or one per image, for what lies outside the image;
        replicate: its border pixels instead.  No antialiasing: keep the zoom
        within 2 by decoding at a `scale`.  dtype, mean, std and scale as
        decode_rgb; the batch is planar.  Asynchronous; the decoder's format,
        scale and constants are restored afterwards."""
        import torch
        _chw, dtype, fmt, norm = self._rgb_format("chw", dtype, mean, std)
        size = (int(size[0]), int(size[1]))
        if min(size) < 1:
            raise ValueError(f"size must be (h, w) with h, w >= 1, got {size}")
        if len(xforms) != len(datas):
            raise ValueError("one matrix per JPEG")
        fills = list(fill) if isinstance(fill, (list, tuple)) else [fill] * len(datas)
        shape = (len(datas), 3) + size
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=torch.device("cuda", self.ctx.device))
        elif not (out.is_cuda and out.is_contiguous() and out.dtype == dtype and tuple(out.shape) == shape):
            raise ValueError(f"out must be a contiguous {dtype} device tensor {shape}")
        return self._with_settings(scale, fmt, norm,
                                   lambda: self.decode_warped(datas, out, xforms, stream, fills=fills,
                                                              replicate=replicate,
                                                              apply_exif_orientation=apply_exif_orientation,
                                                              orientations=orientations), out)

    @staticmethod
    def _colors(colors, n):
        """The colour records of a call as an int32[n][21] array."""
        from .backend import _color
        if colors is None or len(colors) != n:
            raise ValueError("one colour record (21 ints, color_matrix()) per JPEG")
        return ((ctypes.c_int32 * 21) * n)(*[(ctypes.c_int32 * 21)(*_color(c)) for c in colors])

    def _batch_result(self, n, size, dtype, out):
        """The (n, 3, h, w) tensor of a resized or warped call: `out` checked, or a new one."""
        import torch
        size = (int(size[0]), int(size[1]))
        if min(size) < 1:
            raise ValueError(f"size must be (h, w) with h, w >= 1, got {size}")
        shape = (n, 3) + size
        if out is None:
            return torch.empty(shape, dtype=dtype, device=torch.device("cuda", self.ctx.device))
        if not (out.is_cuda and out.is_contiguous() and out.dtype == dtype and tuple(out.shape) == shape):
            raise ValueError(f"out must be a contiguous {dtype} device tensor {shape}")
        return out

    def decode_rgb_resized_color(self, datas: Sequence[bytes], size, flips=None, layout: str = "chw", out=None,
                                 stream=None, scale: int = 1, rois=None, dtype=_UINT8, mean=None, std=None,
                                 apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None,
                                 antialias=False, colors=None):
        """decode_rgb_resized with a colour record per image
        (hjd_gdec_decode_resized_color): colors[i], 21 ints as color_matrix()
        returns them (brightness, contrast, saturation, hue, gray, invert), is
        applied to image i after the resize, on the GPU, before the dtype's
        normalisation: out[i] = normalise(color(resize(orient(decode)))).  A
        record's means (contrast about the mean) are those of the resized
        image.  Every other parameter as decode_rgb_resized.  Records that
        are all COLOR_IDENTITY make it exactly decode_rgb_resized."""
        chw, dtype, fmt, norm = self._rgb_format(layout, dtype, mean, std)
        if not chw:
            raise ValueError('a resized batch is planar: layout must be "chw"')
        n = len(datas)
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        cols = self._colors(colors, n)
        out = self._batch_result(n, size, dtype, out)
        fl = self._flips(flips, n)

        def call():
            _keep, arr_d, arr_s = _byte_arrays(datas)
            ho, wo = int(out.shape[2]), int(out.shape[3])
            check(self.lib.hjd_gdec_decode_resized_color(
                self.handle, arr_d, arr_s, n, self._rects(rois, n),
                (ctypes.c_int32 * n)(*orients) if orients is not None else None, fl, cols, out.data_ptr(), wo, ho,
                wo * out.element_size(), 1 if antialias else 0, _stream_handle(stream)), "hjd_gdec_decode_resized_color")
            self._n = n
        return self._with_settings(scale, fmt, norm, call, out)

    def decode_rgb_warped_color(self, datas: Sequence[bytes], size, xforms, fill=0, replicate=False, out=None,
                                stream=None, scale: int = 1, dtype=_UINT8, mean=None, std=None,
                                apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None,
                                colors=None):
        """decode_rgb_warped with a colour record per image
        (hjd_gdec_decode_warped_color): out[i] = normalise(color(warp(decode))),
        colors as decode_rgb_resized_color takes them (the means are those of
        the warped image, its fill included).  Every other parameter as
        decode_rgb_warped."""
        _chw, dtype, fmt, norm = self._rgb_format("chw", dtype, mean, std)
        n = len(datas)
        mats, fl, fi = self._warp_arrays(xforms, list(fill) if isinstance(fill, (list, tuple)) else [fill] * n,
                                         replicate, n)
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        cols = self._colors(colors, n)
        out = self._batch_result(n, size, dtype, out)

        def call():
            _keep, arr_d, arr_s = _byte_arrays(datas)
            ho, wo = int(out.shape[2]), int(out.shape[3])
            check(self.lib.hjd_gdec_decode_warped_color(
                self.handle, arr_d, arr_s, n, mats, (ctypes.c_int32 * n)(*orients) if orients is not None else None,
                fl, fi, cols, out.data_ptr(), wo, ho, wo * out.element_size(), _stream_handle(stream)),
                "hjd_gdec_decode_warped_color")
            self._n = n
        return self._with_settings(scale, fmt, norm, call, out)

    @staticmethod
    def _tones(curves, modes, n):
        """The tone curves of a call: the numpy records (kept alive by the caller) and their hjd_tone_curve pointer."""
        from .backend import _tone_curves
        recs = _tone_curves(curves, modes, n)
        return recs, recs.ctypes.data_as(ctypes.POINTER(_lib.HjdToneCurve))

    def decode_rgb_resized_tone(self, datas: Sequence[bytes], size, flips=None, layout: str = "chw", out=None,
                                stream=None, scale: int = 1, rois=None, dtype=_UINT8, mean=None, std=None,
                                apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None,
                                antialias=False, colors=None, curves=None, modes=None):
        """decode_rgb_resized with a tone curve per image
        (hjd_gdec_decode_resized_tone): image i goes through the table
        curves[i] (uint8 (3, 256) or (256,), tone_curve() makes them: solarize,
        posterize, gamma, invert), behind the data curve modes[i] --
        TONE_TABLE (none), TONE_AUTOCONTRAST or TONE_EQUALIZE, built on the GPU
        from the resized image's own histogram -- after the resize and after
        colors[i] where colors (as decode_rgb_resized_color takes them) is
        given, before the dtype's normalisation:
        out[i] = normalise(table(data_curve(color(resize(orient(decode)))))).
        curves and modes may each be None (TONE_IDENTITY, TONE_TABLE) or one
        value for all images.  Every other parameter as decode_rgb_resized.
        Curves that are all TONE_IDENTITY in TONE_TABLE make it exactly the
        call without them."""
        chw, dtype, fmt, norm = self._rgb_format(layout, dtype, mean, std)
        if not chw:
            raise ValueError('a resized batch is planar: layout must be "chw"')
        n = len(datas)
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        cols = self._colors(colors, n) if colors is not None else None
        recs, tones = self._tones(curves, modes, n)
        out = self._batch_result(n, size, dtype, out)
        fl = self._flips(flips, n)

        def call():
            _keep, arr_d, arr_s = _byte_arrays(datas)
            ho, wo = int(out.shape[2]), int(out.shape[3])
            check(self.lib.hjd_gdec_decode_resized_tone(
                self.handle, arr_d, arr_s, n, self._rects(rois, n),
                (ctypes.c_int32 * n)(*orients) if orients is not None else None, fl, cols, tones, out.data_ptr(), wo,
                ho, wo * out.element_size(), 1 if antialias else 0, _stream_handle(stream)),
                "hjd_gdec_decode_resized_tone")
            self._n = n
        return self._with_settings(scale, fmt, norm, call, out)

    def decode_rgb_warped_tone(self, datas: Sequence[bytes], size, xforms, fill=0, replicate=False, out=None,
                               stream=None, scale: int = 1, dtype=_UINT8, mean=None, std=None,
                               apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None,
                               colors=None, curves=None, modes=None):
        """decode_rgb_warped with a tone curve per image
        (hjd_gdec_decode_warped_tone):
        out[i] = normalise(table(data_curve(color(warp(decode))))), curves,
        modes and colors as decode_rgb_resized_tone takes them (a histogram is
        that of the warped image, its fill included).  Every other parameter
        as decode_rgb_warped."""
        _chw, dtype, fmt, norm = self._rgb_format("chw", dtype, mean, std)
        n = len(datas)
        mats, fl, fi = self._warp_arrays(xforms, list(fill) if isinstance(fill, (list, tuple)) else [fill] * n,
                                         replicate, n)
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        cols = self._colors(colors, n) if colors is not None else None
        recs, tones = self._tones(curves, modes, n)
        out = self._batch_result(n, size, dtype, out)

        def call():
            _keep, arr_d, arr_s = _byte_arrays(datas)
            ho, wo = int(out.shape[2]), int(out.shape[3])
            check(self.lib.hjd_gdec_decode_warped_tone(
                self.handle, arr_d, arr_s, n, mats, (ctypes.c_int32 * n)(*orients) if orients is not None else None,
                fl, fi, cols, tones, out.data_ptr(), wo, ho, wo * out.element_size(), _stream_handle(stream)),
                "hjd_gdec_decode_warped_tone")
            self._n = n
        return self._with_settings(scale, fmt, norm, call, out)

    @staticmethod
    def _convs(convs, n):
        """The filters of a call: the numpy records (kept alive by the caller) and their hjd_conv_filter pointer."""
        from .backend import _conv_filters
        recs = _conv_filters(convs, n)
        return recs, recs.ctypes.data_as(ctypes.POINTER(_lib.HjdConvFilter))

    def decode_rgb_resized_aug(self, datas: Sequence[bytes], size, flips=None, layout: str = "chw", out=None,
                               stream=None, scale: int = 1, rois=None, dtype=_UINT8, mean=None, std=None,
                               apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None,
                               antialias=False, colors=None, convs=None, curves=None, modes=None):
        """decode_rgb_resized with every optional stage
        (hjd_gdec_decode_resized_aug): a colour record (colors, as
        decode_rgb_resized_color takes them), a filter (convs: one record per
        image or one for all, as conv_sharpness(), conv_gaussian() and
        conv_unsharp() make them) and a tone curve (curves and modes, as
        decode_rgb_resized_tone takes them) per image, in that order -- jitter,
        blur, solarize -- before the dtype's normalisation:
        out[i] = normalise(tone(conv(color(resize(orient(decode)))))).
        A filter's borders are those of the resized image, a histogram is that
        of the filtered one.  Each of colors, convs and (curves, modes) may be
        None: no such stage.  Every other parameter as decode_rgb_resized;
        with all three None, or the identity, it is exactly that call."""
        chw, dtype, fmt, norm = self._rgb_format(layout, dtype, mean, std)
        if not chw:
            raise ValueError('a resized batch is planar: layout must be "chw"')
        n = len(datas)
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        cols = self._colors(colors, n) if colors is not None else None
        crecs, cvs = self._convs(convs, n) if convs is not None else (None, None)
        trecs, tones = self._tones(curves, modes, n) if curves is not None or modes is not None else (None, None)
        out = self._batch_result(n, size, dtype, out)
        fl = self._flips(flips, n)

        def call():
            _keep, arr_d, arr_s = _byte_arrays(datas)
            ho, wo = int(out.shape[2]), int(out.shape[3])
            check(self.lib.hjd_gdec_decode_resized_aug(
                self.handle, arr_d, arr_s, n, self._rects(rois, n),
                (ctypes.c_int32 * n)(*orients) if orients is not None else None, fl, cols, cvs, tones, out.data_ptr(), wo,
                ho, wo * out.element_size(), 1 if antialias else 0, _stream_handle(stream)),
                "hjd_gdec_decode_resized_aug")
            self._n = n
        return self._with_settings(scale, fmt, norm, call, out)

    def decode_rgb_warped_aug(self, datas: Sequence[bytes], size, xforms, fill=0, replicate=False, out=None,
                              stream=None, scale: int = 1, dtype=_UINT8, mean=None, std=None,
                              apply_exif_orientation: bool = False, orientations: Optional[Sequence[int]] = None,
                              colors=None, convs=None, curves=None, modes=None):
        """decode_rgb_warped with every optional stage
        (hjd_gdec_decode_warped_aug):
        out[i] = normalise(tone(conv(color(warp(decode))))), colors, convs,
        curves and modes as decode_rgb_resized_aug takes them (a filter's
        borders are those of the warped image, its fill included).  Every
        other parameter as decode_rgb_warped."""
        _chw, dtype, fmt, norm = self._rgb_format("chw", dtype, mean, std)
        n = len(datas)
        mats, fl, fi = self._warp_arrays(xforms, list(fill) if isinstance(fill, (list, tuple)) else [fill] * n,
                                         replicate, n)
        orients = self._orientations(datas, apply_exif_orientation, orientations)
        cols = self._colors(colors, n) if colors is not None else None
        crecs, cvs = self._convs(convs, n) if convs is not None else (None, None)
        trecs, tones = self._tones(curves, modes, n) if curves is not None or modes is not None else (None, None)
        out = self._batch_result(n, size, dtype, out)

        def call():
            _keep, arr_d, arr_s = _byte_arrays(datas)
            ho, wo = int(out.shape[2]), int(out.shape[3])
            check(self.lib.hjd_gdec_decode_warped_aug(
                self.handle, arr_d, arr_s, n, mats, (ctypes.c_int32 * n)(*orients) if orients is not None else None,
                fl, fi, cols, cvs, tones, out.data_ptr(), wo, ho, wo * out.element_size(), _stream_handle(stream)),
                "hjd_gdec_decode_warped_aug")
            self._n = n
        return self._with_settings(scale, fmt, norm, call, out)

    def decode_coefs(self, datas: Sequence[bytes], coefs, stream=None) -> List[int]:
        """Entropy decode only into `coefs` (int16 device tensor, [blocks][64]);
        returns each frame's first block."""
        _keep, arr_d, arr_s = _byte_arrays(datas)
        n = len(datas)
        if not (coefs.is_cuda and coefs.is_contiguous() and coefs.element_size() == 2):
            raise ValueError("coefs must be a contiguous int16 device tensor")
        offs = (ctypes.c_int64 * n)()
        check(self.lib.hjd_gdec_decode_coefs(self.handle, arr_d, arr_s, n, coefs.data_ptr(), offs,
                                             _stream_handle(stream)), "hjd_gdec_decode_coefs")
        self._n = n
        return list(offs)

    def last_bytes(self) -> dict:
        """Bytes of the most recent decode call: scan bytes the host CPU
        read + wrote (0 when every scan was destuffed on the GPU) and bytes
        moved host -> device."""
        hb, h2d = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self.lib.hjd_gdec_last_bytes(self.handle, ctypes.byref(hb), ctypes.byref(h2d)), "hjd_gdec_last_bytes")
        return {"host_scan_bytes": hb.value, "h2d_bytes": h2d.value}

    def debug_state(self) -> dict:
        """Test hook: the state the decoder carries from call to call
        (struct hjd_gdec_debug_state, include/hjd_host.h) as a dict of ints."""
        st = _lib.HjdGdecDebugState()
        check(self.lib.hjd_debug_gdec_state(self.handle, ctypes.byref(st)), "hjd_debug_gdec_state")
        return {name: int(getattr(st, name)) for name, _ in st._fields_}

    def debug_set_chain_epoch(self, value: int):
        """Test hook: sets the host's look-back tag counter (not the words on
        the device); the next call advances it as ever.  Refused while a call
        is pending."""
        check(self.lib.hjd_debug_gdec_set_chain_epoch(self.handle, int(value)), "hjd_debug_gdec_set_chain_epoch")

    def sync(self, raise_on_error: bool = True) -> List[int]:
        """Wait for the last call; per-frame status words (include/hjd_host.h:
        bit 0 HJD_GDEC_SEQUENTIAL is informational, a sequential verification
        or a chain repair; bits 1-2 are errors and raise unless
        raise_on_error is False)."""
        status = (ctypes.c_int32 * max(self._n, 1))()
        rc = self.lib.hjd_gdec_sync(self.handle, status)
        if raise_on_error:
            check(rc, "hjd_gdec_sync")
        return list(status)[: self._n]

    def close(self):
        if self.handle:
            self.lib.hjd_gdec_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuJpegStream:
    """hjd_gstream: worker threads parse/destuff JPEGs into pinned batches;
    each batch is Huffman-decoded and converted to BGRX on the GPU."""

    def __init__(self, ctx, max_frames: int, max_scan_bytes: int, max_blocks: int, nslots: int = 3,
                 nthreads: int = 0, out_format: int = 0):
        self.lib = _lib.load()
        self.ctx = ctx
        h = ctypes.c_void_p()
        check(self.lib.hjd_gstream_create(ctx.handle, int(max_frames), int(max_scan_bytes), int(max_blocks),
                                          int(nslots), int(nthreads), ctypes.byref(h)), "hjd_gstream_create")
        self.handle = h
        self._keep = []
        self.out_format = 0
        if out_format:
            self.set_output_format(out_format)

    def set_output_format(self, out_format: int):
        """OUT_BGRX, OUT_BGR24, OUT_RGB24 ((H, W, 3) uint8 outputs) or
        OUT_RGB_PLANAR ((3, H, W) uint8 outputs), between sync() and the next
        submit."""
        check(self.lib.hjd_gstream_set_output_format(self.handle, int(out_format)), "hjd_gstream_set_output_format")
        self.out_format = int(out_format)

    def submit(self, data: bytes, out, out_pitch: Optional[int] = None):
        """out: contiguous device tensor, or a (pinned) host tensor / numpy
        array -- then the pixels are copied back to host memory (D2H sink)."""
        addr, size, keep = _ptr_size(data)
        self._keep.append(keep)
        src = ctypes.cast(addr, _u8p)
        if isinstance(out, np.ndarray):
            if not out.flags.c_contiguous:
                raise ValueError("out must be C-contiguous")
            self._keep.append(out)
            pitch = out_pitch or _out_pitch(out, self.out_format)
            check(self.lib.hjd_gstream_submit_host(self.handle, src, size, out.ctypes.data, int(pitch)),
                  "hjd_gstream_submit_host")
            return
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
        out_pitch = out_pitch or _out_pitch(out, self.out_format)
        if out.is_cuda:
            check(self.lib.hjd_gstream_submit(self.handle, src, size, out.data_ptr(), int(out_pitch)),
                  "hjd_gstream_submit")
        else:
            self._keep.append(out)
            check(self.lib.hjd_gstream_submit_host(self.handle, src, size, out.data_ptr(), int(out_pitch)),
                  "hjd_gstream_submit_host")

    def sync(self) -> dict:
        stats = (ctypes.c_int64 * 5)()
        rc = self.lib.hjd_gstream_sync(self.handle, stats)
        self._keep.clear()
        check(rc, "hjd_gstream_sync")
        hb = ctypes.c_int64(0)
        check(self.lib.hjd_gstream_host_bytes(self.handle, ctypes.byref(hb)), "hjd_gstream_host_bytes")
        return {"images": stats[0], "pixels": stats[1], "host_prep_ns": stats[2], "h2d_bytes": stats[3],
                "batches": stats[4], "host_scan_bytes": hb.value}

    def close(self):
        if self.handle:
            self.lib.hjd_gstream_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bmp_header(width: int, height: int, bpp: int = 32) -> bytes:
    """The reference's 54-byte BMP header (src/decoder.cpp:372-394): 32 bpp,
    top-down; bpp=24 gives the 24-bpp counterpart (rows padded to 4 bytes)."""
    lib = _lib.load()
    h = (ctypes.c_uint8 * 54)()
    if bpp == 32:
        check(lib.hjd_bmp_header(int(width), int(height), h), "hjd_bmp_header")
    elif bpp == 24:
        check(lib.hjd_bmp_header_bgr24(int(width), int(height), h), "hjd_bmp_header_bgr24")
    else:
        raise ValueError("bpp must be 32 or 24")
    return bytes(h)


def bmp_bytes(pixels, width: Optional[int] = None) -> bytes:
    """A BMP file from decoded pixels, as the reference writes it from the GPU
    path: an (H, W) array of BGRX words gives the reference's 32-bpp file; an
    (H, pitch) uint8 array of BGR24 rows (pitch = (3W+3)&~3, as decode_jpeg
    returns with OUT_BGR24) gives the 24-bpp file (width W required)."""
    a = np.ascontiguousarray(pixels)
    if a.dtype == np.uint8:
        if width is None or a.shape[1] != (3 * width + 3) & ~3:
            raise ValueError("BGR24 rows need width and pitch (3*width+3)&~3")
        return bmp_header(width, a.shape[0], 24) + a.tobytes()
    a = a.view(np.uint32)
    return bmp_header(a.shape[1], a.shape[0]) + a.astype("<u4").tobytes()


def emulate_entropy(data: bytes, sub_bits: int = 0):
    """Test hook: the GPU entropy algorithm run on the host (no GPU) ->
    (int16 [nblocks][64] coefficients, status bits)."""
    lib = _lib.load()
    info = parse(data)
    coefs = np.zeros((info.nblocks, 64), np.int16)
    status = ctypes.c_int32(0)
    check(lib.hjd_debug_entropy_emulate(_buf(data), len(data), int(sub_bits), coefs.ctypes.data_as(_i16p),
                                        info.nblocks, ctypes.byref(status)), "hjd_debug_entropy_emulate")
    return coefs, status.value
