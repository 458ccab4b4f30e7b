"""Python host API over the C ABI (include/hjd.h).

PyTorch is used only as plumbing: device memory (tensors), streams.  All pixel
work runs in the HIP kernels of libhjd.so.
"""
from __future__ import annotations

import contextlib
import ctypes
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import HjdFrame, HjdRect, check

YUV444 = 0
YUV420 = 1  # == the reference's ColorSpace::YUV411 (src/macro.h:114-119), H2V2
OTHER = 2
YUV422 = 3  # extension (Y H2V1), include/hjd.h
GRAY = 4    # extension (one component), include/hjd.h
YUV411_H4V1 = 5  # extension (Y H4V1: true 4:1:1, not the reference's "YUV411"), include/hjd.h
YUV440 = 6  # extension (Y H1V2), include/hjd.h

# sampling -> (MCU px width, MCU px height, blocks per MCU, luma blocks per MCU)
_GEOM = {YUV444: (8, 8, 3, 1), YUV420: (16, 16, 6, 4), YUV422: (16, 8, 4, 2), GRAY: (8, 8, 1, 1),
         YUV411_H4V1: (32, 8, 6, 4), YUV440: (8, 16, 4, 2)}

IN_Q16_ZIGZAG = 0
IN_I32_NATURAL = 1

KERNEL_AUTO, KERNEL_PERSISTENT, KERNEL_LATENCY = 0, 1, 2   # include/hjd.h hjd_kernel_mode

OUT_BGRX = 0    # 4 B/px: B, G, R, 0 (the reference's RGB32 / 32-bpp BMP rows)
OUT_BGR24 = 1   # 3 B/px: B, G, R (extension: 24-bpp BMP rows)
OUT_RGB24 = 2   # 3 B/px: R, G, B interleaved (extension: an (H, W, 3) uint8 array)
OUT_RGB_PLANAR = 3   # three uint8 planes R, G, B at pitch * height (extension: a (3, H, W) uint8 array)
# extensions: three planes R, G, B of normalised half / float elements, out = fma(float(u8), a[c], b[c])
OUT_RGB_PLANAR_F16 = 5   # a (3, H, W) float16 array (4 is not a format)
OUT_RGB_PLANAR_F32 = 6   # a (3, H, W) float32 array
OUT_BYTES = {OUT_BGRX: 4, OUT_BGR24: 3, OUT_RGB24: 3, OUT_RGB_PLANAR: 3,
             OUT_RGB_PLANAR_F16: 6, OUT_RGB_PLANAR_F32: 12}   # bytes per pixel overall
_ROW_BYTES = {OUT_BGRX: 4, OUT_BGR24: 3, OUT_RGB24: 3, OUT_RGB_PLANAR: 1,
              OUT_RGB_PLANAR_F16: 2, OUT_RGB_PLANAR_F32: 4}   # bytes per pixel within a row
_PLANAR = (OUT_RGB_PLANAR, OUT_RGB_PLANAR_F16, OUT_RGB_PLANAR_F32)


def default_pitch(width: int, out_format: int = OUT_BGRX) -> int:
    """Tightest legal row pitch: bytes of one row rounded up to 4 (BGRX,
    BGR24); the RGB formats take any pitch, so theirs is the contiguous one
    (3*width, planar: width; float planar: 2*width or 4*width)."""
    if out_format in (OUT_RGB24,) + _PLANAR:
        return _ROW_BYTES[out_format] * width
    return (OUT_BYTES[out_format] * width + 3) & ~3


def out_rows(height: int, out_format: int) -> int:
    """Rows of `pitch` bytes a frame occupies (planar: three planes)."""
    return 3 * height if out_format in _PLANAR else height


def norm_constants(mean=None, std=None):
    """(a, b): the float formats' constants as two float32 triples (R, G, B),
    out = fma(float(u8), a, b).  Without arguments a = fp32(1/255), b = 0
    (ToTensor); with mean and std (scalars or triples, on the [0, 1] scale)
    a_c = fp32(1 / (255 std_c)), b_c = fp32(-mean_c / std_c), each computed in
    float64 and rounded once."""
    m = np.broadcast_to(np.asarray(0.0 if mean is None else mean, dtype=np.float64), (3,))
    s = np.broadcast_to(np.asarray(1.0 if std is None else std, dtype=np.float64), (3,))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = (1.0 / (255.0 * s)).astype(np.float32)
        b = (-m / s).astype(np.float32) + np.float32(0)   # no -0 from mean = 0
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError(f"normalisation constants are not finite: mean={mean}, std={std}")
    return a, b


def _norm_arrays(normalize):
    """normalize = (a, b) as two ctypes float[3] arrays (scalars broadcast)."""
    a, b = normalize
    a = np.broadcast_to(np.asarray(a, dtype=np.float32), (3,))
    b = np.broadcast_to(np.asarray(b, dtype=np.float32), (3,))
    return (ctypes.c_float * 3)(*a.tolist()), (ctypes.c_float * 3)(*b.tolist())


def frame_check(spec, input_format: int = 0, scale: int = 1):
    """hjd_frame_check: raise HjdError unless a plan of `scale` would take this
    FrameSpec's geometry and output layout.  Host only."""
    c = spec.to_c(scale)
    r = HjdRect(*[int(v) for v in spec.roi]) if spec.roi is not None else None
    check(_lib.load().hjd_frame_check(ctypes.byref(c), int(input_format), int(scale),
                                      ctypes.byref(r) if r is not None else None), "hjd_frame_check")


def mcu_geometry(width: int, height: int, sampling: int):
    """(mcu_w, mcu_h, blocks_per_mcu, (mcu_px_w, mcu_px_h)) -- src/decoder.cpp:161-192."""
    if sampling not in _GEOM:
        raise ValueError(f"unsupported sampling {sampling}")
    pw, ph, bpm, _ = _GEOM[sampling]
    return (width - 1) // pw + 1, (height - 1) // ph + 1, bpm, (pw, ph)


def block_components(sampling: int, nblocks: int) -> np.ndarray:
    """Component (0 Y, 1 Cb, 2 Cr) of each block of an MCU-major block list."""
    _, _, bpm, nluma = _GEOM[sampling]
    return np.array(([0] * nluma + [1, 2][: bpm - nluma]) * (nblocks // bpm), dtype=np.int64)


def scaled_size(width: int, height: int, scale: int):
    """(W', H') = (ceil(width / scale), ceil(height / scale)) of a scaled
    decode (hjd_scaled_size; scale 1, 2, 4 or 8).  Host only."""
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.load().hjd_scaled_size(int(width), int(height), int(scale), ctypes.byref(w), ctypes.byref(h)),
          "hjd_scaled_size")
    return w.value, h.value


def roi_geometry(width: int, height: int, sampling: int, scale: int, roi):
    """(tasks, blocks) of the ROI (x, y, w, h) on the output grid of a
    width x height source of `sampling` at `scale` (hjd_roi_geometry): the
    pixel kernel's tasks and the coefficient blocks they read.  An invalid
    rectangle raises HjdError.  Host only."""
    r = HjdRect(*[int(v) for v in roi])
    tasks, blocks = ctypes.c_int64(0), ctypes.c_int64(0)
    check(_lib.load().hjd_roi_geometry(int(width), int(height), int(sampling), int(scale), ctypes.byref(r),
                                       ctypes.byref(tasks), ctypes.byref(blocks)), "hjd_roi_geometry")
    return tasks.value, blocks.value


def frame_blocks(width: int, height: int, sampling: int) -> int:
    mw, mh, bpm, _ = mcu_geometry(width, height, sampling)
    return mw * mh * bpm


def device_count() -> int:
    lib = _lib.load()
    n = ctypes.c_int32(0)
    check(lib.hjd_device_count(ctypes.byref(n)), "hjd_device_count")
    return n.value


def _stream_ptr(stream) -> Optional[int]:
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


class Context:
    """One device (hjd_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        check(self.lib.hjd_ctx_create(device, ctypes.byref(h)), "hjd_ctx_create")
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            self.lib.hjd_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- kernels outside a plan -------------------------------------------------
    def idct_blocks(self, d_in, d_out, nblocks: int, stream=None):
        """IDCT only (int32 natural in -> int32 samples), tensors on this device."""
        for t in (d_in, d_out):
            if not (t.is_cuda and t.is_contiguous() and t.element_size() == 4 and t.numel() >= 64 * nblocks):
                raise ValueError("idct_blocks needs contiguous int32 device tensors of >= 64*nblocks elements")
        check(self.lib.hjd_idct_blocks(self.handle, d_in.data_ptr(), d_out.data_ptr(), int(nblocks),
                                       _stream_ptr(stream)), "hjd_idct_blocks")

    def debug_csc(self, y, u, v, out, mode: int = 0, stream=None):
        for t in (y, u, v, out):
            if not (t.is_cuda and t.is_contiguous() and t.element_size() == 4 and t.numel() >= y.numel()):
                raise ValueError("debug_csc needs contiguous 4-byte device tensors of equal length")
        check(self.lib.hjd_debug_csc(self.handle, y.data_ptr(), u.data_ptr(), v.data_ptr(), out.data_ptr(),
                                     y.numel(), mode, _stream_ptr(stream)), "hjd_debug_csc")

    def debug_csc_exhaustive(self, out, mode: int = 0, stream=None):
        assert out.numel() * out.element_size() >= 4 << 27
        check(self.lib.hjd_debug_csc_exhaustive(self.handle, out.data_ptr(), mode, _stream_ptr(stream)),
              "hjd_debug_csc_exhaustive")

    def debug_rw_mix(self, src, dst, read_kib: int, write_kib: int, units_per_wave: int = 2, flags: int = 3,
                     stream=None) -> int:
        """The box's streaming ceiling kernel (hjd_debug_rw_mix): one launch;
        returns the bytes it moves (read + written)."""
        for t in (src, dst):
            if not (t.is_cuda and t.is_contiguous()):
                raise ValueError("debug_rw_mix needs contiguous device tensors")
        units = ctypes.c_int64(0)
        check(self.lib.hjd_debug_rw_mix(self.handle, src.data_ptr(), dst.data_ptr(), src.numel() * src.element_size(),
                                        dst.numel() * dst.element_size(), int(read_kib), int(write_kib),
                                        int(units_per_wave), int(flags), _stream_ptr(stream), ctypes.byref(units)),
              "hjd_debug_rw_mix")
        return units.value * (read_kib + write_kib) * 1024

    def clock_probe(self, out, nsamples: int, interval_ticks: int, stream=None):
        """Launch the clock probe (hjd_debug_clock_probe) writing 2*nsamples
        int64 words into `out` (a device tensor); see clock_summary()."""
        if not (out.is_cuda and out.is_contiguous() and out.element_size() == 8 and out.numel() >= 2 * nsamples):
            raise ValueError("clock_probe needs a contiguous int64 device tensor of >= 2*nsamples elements")
        check(self.lib.hjd_debug_clock_probe(self.handle, out.data_ptr(), int(nsamples), int(interval_ticks),
                                             _stream_ptr(stream)), "hjd_debug_clock_probe")

    def d16_gather(self):
        """(probe_zeroes, selected) of hjd_debug_d16_gather for this device."""
        a, b = ctypes.c_int32(-1), ctypes.c_int32(-1)
        check(self.lib.hjd_debug_d16_gather(self.device, ctypes.byref(a), ctypes.byref(b)), "hjd_debug_d16_gather")
        return bool(a.value), bool(b.value)


@dataclass
class FrameSpec:
    width: int
    height: int
    sampling: int
    coef_offset: int = 0          # in blocks
    out_offset: int = 0           # bytes
    out_pitch: int = 0            # bytes (0 -> default_pitch(width, out_format); of the scaled width in a scaled plan);
    #                               at most 2**28 (HJD_MAX_OUT_PITCH, include/hjd.h)
    qt_index: Sequence[int] = field(default_factory=lambda: (0, 1, 1))
    out_format: int = OUT_BGRX
    roi: Optional[Sequence[int]] = None   # (x, y, w, h) on the output grid: the frame comes out cropped to it

    @property
    def pitch(self) -> int:
        return self.out_pitch or default_pitch(self.roi[2] if self.roi is not None else self.width, self.out_format)

    def out_size(self, scale: int = 1):
        """(W, H) of what the frame writes: the ROI's, else the (scaled) frame's."""
        if self.roi is not None:
            return int(self.roi[2]), int(self.roi[3])
        return (self.width, self.height) if scale == 1 else scaled_size(self.width, self.height, scale)

    def to_c(self, scale: int = 1) -> HjdFrame:
        """The C record; width and height stay the source's, out_pitch = 0
        resolves against the size scaled by `scale`."""
        f = HjdFrame()
        f.coef_offset = self.coef_offset
        f.out_offset = self.out_offset
        f.width = self.width
        f.height = self.height
        f.out_pitch = self.pitch if scale == 1 or self.roi is not None else (
            self.out_pitch or default_pitch(scaled_size(self.width, self.height, scale)[0], self.out_format))
        f.sampling = self.sampling
        for i in range(3):
            f.qt_index[i] = int(self.qt_index[i])
        f.out_format = self.out_format
        return f


class Plan:
    """A validated batch of frames with its device-side frame table (hjd_plan)."""

    def __init__(self, ctx: Context, frames: Sequence[FrameSpec], input_format: int = IN_Q16_ZIGZAG,
                 qtables: Optional[np.ndarray] = None, scale: int = 1, normalize=None):
        """normalize = (a, b): the constants of a float-format plan
        (set_normalize; norm_constants() makes them).
        scale 2, 4 or 8: a scaled plan (hjd_plan_create_scaled).  Frames
        carry the source size; every frame comes out scaled_size(W, H, scale)
        and out_pitch (0: default_pitch of the scaled width) refers to that.
        A plan is a ROI plan (hjd_plan_create_roi) when any frame has a roi;
        frames without one take their whole output grid."""
        self.ctx = ctx
        self.lib = ctx.lib
        self.frames = list(frames)
        if scale != 1:
            scaled_size(1, 1, scale)   # a bad scale raises here, before any frame is sized with it
        arr = (HjdFrame * max(1, len(self.frames)))(*[f.to_c(scale) for f in self.frames])
        if qtables is not None:
            q = np.ascontiguousarray(qtables, dtype=np.int32).reshape(-1, 64)
            qp, nq = q.ctypes.data_as(_lib.c_i32p), q.shape[0]
        else:
            q, qp, nq = None, None, 0
        h = ctypes.c_void_p()
        if any(f.roi is not None for f in self.frames):
            whole = [(0, 0) + f.out_size(scale) for f in self.frames]
            rects = (HjdRect * len(self.frames))(*[HjdRect(*[int(v) for v in (f.roi if f.roi is not None else r)])
                                                   for f, r in zip(self.frames, whole)])
            check(self.lib.hjd_plan_create_roi(ctx.handle, arr, len(self.frames), input_format, qp, nq, int(scale),
                                               rects, ctypes.byref(h)), "hjd_plan_create_roi")
        elif scale == 1:
            check(self.lib.hjd_plan_create(ctx.handle, arr, len(self.frames), input_format, qp, nq, ctypes.byref(h)),
                  "hjd_plan_create")
        else:
            check(self.lib.hjd_plan_create_scaled(ctx.handle, arr, len(self.frames), input_format, qp, nq, int(scale),
                                                  ctypes.byref(h)), "hjd_plan_create_scaled")
        self.handle = h
        self.scale = self.lib.hjd_plan_scale(h)
        self.has_roi = bool(self.lib.hjd_plan_has_roi(h))
        self.input_format = input_format
        self.tasks = self.lib.hjd_plan_tasks(h)
        self.pixels = self.lib.hjd_plan_pixels(h)
        self.coef_bytes = self.lib.hjd_plan_coef_bytes(h)
        # extents the kernel will touch: validated against the tensors at launch
        self.coef_elem_bytes = 2 if input_format == IN_Q16_ZIGZAG else 4
        self.coef_elems_needed = max([64 * (f.coef_offset + frame_blocks(f.width, f.height, f.sampling))
                                      for f in self.frames] or [0])
        self.out_bytes_needed = 0
        for f, c in zip(self.frames, arr):   # on the ROI's or the scaled size (scale 1: the frame's own)
            sw, sh = f.out_size(scale)
            self.out_bytes_needed = max(self.out_bytes_needed, f.out_offset + (out_rows(sh, f.out_format) - 1) *
                                        c.out_pitch + _ROW_BYTES[f.out_format] * sw)
        if normalize is not None:
            self.set_normalize(*normalize)

    def set_normalize(self, a, b):
        """hjd_plan_set_normalize: the constants (R, G, B triples, or scalars)
        of an OUT_RGB_PLANAR_F16 / _F32 plan for the launches that follow:
        out = fma(float(u8), a, b); a new plan has a = 1, b = 0."""
        ca, cb = _norm_arrays((a, b))
        check(self.lib.hjd_plan_set_normalize(self.handle, ca, cb), "hjd_plan_set_normalize")

    def _check_tensor(self, t, what, elem_bytes, nbytes_needed):
        if isinstance(t, int):
            return t                       # raw device pointer: caller's responsibility
        if not t.is_cuda:
            raise ValueError(f"{what} must be a device tensor")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        if elem_bytes and t.element_size() != elem_bytes:
            raise ValueError(f"{what} must have {elem_bytes}-byte elements for this plan, got {t.dtype}")
        if t.numel() * t.element_size() < nbytes_needed:
            raise ValueError(f"{what} too small: {t.numel() * t.element_size()} B < {nbytes_needed} B")
        if t.device.index != self.ctx.device:
            raise ValueError(f"{what} is on {t.device}, plan is for device {self.ctx.device}")
        return t.data_ptr()

    def set_kernel(self, mode: int):
        """KERNEL_AUTO (default), KERNEL_PERSISTENT or KERNEL_LATENCY; identical outputs."""
        check(self.lib.hjd_plan_set_kernel(self.handle, int(mode)), "hjd_plan_set_kernel")

    def set_chunk(self, tasks: int):
        """Pin the persistent kernel's tasks per wave (hjd_plan_set_chunk); 0 = default."""
        check(self.lib.hjd_plan_set_chunk(self.handle, int(tasks)), "hjd_plan_set_chunk")

    def set_variant(self, variant: int):
        """Kernel variant bits (tuning/A-B only; outputs are identical)."""
        check(self.lib.hjd_plan_set_variant(self.handle, int(variant)), "hjd_plan_set_variant")

    def launch(self, coefs, out, stream=None, grid_blocks: int = 0):
        """Enqueue the fused kernel; coefs/out are device tensors (or raw pointers)."""
        cp = self._check_tensor(coefs, "coefs", self.coef_elem_bytes, self.coef_elems_needed * self.coef_elem_bytes)
        op = self._check_tensor(out, "out", 0, self.out_bytes_needed)
        check(self.lib.hjd_plan_launch(self.handle, cp, op, _stream_ptr(stream), grid_blocks), "hjd_plan_launch")

    def autotune(self, coefs, out, stream=None, rounds: int = 2):
        """hjd_plan_autotune: time the launch shapes on these buffers and keep
        the fastest for later launches; returns (tasks_per_wave, variant).
        The choice is cached per process by kernel and batch geometry
        (include/hjd.h): on a cache hit nothing is launched and `out` is NOT
        written -- call launch() for a decode (launch_shape()["autotune_cached"]
        tells which happened)."""
        cp = self._check_tensor(coefs, "coefs", self.coef_elem_bytes, self.coef_elems_needed * self.coef_elem_bytes)
        op = self._check_tensor(out, "out", 0, self.out_bytes_needed)
        tpw, var = ctypes.c_int32(0), ctypes.c_int32(0)
        check(self.lib.hjd_plan_autotune(self.handle, cp, op, _stream_ptr(stream), int(rounds), ctypes.byref(tpw),
                                         ctypes.byref(var)), "hjd_plan_autotune")
        return tpw.value, var.value

    def launch_shape(self) -> dict:
        """hjd_plan_launch_shape: the shape the next default launch uses, and
        what the last autotune did (launches made, cache hit)."""
        r = _lib.HjdLaunchShape()
        check(self.lib.hjd_plan_launch_shape(self.handle, ctypes.byref(r)), "hjd_plan_launch_shape")
        d = {n: getattr(r, n) for n, _ in r._fields_}
        d["kernel"] = {KERNEL_PERSISTENT: "persistent", KERNEL_LATENCY: "latency"}.get(d["kernel"], d["kernel"])
        return d

    def launch_stages(self, stages: int, coefs, out, stream=None, grid_blocks: int = 0):
        """Timing-only launch with kernel stages skipped (hjd_debug_plan_launch_stages;
        80 memory only, 4 no stores, ...): the output is WRONG by design."""
        cp = self._check_tensor(coefs, "coefs", self.coef_elem_bytes, self.coef_elems_needed * self.coef_elem_bytes)
        op = self._check_tensor(out, "out", 0, self.out_bytes_needed)
        check(self.lib.hjd_debug_plan_launch_stages(self.handle, int(stages), cp, op, _stream_ptr(stream),
                                                    int(grid_blocks)),
              "hjd_debug_plan_launch_stages")

    def close(self):
        if self.handle:
            self.lib.hjd_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


RESIZE_FLIP_H = 1   # hjd_resize_item.flags bit 0
RESIZE_BILINEAR, RESIZE_TRIANGLE_AA = 0, 1   # the resize's filter (include/hjd.h)
_DTYPE_FORMATS = {"torch.uint8": OUT_RGB_PLANAR, "torch.float16": OUT_RGB_PLANAR_F16,
                  "torch.float32": OUT_RGB_PLANAR_F32}


def resize_scale(src_w: int, src_h: int, out_w: int, out_h: int) -> int:
    """The decode scale to resize from: the largest s in (8, 4, 2, 1) that
    leaves a src_w x src_h region (at scale 1) at least out_w x out_h, that is
    ceil(src_w / s) >= out_w and ceil(src_h / s) >= out_h; 1 if none does (an
    upscale).  The box means of the scaled decode then do the reduction beyond
    2x that plain bilinear would alias on.  Pure Python."""
    for s in (8, 4, 2):
        if -(-int(src_w) // s) >= out_w and -(-int(src_h) // s) >= out_h:
            return s
    return 1


def _planes(s, i, what, uint8=False):
    """(tensor, pitch in bytes) of a (3, h, w) tensor or a (tensor, pitch) pair."""
    t, p = s if isinstance(s, (tuple, list)) else (s, None)
    if not (t.is_cuda and t.ndim == 3 and t.shape[0] == 3 and (not uint8 or t.element_size() == 1)):
        raise ValueError(f"{what} {i} must be a (3, h, w) {'uint8 ' if uint8 else ''}device tensor")
    if p is None:   # contiguous, or a [..., :w] view of wider rows
        row = t.stride(1)
        if t.stride(2) != 1 or row < t.shape[2] or t.stride(0) != t.shape[1] * row:
            raise ValueError(f"{what} {i} must be contiguous, a [..., :w] view of wider rows, or come with its pitch")
        p = row * t.element_size()
    return t, p


def _source(s, i):
    """_planes of a source of Orient or Warp: uint8."""
    t, p = _planes(s, i, "source")
    if t.element_size() != 1:
        raise ValueError(f"source {i} must be a (3, h, w) uint8 device tensor")
    return t, p


def _batch_out(out, n):
    """(out_format, Wo, Ho, pitch in bytes) of the (N, 3, Ho, Wo) output of n sources (Resize, Warp)."""
    if not (out.is_cuda and out.ndim == 4 and out.shape[1] == 3 and str(out.dtype) in _DTYPE_FORMATS):
        raise ValueError("out must be a uint8 / float16 / float32 device tensor (N, 3, Ho, Wo)")
    ho, wo = int(out.shape[2]), int(out.shape[3])
    row = out.stride(2)   # elements between rows: Wo, or more for a [..., :Wo] view of wider rows
    if out.stride(3) != 1 or row < wo or out.stride(1) != ho * row or (n > 1 and out.stride(0) != 3 * ho * row):
        raise ValueError("out must be contiguous, or a [..., :Wo] view of a contiguous (N, 3, Ho, P) tensor")
    if out.shape[0] != n:
        raise ValueError(f"out holds {out.shape[0]} images, {n} sources given")
    return _DTYPE_FORMATS[str(out.dtype)], wo, ho, row * out.element_size()


class _Stage:
    """The handle of an hjd_resize / hjd_orient / hjd_warp object and the calls
    every kind has; _prefix is the kind's C prefix."""
    _prefix = ""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib
        self.handle = None
        self._keep = []

    def _call(self, name, *args):
        check(getattr(self.lib, f"{self._prefix}_{name}")(*args), f"{self._prefix}_{name}")

    def _create(self, name, normalize, *args):
        h = ctypes.c_void_p()
        self._call(name, self.ctx.handle, *args, ctypes.byref(h))
        self.handle = h
        if normalize is not None:
            self.set_normalize(*normalize)

    def set_normalize(self, a, b):
        """hjd_<kind>_set_normalize: out = fma(float(u8), a, b) for the launches that follow."""
        self._call("set_normalize", self.handle, *_norm_arrays((a, b)))

    def launch(self, stream=None):
        """Enqueue the object's kernels (asynchronous)."""
        self._call("launch", self.handle, _stream_ptr(stream))

    def close(self):
        if self.handle:
            getattr(self.lib, f"{self._prefix}_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Resize(_Stage):
    """hjd_resize: N planar uint8 RGB images of different sizes -> one
    (N, 3, Ho, Wo) batch in one launch (include/hjd.h: bilinear, half-pixel
    centres, 11-bit integer weights, no antialiasing; sizes 1..16384).
    antialias=True takes the exact triangle filter instead
    (RESIZE_TRIANGLE_AA: what interpolate(antialias=True) computes, two
    launches through an intermediate the object owns, so the launches of one
    object must be ordered, e.g. on one stream; a source dimension d going to
    o needs d * d <= 2**21 * o)."""
    _prefix = "hjd_resize"

    def __init__(self, ctx: Context, srcs, out, flips=None, normalize=None, antialias=False):
        """srcs: N device tensors (3, h, w) uint8 (contiguous, or a [..., :w]
        view of wider rows), or (tensor, pitch) pairs: 3 * h rows of `pitch`
        bytes from the tensor's data_ptr, whose shape (3, h, w) gives h and w.
        out: a device tensor (N, 3, Ho, Wo) of uint8, float16 or float32,
        contiguous or a [..., :Wo] view of wider rows.  flips: N truthy
        values, image i mirrored horizontally where set.  normalize = (a, b):
        the float dtypes' constants (set_normalize; default a = 1, b = 0).
        antialias: the filter, RESIZE_TRIANGLE_AA if true."""
        super().__init__(ctx)
        n = len(srcs)
        self.out_format, wo, ho, pitch = _batch_out(out, n)
        if flips is not None and len(flips) != n:
            raise ValueError("one flip flag per source")
        items = (_lib.HjdResizeItem * max(1, n))()
        for i, s in enumerate(srcs):
            t, sp = _planes(s, i, "source", uint8=True)
            self._keep.append(t)
            items[i] = _lib.HjdResizeItem(t.data_ptr(), out[i].data_ptr(), int(t.shape[2]), int(t.shape[1]), int(sp),
                                          RESIZE_FLIP_H if flips is not None and flips[i] else 0)
        self.out = out
        self.filter = RESIZE_TRIANGLE_AA if antialias else RESIZE_BILINEAR
        self._create("create_filter", normalize, items, n, wo, ho, pitch, self.out_format, self.filter)

    def launch_pass(self, which: int, stream=None):
        """Timing only (hjd_debug_resize_launch_pass): one launch of an
        antialias=True object, 0 the horizontal kernel, 1 the vertical one."""
        check(self.lib.hjd_debug_resize_launch_pass(self.handle, int(which), _stream_ptr(stream)),
              "hjd_debug_resize_launch_pass")


def oriented_size(width: int, height: int, orientation: int):
    """(W, H) of the displayed image of a width x height stored one under EXIF
    orientation 1..8 (include/hjd.h): swapped for 5..8.  Pure Python."""
    o = int(orientation)
    if not 1 <= o <= 8:
        raise ValueError(f"orientation {orientation} is outside 1..8")
    return (int(height), int(width)) if o >= 5 else (int(width), int(height))


def oriented_roi(width: int, height: int, orientation: int, roi):
    """hjd_orient_roi: the (x, y, w, h) rectangle on the stored width x height
    frame (already scaled) that holds the pixels of `roi`, a rectangle on the
    displayed image.  HjdError for a rectangle outside it."""
    lib = _lib.load()
    d, s = _lib.HjdRect(*[int(v) for v in roi]), _lib.HjdRect()
    check(lib.hjd_orient_roi(int(width), int(height), int(orientation), ctypes.byref(d), ctypes.byref(s)),
          "hjd_orient_roi")
    return (s.x, s.y, s.w, s.h)


class Orient(_Stage):
    """hjd_orient: N planar uint8 RGB images of different sizes, each permuted
    by its EXIF orientation (1..8; include/hjd.h has the table) into its own
    output, in one launch.  A pure permutation of bytes; the float dtypes are
    fma(float(u8), a, b) of the permuted bytes."""
    _prefix = "hjd_orient"

    def __init__(self, ctx: Context, srcs, outs, orientations, normalize=None):
        """srcs: N device tensors (3, h, w) uint8 (contiguous, or a [..., :w]
        view of wider rows), or (tensor, pitch) pairs as Resize takes them.
        outs: N device tensors of one dtype (uint8, float16 or float32), out i
        shaped (3, H, W) with (W, H) = oriented_size(w, h, orientations[i]),
        contiguous or a [..., :W] view of wider rows, or (tensor, pitch)
        pairs: 3 * H rows of `pitch` bytes from the tensor's data_ptr.
        normalize = (a, b): the float dtypes' constants."""
        super().__init__(ctx)
        n = len(srcs)
        if len(outs) != n or len(orientations) != n:
            raise ValueError("one output and one orientation per source")
        items = (_lib.HjdOrientItem * max(1, n))()
        fmt = None
        for i, (s, d) in enumerate(zip(srcs, outs)):
            t, sp = _source(s, i)
            u, dp = _planes(d, i, "output")
            if str(u.dtype) not in _DTYPE_FORMATS or (fmt is not None and _DTYPE_FORMATS[str(u.dtype)] != fmt):
                raise ValueError("outputs must be uint8 / float16 / float32 device tensors of one dtype")
            fmt = _DTYPE_FORMATS[str(u.dtype)]
            w, h = int(t.shape[2]), int(t.shape[1])
            if 1 <= int(orientations[i]) <= 8 and (int(u.shape[2]), int(u.shape[1])) != oriented_size(
                    w, h, orientations[i]):
                raise ValueError(f"output {i} is {u.shape[2]}x{u.shape[1]}, the oriented image "
                                 f"{'x'.join(map(str, oriented_size(w, h, orientations[i])))}")
            self._keep += [t, u]
            items[i] = _lib.HjdOrientItem(t.data_ptr(), u.data_ptr(), w, h, int(sp), int(orientations[i]), int(dp), 0)
        self.out_format = fmt if fmt is not None else OUT_RGB_PLANAR
        self._create("create", normalize, items, n, self.out_format)


WARP_REPLICATE = 1   # hjd_warp_item.flags bit 0


def _xform(xform):
    """Six Python ints of a warp's matrix; ValueError unless six int32 values."""
    m = [int(v) for v in xform]
    if len(m) != 6 or any(v != f for v, f in zip(m, xform)):
        raise ValueError("a warp's matrix is six integers (Q16)")
    if any(not -2 ** 31 <= v < 2 ** 31 for v in m):
        raise ValueError(f"a matrix entry leaves int32: {m}")
    return m


def warp_xform(src_w: int, src_h: int, out_w: int, out_h: int, angle: float = 0.0, zoom: float = 1.0,
               shear=(0.0, 0.0), center=None, hflip: bool = False):
    """The six Q16 integers (hjd_warp_item.m, the inverse map output -> source)
    of an affine augmentation.  Pure Python, float64.

    On pixel-centre coordinates (the centre of pixel k at k + 0.5) the output
    position p = (j + 0.5, i + 0.5) reads the source position

        s = ctr + zoom * A * (p - (out_w / 2, out_h / 2))

    with ctr = center, by default (src_w / 2, src_h / 2): the output's centre
    shows the source's.  zoom is source pixels per output pixel (2: the output
    covers twice its own size of the source).  A is the inverse of an image
    library's rotate-and-shear matrix: with r = -radians(angle) and
    (sx, sy) = radians(shear),

        a = cos(r - sy) / cos(sy)       b = -cos(r - sy) * tan(sx) / cos(sy) - sin(r)
        c = sin(r - sy) / cos(sy)       d = -sin(r - sy) * tan(sx) / cos(sy) + cos(r)
        A = [[d, -b], [-c, a]]          (no shear: [[cos t, -sin t], [sin t, cos t]], t = radians(angle))

    so a positive angle turns the picture counter-clockwise on the screen
    (angle = 90 on a square is orientation 8).  hflip mirrors the output:
    column j shows what column out_w - 1 - j would (A's first column negated).
    In source pixel indices (the centre of pixel k at k), X = s.x - 0.5:

        m0 = A00   m1 = A01   m2 = ctr.x - 0.5 + A00 * (0.5 - out_w / 2) + A01 * (0.5 - out_h / 2)
        m3 = A10   m4 = A11   m5 = ctr.y - 0.5 + A10 * (0.5 - out_w / 2) + A11 * (0.5 - out_h / 2)

    times zoom where A appears, each times 65536 and rounded to nearest: the
    position of output pixel (j, i) is then off by at most (j + i + 1) * 2**-17
    pixel.  ValueError if an entry leaves int32."""
    import math
    r = -math.radians(float(angle))
    sx, sy = (math.radians(float(v)) for v in shear)
    a = math.cos(r - sy) / math.cos(sy)
    b = -math.cos(r - sy) * math.tan(sx) / math.cos(sy) - math.sin(r)
    c = math.sin(r - sy) / math.cos(sy)
    d = -math.sin(r - sy) * math.tan(sx) / math.cos(sy) + math.cos(r)
    z = float(zoom)
    a00, a01, a10, a11 = z * d, z * -b, z * -c, z * a
    if hflip:
        a00, a10 = -a00, -a10
    cx, cy = (src_w / 2.0, src_h / 2.0) if center is None else (float(center[0]), float(center[1]))
    ox, oy = 0.5 - out_w / 2.0, 0.5 - out_h / 2.0
    real = (a00, a01, cx - 0.5 + a00 * ox + a01 * oy, a10, a11, cy - 0.5 + a10 * ox + a11 * oy)
    m = [int(math.floor(v * 65536.0 + 0.5)) for v in real]
    if any(not -2 ** 31 <= v < 2 ** 31 for v in m):
        raise ValueError(f"a matrix entry leaves int32 (Q16): {m}")
    return m


def warp_roi(width: int, height: int, xform, out_w: int, out_h: int):
    """hjd_warp_roi: the smallest (x, y, w, h) of a width x height frame that
    holds every tap an out_w x out_h output reads through xform, the tap range
    clamped into the frame (never empty).  Warping that crop with
    xform[2] - (x << 16) and xform[5] - (y << 16) equals warping the frame."""
    lib = _lib.load()
    m, r = (ctypes.c_int32 * 6)(*_xform(xform)), _lib.HjdRect()
    check(lib.hjd_warp_roi(int(width), int(height), m, int(out_w), int(out_h), ctypes.byref(r)), "hjd_warp_roi")
    return (r.x, r.y, r.w, r.h)


def warp_orient(xform, stored_w: int, stored_h: int, orientation: int):
    """hjd_warp_orient: xform addresses the displayed image of a stored_w x
    stored_h image under EXIF orientation 1..8; the six ints returned address
    the stored image.  Exact; HjdError if an entry leaves int32."""
    lib = _lib.load()
    m, out = (ctypes.c_int32 * 6)(*_xform(xform)), (ctypes.c_int32 * 6)()
    check(lib.hjd_warp_orient(m, int(stored_w), int(stored_h), int(orientation), out), "hjd_warp_orient")
    return list(out)


class Warp(_Stage):
    """hjd_warp: N planar uint8 RGB images of different sizes, each sampled
    through its own affine map (six Q16 integers, warp_xform() makes them)
    into one (N, 3, Ho, Wo) batch in one launch (include/hjd.h: bilinear,
    11-bit integer weights, one rounding, no antialiasing).  Taps outside an
    image are its fill colour, or with replicate its nearest pixel."""
    _prefix = "hjd_warp"

    def __init__(self, ctx: Context, srcs, out, xforms, fills=None, replicate=False, normalize=None):
        """srcs and out as Resize takes them.  xforms: N sequences of six
        ints.  fills: N colours 0xRRGGBB (default 0); replicate: one truthy
        value for all images or N of them (WARP_REPLICATE).  normalize =
        (a, b): the float dtypes' constants."""
        super().__init__(ctx)
        n = len(srcs)
        self.out_format, wo, ho, pitch = _batch_out(out, n)
        if len(xforms) != n:
            raise ValueError("one matrix per source")
        if fills is not None and len(fills) != n:
            raise ValueError("one fill colour per source")
        flags = _warp_flags(replicate, n)
        items = (_lib.HjdWarpItem * max(1, n))()
        for i, s in enumerate(srcs):
            t, sp = _source(s, i)
            self._keep.append(t)
            items[i] = _lib.HjdWarpItem(t.data_ptr(), out[i].data_ptr(), int(t.shape[2]), int(t.shape[1]), int(sp),
                                        flags[i], (ctypes.c_int32 * 6)(*_xform(xforms[i])),
                                        int(fills[i]) if fills is not None else 0, 0)
        self.out = out
        self._create("create", normalize, items, n, wo, ho, pitch, self.out_format)

    def launch_form(self, tiled: bool, stream=None):
        """Timing only (hjd_debug_warp_launch_form): the same launch with the
        output dealt to the waves row-major (False) or in 8 x 8-quad tiles (True)."""
        check(self.lib.hjd_debug_warp_launch_form(self.handle, 1 if tiled else 0, _stream_ptr(stream)),
              "hjd_debug_warp_launch_form")


def _warp_flags(replicate, n):
    """Per-image hjd_warp_item.flags of a `replicate` argument: one value for all, or n of them."""
    if isinstance(replicate, (list, tuple)):
        if len(replicate) != n:
            raise ValueError("one replicate flag per image")
        return [WARP_REPLICATE if r else 0 for r in replicate]
    return [WARP_REPLICATE if replicate else 0] * n


COLOR_IDENTITY = (4096, 0, 0, 0, 4096, 0, 0, 0, 4096) + (0,) * 12   # a colour record that copies: m = I, p = t = 0
COLOR_MAX_COEF, COLOR_MAX_OFFSET = 32767, 1 << 23             # include/hjd.h HJD_COLOR_MAX_*
_LUMA = (0.299, 0.587, 0.114)
# RGB -> YIQ (NTSC; rows Y, I, Q: I and Q sum to 0, so greys have I = Q = 0); _color_ops inverts it
_RGB_TO_YIQ = ((0.299, 0.587, 0.114), (0.595716, -0.274453, -0.321263), (0.211456, -0.522591, 0.311135))
_COLOR_OPS = ("brightness", "contrast", "saturation", "hue")


def _mat3(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _inv3(a):
    c = [[a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3]
          for j in range(3)] for i in range(3)]   # cofactors
    det = sum(a[0][j] * c[0][j] for j in range(3))
    return [[c[j][i] / det for j in range(3)] for i in range(3)]


def _add3(a, b):
    return [[a[i][j] + b[i][j] for j in range(3)] for i in range(3)]


def _color(record):
    """21 Python ints of a colour record; ValueError unless 21 int32 values (their ranges are the library's to refuse)."""
    c = [int(v) for v in record]
    if len(c) != 21 or any(v != f for v, f in zip(c, record)):
        raise ValueError("a colour record is 21 integers: m[9], p[9], t[3] (Q12)")
    if any(not -2 ** 31 <= v < 2 ** 31 for v in c):
        raise ValueError(f"an entry of a colour record leaves int32: {c}")
    return c


def _color_ops(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, gray=False, invert=False,
              order=_COLOR_OPS, pivot="mean"):
    """The real-valued map color_matrix() rounds: (M, P, t), 3 x 3 lists and a
    3-list of float64 with x -> M x + P xbar + t on grey levels 0..255, xbar the
    channel means of the image.  Pure Python."""
    import math
    order = tuple(order)
    if sorted(order) != sorted(_COLOR_OPS):
        raise ValueError(f"order must be a permutation of {_COLOR_OPS}")
    if not (isinstance(pivot, (int, float)) or pivot == "mean"):
        raise ValueError('pivot is "mean" or a grey level')
    if not -0.5 <= float(hue) <= 0.5:
        raise ValueError("hue is in turns, -0.5..0.5")
    for name, v in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
        if not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"{name} must be a finite factor >= 0")
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    zero = [[0.0] * 3 for _ in range(3)]
    lum = [list(_LUMA) for _ in range(3)]           # x -> L(x) * 1

    def scaled(a, f):
        return [[f * v for v in row] for row in a]

    def step(name):
        if name == "brightness":
            return scaled(eye, float(brightness)), zero, [0.0] * 3
        if name == "contrast":
            f = float(contrast)
            if pivot == "mean":
                return scaled(eye, f), scaled(lum, 1.0 - f), [0.0] * 3
            return scaled(eye, f), zero, [(1.0 - f) * float(pivot)] * 3
        if name == "saturation":
            f = float(saturation)
            return _add3(scaled(eye, f), scaled(lum, 1.0 - f)), zero, [0.0] * 3
        if name == "hue":
            a = 2.0 * math.pi * float(hue)
            rot = [[1.0, 0.0, 0.0], [0.0, math.cos(a), -math.sin(a)], [0.0, math.sin(a), math.cos(a)]]
            return _mat3(_inv3(_RGB_TO_YIQ), _mat3(rot, _RGB_TO_YIQ)), zero, [0.0] * 3
        if name == "gray":
            return lum, zero, [0.0] * 3
        return scaled(eye, -1.0), zero, [255.0] * 3   # invert

    steps = [n for n in order if {"brightness": brightness != 1.0, "contrast": contrast != 1.0,
                                  "saturation": saturation != 1.0, "hue": hue != 0.0}[n]]
    steps += (["gray"] if gray else []) + (["invert"] if invert else [])
    M, P, t = eye, zero, [0.0] * 3
    for name in steps:   # (M2, P2, t2) o (M, P, t) = (M2 M, M2 P + P2 (M + P), (M2 + P2) t + t2)
        M2, P2, t2 = step(name)
        MP2 = _add3(M2, P2)
        M, P, t = (_mat3(M2, M), _add3(_mat3(M2, P), _mat3(P2, _add3(M, P))),
                   [sum(MP2[i][k] * t[k] for k in range(3)) + t2[i] for i in range(3)])
    return M, P, t


def color_matrix(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, gray=False, invert=False,
                 order=_COLOR_OPS, pivot="mean"):
    """The 21 integers (hjd_color_item's m[9], p[9], t[3], Q12) of a colour
    augmentation: x -> M x + P xbar + t on RGB grey levels 0..255, xbar the
    channel means of the image the stage reads.  Pure Python, float64.

    The operations, applied in `order`, then gray, then invert, each skipped
    at its default, with L(x) = 0.299 R + 0.587 G + 0.114 B:

        brightness f   x -> f x
        contrast f     x -> f x + (1 - f) L(xbar) 1     (pivot = <number>: that grey level for L(xbar))
        saturation f   x -> f x + (1 - f) L(x) 1
        hue h          the rotation by 2 pi h (h in turns, -0.5..0.5) about the grey axis in YIQ
        gray           x -> L(x) 1
        invert         x -> 255 - x

    They are composed as real-valued maps with NO clamp in between: the means
    after a step are (M + P) xbar + t, so

        (M2, P2, t2) o (M1, P1, t1) = (M2 M1, M2 P1 + P2 (M1 + P1), (M2 + P2) t1 + t2)

    and only the final result is clamped to 0..255 (include/hjd.h).
    torchvision's ColorJitter clamps after each operation, so the two agree
    only while no intermediate saturates.  The hue map is DALI's and
    tf.image's rotation in YIQ; it is NOT torchvision's, which shifts H in HSV.
    Each entry is rounded to nearest in Q12 (4096 is 1.0; t in Q12 grey
    levels); ValueError if a coefficient leaves +-32767 (about +-8.0) or an
    offset +-2^23 (2048 grey levels), and for arguments outside their ranges."""
    import math
    M, P, t = _color_ops(brightness, contrast, saturation, hue, gray, invert, order, pivot)
    flat = [v for row in M for v in row] + [v for row in P for v in row] + list(t)
    c = [int(math.floor(v * 4096.0 + 0.5)) for v in flat]
    if any(abs(v) > COLOR_MAX_COEF for v in c[:18]):
        raise ValueError(f"a coefficient of m or p is outside +-{COLOR_MAX_COEF} (Q12): {c[:18]}")
    if any(abs(v) > COLOR_MAX_OFFSET for v in c[18:]):
        raise ValueError(f"an offset t is outside +-2^23 (Q12 grey levels): {c[18:]}")
    return c


class Color(_Stage):
    """hjd_color: N planar uint8 RGB images of different sizes, each through
    its own colour record (21 Q12 integers, color_matrix() makes them) into
    its own output of the same size, in one launch -- two where a record reads
    its image's channel means (include/hjd.h: exact integers, one rounding)."""
    _prefix = "hjd_color"

    def __init__(self, ctx: Context, srcs, outs, colors, normalize=None):
        """srcs as Resize takes them.  outs: N device tensors of one dtype
        (uint8, float16 or float32), out i shaped (3, h, w) as source i,
        contiguous or a [..., :w] view of wider rows, or (tensor, pitch)
        pairs -- or one (N, 3, h, w) tensor where the sizes agree.  A uint8
        out that is its source (same tensor, same pitch) runs in place.
        colors: N records of 21 ints.  normalize = (a, b): the float dtypes'
        constants."""
        super().__init__(ctx)
        n = len(srcs)
        if not isinstance(outs, (list, tuple)):
            if not (outs.ndim == 4 and outs.shape[0] == n):
                raise ValueError(f"outs must be {n} tensors or one (N, 3, h, w) tensor of {n} images")
            outs = [outs[i] for i in range(n)]
        if len(outs) != n or len(colors) != n:
            raise ValueError("one output and one colour record per source")
        items = (_lib.HjdColorItem * max(1, n))()
        fmt = None
        for i, (s, d) in enumerate(zip(srcs, outs)):
            t, sp = _planes(s, i, "source", uint8=True)
            u, dp = _planes(d, i, "output")
            if str(u.dtype) not in _DTYPE_FORMATS or (fmt is not None and _DTYPE_FORMATS[str(u.dtype)] != fmt):
                raise ValueError("outputs must be uint8 / float16 / float32 device tensors of one dtype")
            fmt = _DTYPE_FORMATS[str(u.dtype)]
            if tuple(u.shape) != tuple(t.shape):
                raise ValueError(f"output {i} is {tuple(u.shape)}, its source {tuple(t.shape)}")
            c = _color(colors[i])
            self._keep += [t, u]
            items[i] = _lib.HjdColorItem(t.data_ptr(), u.data_ptr(), int(t.shape[2]), int(t.shape[1]), int(sp), int(dp),
                                         (ctypes.c_int32 * 9)(*c[:9]), (ctypes.c_int32 * 9)(*c[9:18]),
                                         (ctypes.c_int32 * 3)(*c[18:]), 0)
        self.out_format = fmt if fmt is not None else OUT_RGB_PLANAR
        self._create("create", normalize, items, n, self.out_format)


TONE_TABLE, TONE_AUTOCONTRAST, TONE_EQUALIZE = 0, 1, 2   # include/hjd.h HJD_TONE_*: the data curve in front of the table
TONE_IDENTITY = np.tile(np.arange(256, dtype=np.uint8), (3, 1))   # a table that copies: lut[c][v] = v
TONE_IDENTITY.setflags(write=False)
_TONE_OPS = ("gamma", "posterize", "solarize")
# struct hjd_tone_curve and struct hjd_tone_item (include/hjd.h) as numpy records
_TONE_CURVE_FIELDS = [("mode", "<i4"), ("reserved", "<i4"), ("lut", "u1", (3, 256))]
_TONE_CURVE_DTYPE = np.dtype(_TONE_CURVE_FIELDS)
_TONE_ITEM_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("w", "<i4"), ("h", "<i4"), ("src_pitch", "<i4"),
                             ("dst_pitch", "<i4")] + _TONE_CURVE_FIELDS)
assert _TONE_CURVE_DTYPE.itemsize == 776 and _TONE_ITEM_DTYPE.itemsize == 808


def _tone_table(table, what="a tone table"):
    """`table` as a uint8 (3, 256) array: 256 values for all channels, or 3 x 256; ValueError unless bytes."""
    t = np.asarray(table)
    if t.shape not in ((256,), (3, 256)) or t.dtype.kind not in "iu":
        raise ValueError(f"{what} is 256 or 3 x 256 integers in 0..255")
    if t.size and (int(t.min()) < 0 or int(t.max()) > 255):
        raise ValueError(f"{what} has an entry outside 0..255")
    return np.ascontiguousarray(np.broadcast_to(t.astype(np.uint8), (3, 256)))


def tone_curve(solarize=None, posterize=None, gamma=None, invert=False, table=None, order=_TONE_OPS):
    """The uint8 (3, 256) table (hjd_tone_curve's lut) of a pointwise tone
    augmentation, the same in the three channels unless `table` differs.  numpy.

    The operations, applied in `order`, then invert, then table, each skipped
    at its default, on a grey level v in 0..255:

        gamma g       v -> floor(255 (v / 255)^g + 0.5)      (g finite and > 0, float64)
        posterize b   v -> v with its top b bits kept          (b in 1..8; Pillow's ImageOps.posterize)
        solarize t    v -> v if v < t else 255 - v             (t in 0..256; Pillow's ImageOps.solarize)
        invert        v -> 255 - v
        table         v -> table[v] or table[c][v]             (256 or 3 x 256 bytes)

    Every step maps bytes to bytes, so the composition is exact: the result
    is step_k[... step_1[v]].  With no argument it is TONE_IDENTITY.  A data
    curve (modes=TONE_AUTOCONTRAST / TONE_EQUALIZE) runs in front of the whole
    table, never between its steps."""
    import math
    order = tuple(order)
    if sorted(order) != sorted(_TONE_OPS):
        raise ValueError(f"order must be a permutation of {_TONE_OPS}")
    v = np.arange(256, dtype=np.int64)
    steps = {}
    if gamma is not None:
        g = float(gamma)
        if not (math.isfinite(g) and g > 0.0):
            raise ValueError("gamma must be a finite exponent > 0")
        steps["gamma"] = np.floor(255.0 * (v / 255.0) ** g + 0.5).astype(np.int64)
    if posterize is not None:
        if int(posterize) != posterize or not 1 <= int(posterize) <= 8:
            raise ValueError("posterize keeps 1..8 bits")
        steps["posterize"] = v & ~((1 << (8 - int(posterize))) - 1)
    if solarize is not None:
        if int(solarize) != solarize or not 0 <= int(solarize) <= 256:
            raise ValueError("solarize takes a threshold in 0..256")
        steps["solarize"] = np.where(v < int(solarize), v, 255 - v)
    lut = v
    for name in order:
        if name in steps:
            lut = steps[name][lut]
    if invert:
        lut = 255 - lut
    out = np.ascontiguousarray(np.broadcast_to(lut.astype(np.uint8), (3, 256)))
    if table is not None:
        out = np.take_along_axis(_tone_table(table, "table"), out.astype(np.int64), axis=1)
    return out


def _tone_curves(curves, modes, n, dtype=_TONE_CURVE_DTYPE):
    """n records of `dtype` (hjd_tone_curve, or hjd_tone_item with its other fields 0) from `curves`
    -- None (all TONE_IDENTITY), one table for all images or n tables -- and `modes` -- None (all
    TONE_TABLE), one mode or n.  ValueError for wrong counts; the range of a mode is the library's to refuse."""
    recs = np.zeros(max(1, n), dtype=dtype)
    if curves is None:
        recs["lut"][:] = TONE_IDENTITY
    elif isinstance(curves, np.ndarray) and curves.shape in ((256,), (3, 256)):
        recs["lut"][:] = _tone_table(curves)
    else:
        if len(curves) != n:
            raise ValueError("one tone table (tone_curve()) per image, or one for all")
        for i, c in enumerate(curves):
            recs["lut"][i] = _tone_table(c, f"tone table {i}")
    if modes is None:
        modes = [TONE_TABLE] * n
    elif isinstance(modes, (int, np.integer)):
        modes = [int(modes)] * n
    if len(modes) != n or any(int(m) != m or not -2 ** 31 <= int(m) < 2 ** 31 for m in modes):
        raise ValueError("one mode (TONE_TABLE, TONE_AUTOCONTRAST, TONE_EQUALIZE) per image, or one for all")
    recs["mode"][:n] = [int(m) for m in modes]
    return recs


class Tone(_Stage):
    """hjd_tone: N planar uint8 RGB images of different sizes, each through its
    own tone curve -- a 3 x 256 table (tone_curve() makes them), optionally
    behind autocontrast or equalize of the image's own histogram -- into its
    own output of the same size; one launch, three where a mode is not
    TONE_TABLE (include/hjd.h: exact integers, u8 = lut[c][D_c[x]])."""
    _prefix = "hjd_tone"

    def __init__(self, ctx: Context, srcs, outs, curves=None, modes=None, normalize=None):
        """srcs and outs as Color takes them (a uint8 out that is its source,
        same tensor and pitch, runs in place).  curves: N uint8 (3, 256) or
        (256,) tables, one for all, or None (TONE_IDENTITY).  modes: N of
        TONE_TABLE / TONE_AUTOCONTRAST / TONE_EQUALIZE, one for all, or None
        (TONE_TABLE).  normalize = (a, b): the float dtypes' constants."""
        super().__init__(ctx)
        n = len(srcs)
        if not isinstance(outs, (list, tuple)):
            if not (outs.ndim == 4 and outs.shape[0] == n):
                raise ValueError(f"outs must be {n} tensors or one (N, 3, h, w) tensor of {n} images")
            outs = [outs[i] for i in range(n)]
        if len(outs) != n:
            raise ValueError("one output per source")
        items = _tone_curves(curves, modes, n, _TONE_ITEM_DTYPE)
        fmt = None
        for i, (s, d) in enumerate(zip(srcs, outs)):
            t, sp = _planes(s, i, "source", uint8=True)
            u, dp = _planes(d, i, "output")
            if str(u.dtype) not in _DTYPE_FORMATS or (fmt is not None and _DTYPE_FORMATS[str(u.dtype)] != fmt):
                raise ValueError("outputs must be uint8 / float16 / float32 device tensors of one dtype")
            fmt = _DTYPE_FORMATS[str(u.dtype)]
            if tuple(u.shape) != tuple(t.shape):
                raise ValueError(f"output {i} is {tuple(u.shape)}, its source {tuple(t.shape)}")
            self._keep += [t, u]
            for name, v in (("src", t.data_ptr()), ("dst", u.data_ptr()), ("w", t.shape[2]), ("h", t.shape[1]),
                            ("src_pitch", sp), ("dst_pitch", dp)):
                items[name][i] = int(v)
        self.out_format = fmt if fmt is not None else OUT_RGB_PLANAR
        self._create("create", normalize, items.ctypes.data_as(ctypes.POINTER(_lib.HjdToneItem)), n, self.out_format)


CONV_KEEP, CONV_REFLECT, CONV_REPLICATE = 0, 1, 2   # include/hjd.h HJD_CONV_*: what a filter reads outside the image
CONV_MAX_RADIUS, CONV_MAX_GAIN = 11, 1 << 20        # include/hjd.h HJD_CONV_MAX_*
# struct hjd_conv_filter and struct hjd_conv_item (include/hjd.h) as numpy records
_CONV_FILTER_FIELDS = [("rx", "<i4"), ("ry", "<i4"), ("border", "<i4"), ("a", "<i4"), ("b", "<i4"), ("reserved", "<i4"),
                       ("kh", "<u2", (24,)), ("kv", "<u2", (24,))]
_CONV_FILTER_DTYPE = np.dtype(_CONV_FILTER_FIELDS)
_CONV_ITEM_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("w", "<i4"), ("h", "<i4"), ("src_pitch", "<i4"),
                             ("dst_pitch", "<i4")] + _CONV_FILTER_FIELDS)
assert _CONV_FILTER_DTYPE.itemsize == 120 and _CONV_ITEM_DTYPE.itemsize == 152


def conv_filter(kh, kv, a, b, border=CONV_REFLECT):
    """One hjd_conv_filter record (a 0-d numpy record of 120 bytes) from two
    odd-length rows of Q12 integer taps and two Q12 integer gains:
    u8 = clamp((a (x << 24) + b S + 2^35) >> 36), S the window under kv x kh
    (include/hjd.h).  ValueError unless the rows are 1, 3, .. 23 integers in
    0..4096; the other ranges are the library's to refuse."""
    f = np.zeros((), dtype=_CONV_FILTER_DTYPE)
    for name, radius, taps in (("kh", "rx", kh), ("kv", "ry", kv)):
        t = [int(v) for v in taps]
        if len(t) % 2 != 1 or len(t) > 2 * CONV_MAX_RADIUS + 1 or any(v != u or not 0 <= v <= 4096 for v, u in zip(t, taps)):
            raise ValueError(f"{name} is 1, 3, .. {2 * CONV_MAX_RADIUS + 1} integer taps in 0..4096 (Q12)")
        f[name][:len(t)] = t
        f[radius] = len(t) // 2
    for name, v in (("a", a), ("b", b), ("border", border)):
        if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError(f"{name} is an int32")
        f[name] = int(v)
    return f


CONV_IDENTITY = conv_filter([4096], [4096], 4096, 0, CONV_KEEP)   # a filter that copies: rx = ry = 0, a = 4096, b = 0
CONV_IDENTITY.setflags(write=False)


def conv_sharpness(factor):
    """The filter of a sharpness factor f >= 0 (Pillow's ImageEnhance.Sharpness,
    torchvision's adjust_sharpness): the real map f x + (1 - f) (box + 4 x) / 13,
    box the sum of the 3 x 3 window, with ONE rounding -- rx = ry = 1,
    CONV_KEEP, taps (1024, 1024, 1024) on both axes, a = round(4096 (4 + 9 f) /
    13), b = round(65536 (1 - f) / 13).  f = 0 smooths, 1 is CONV_IDENTITY, 2
    sharpens.  Pillow rounds the smoothed image and truncates the blend: within
    2 grey levels for f in 0..2 (include/hjd.h has what was measured)."""
    import math
    f = float(factor)
    if not (math.isfinite(f) and f >= 0.0):
        raise ValueError("factor must be a finite number >= 0")
    if f == 1.0:
        return CONV_IDENTITY.copy()
    a, b = int(math.floor(4096.0 * (4.0 + 9.0 * f) / 13.0 + 0.5)), int(math.floor(65536.0 * (1.0 - f) / 13.0 + 0.5))
    if abs(a) > CONV_MAX_GAIN or abs(b) > CONV_MAX_GAIN:
        raise ValueError(f"factor {factor}: a gain leaves +-2^20 (Q12)")
    return conv_filter([1024] * 3, [1024] * 3, a, b, CONV_KEEP)


def _gaussian_real(sigma, ksize):
    """torchvision's taps in float64: exp(-(t / sigma)^2 / 2) on linspace(-(k - 1) / 2, (k - 1) / 2, k), normalised."""
    t = np.linspace(-(ksize - 1) / 2.0, (ksize - 1) / 2.0, ksize)
    k = np.exp(-0.5 * (t / float(sigma)) ** 2)
    return k / k.sum()


def _gaussian_taps(sigma, ksize):
    """_gaussian_real in Q12 by largest remainder, so the row sums to exactly
    4096 (ties: nearer the centre, then the lower index); zero taps at both
    ends trimmed symmetrically."""
    import math
    if not (math.isfinite(float(sigma)) and float(sigma) > 0.0):
        raise ValueError("sigma must be a finite number > 0")
    if ksize is None:
        ksize = min(2 * CONV_MAX_RADIUS + 1, 2 * int(math.ceil(3.0 * float(sigma))) + 1)
    if int(ksize) != ksize or int(ksize) % 2 != 1 or not 1 <= int(ksize) <= 2 * CONV_MAX_RADIUS + 1:
        raise ValueError(f"ksize is odd, 1..{2 * CONV_MAX_RADIUS + 1}")
    ksize = int(ksize)
    scaled = _gaussian_real(sigma, ksize) * 4096.0
    q = np.floor(scaled).astype(np.int64)
    frac = scaled - q
    order = sorted(range(ksize), key=lambda i: (-frac[i], abs(i - ksize // 2), i))
    for i in order[:4096 - int(q.sum())]:
        q[i] += 1
    q = [int(v) for v in q]
    assert sum(q) == 4096
    while len(q) > 1 and q[0] == 0 and q[-1] == 0:
        q = q[1:-1]
    return q


def _ksizes(ksize):
    return tuple(ksize) if isinstance(ksize, (list, tuple)) else (ksize, ksize)


def conv_gaussian(sigma, ksize=None, sigma_y=None, border=CONV_REFLECT):
    """The filter of a Gaussian blur (torchvision's GaussianBlur): per axis the
    taps exp(-(t / sigma)^2 / 2) on linspace(-(k - 1) / 2, (k - 1) / 2, k),
    normalised, quantised to Q12 by largest remainder so each row sums to
    exactly 4096, zero taps at both ends trimmed (the radius shrinks); a = 0,
    b = 4096, so u8 = (S + 2^23) >> 24.  ksize: odd, 1..23, one number or (kx,
    ky); None: 2 ceil(3 sigma) + 1, capped at 23.  sigma_y: the vertical
    sigma (None: sigma).  This is NOT Pillow's GaussianBlur, a repeated box blur."""
    kx, ky = _ksizes(ksize)
    return conv_filter(_gaussian_taps(sigma, kx), _gaussian_taps(sigma if sigma_y is None else sigma_y, ky), 0, 4096, border)


def conv_unsharp(sigma, amount, ksize=None, border=CONV_REFLECT):
    """Unsharp masking, x + amount (x - blur(x)): conv_gaussian's taps with
    a = round(4096 (1 + amount)), b = round(-4096 amount), one rounding."""
    import math
    m = float(amount)
    if not math.isfinite(m):
        raise ValueError("amount must be finite")
    a, b = int(math.floor(4096.0 * (1.0 + m) + 0.5)), int(math.floor(-4096.0 * m + 0.5))
    if abs(a) > CONV_MAX_GAIN or abs(b) > CONV_MAX_GAIN:
        raise ValueError(f"amount {amount}: a gain leaves +-2^20 (Q12)")
    kx, ky = _ksizes(ksize)
    return conv_filter(_gaussian_taps(sigma, kx), _gaussian_taps(sigma, ky), a, b, border)


def _conv_filters(filters, n, dtype=_CONV_FILTER_DTYPE):
    """n records of `dtype` (hjd_conv_filter, or hjd_conv_item with its other fields 0) from `filters`
    -- None (all CONV_IDENTITY), one record for all images or n records (conv_filter() and its kin make
    them).  ValueError for wrong counts and for anything that is not such a record."""
    recs = np.zeros(max(1, n), dtype=dtype)

    def one(f, what):
        f = np.asarray(f)
        if f.dtype != _CONV_FILTER_DTYPE or f.shape != ():
            raise ValueError(f"{what} is not a filter record (conv_filter(), conv_sharpness(), conv_gaussian(), "
                             "conv_unsharp())")
        return f

    if filters is None or (isinstance(filters, np.ndarray) and filters.shape == ()):
        f = one(CONV_IDENTITY if filters is None else filters, "filters")
        for name, *_ in _CONV_FILTER_FIELDS:
            recs[name][:] = f[name]
    else:
        if len(filters) != n:
            raise ValueError("one filter record per image, or one for all")
        for i, f in enumerate(filters):
            f = one(f, f"filter {i}")
            for name, *_ in _CONV_FILTER_FIELDS:
                recs[name][i] = f[name]
    return recs


class Conv(_Stage):
    """hjd_conv: N planar uint8 RGB images of different sizes, each through its
    own small separable filter with a blend against the centre pixel
    (conv_sharpness(), conv_gaussian(), conv_unsharp() make the records) into
    its own output of the same size, in one launch (include/hjd.h: exact
    integers, one rounding)."""
    _prefix = "hjd_conv"

    def __init__(self, ctx: Context, srcs, outs, filters=None, normalize=None):
        """srcs and outs as Color takes them, but no out may be its source: a
        filter cannot run in place.  filters: N filter records, one for all, or
        None (CONV_IDENTITY).  normalize = (a, b): the float dtypes' constants."""
        super().__init__(ctx)
        n = len(srcs)
        if not isinstance(outs, (list, tuple)):
            if not (outs.ndim == 4 and outs.shape[0] == n):
                raise ValueError(f"outs must be {n} tensors or one (N, 3, h, w) tensor of {n} images")
            outs = [outs[i] for i in range(n)]
        if len(outs) != n:
            raise ValueError("one output per source")
        items = _conv_filters(filters, n, _CONV_ITEM_DTYPE)
        fmt = None
        for i, (s, d) in enumerate(zip(srcs, outs)):
            t, sp = _planes(s, i, "source", uint8=True)
            u, dp = _planes(d, i, "output")
            if str(u.dtype) not in _DTYPE_FORMATS or (fmt is not None and _DTYPE_FORMATS[str(u.dtype)] != fmt):
                raise ValueError("outputs must be uint8 / float16 / float32 device tensors of one dtype")
            fmt = _DTYPE_FORMATS[str(u.dtype)]
            if tuple(u.shape) != tuple(t.shape):
                raise ValueError(f"output {i} is {tuple(u.shape)}, its source {tuple(t.shape)}")
            self._keep += [t, u]
            for name, v in (("src", t.data_ptr()), ("dst", u.data_ptr()), ("w", t.shape[2]), ("h", t.shape[1]),
                            ("src_pitch", sp), ("dst_pitch", dp)):
                items[name][i] = int(v)
        self.out_format = fmt if fmt is not None else OUT_RGB_PLANAR
        self._create("create", normalize, items.ctypes.data_as(ctypes.POINTER(_lib.HjdConvItem)), n, self.out_format)


def worker_cpus(bus: str, gpus: Sequence[str], sysfs_root: Optional[str] = None, only_allowed: bool = False):
    """hjd_debug_worker_cpus: the host CPUs the worker pool of the GPU at PCI
    address `bus` binds to, among the GPUs `gpus` (its NUMA node's CPUs split
    per GPU of that node), from the sysfs tree at `sysfs_root` (None: the real one)."""
    lib = _lib.load()
    arr = (ctypes.c_char_p * max(1, len(gpus)))(*[g.encode() for g in gpus])
    cap = 4096
    out = (ctypes.c_int32 * cap)()
    n = ctypes.c_int32(0)
    check(lib.hjd_debug_worker_cpus(sysfs_root.encode() if sysfs_root else None, bus.encode(), arr, len(gpus),
                                    int(only_allowed), out, cap, ctypes.byref(n)), "hjd_debug_worker_cpus")
    return list(out[:min(n.value, cap)])


def device_worker_cpus(device: int):
    """hjd_device_worker_cpus: the host CPUs the stream workers of HIP device
    `device` bind to (its share of its NUMA node; [] = unknown topology)."""
    lib = _lib.load()
    if getattr(lib, "hjd_device_worker_cpus", None) is None:   # an older HJD_LIB tuning build
        return []
    cap = 4096
    out = (ctypes.c_int32 * cap)()
    n = ctypes.c_int32(0)
    check(lib.hjd_device_worker_cpus(int(device), out, cap, ctypes.byref(n)), "hjd_device_worker_cpus")
    return list(out[:min(n.value, cap)])


def cpu_share(root: Optional[str] = None) -> int:
    """hjd_host_cpu_share (root None) or hjd_debug_cpu_share on a fake tree:
    affinity CPUs capped by the cgroup's CPU quota."""
    lib = _lib.load()
    return lib.hjd_host_cpu_share() if root is None else lib.hjd_debug_cpu_share(root.encode())


def stream_worker_threads(share: int, world: int, slice_cpus: int) -> int:
    """Host worker threads per GPU of a multi-rank stream job (bench.py config
    5): the process's CPU share split over the ranks on the host, capped by the
    GPU's CPU slice when the topology is known (every logical CPU of the slice:
    SMT pays for the Huffman decode, profiles/r06a_smt_probe.json)."""
    per_rank = max(1, share // max(1, world))
    return min(per_rank, slice_cpus) if slice_cpus > 0 else per_rank


def autotune_cache_clear():
    """Forget every cached hjd_plan_autotune choice of this process."""
    check(_lib.load().hjd_autotune_cache_clear(), "hjd_autotune_cache_clear")


def _set_tuning(name: str, value):
    fn = getattr(_lib.load(), "hjd_debug_set_tuning", None)
    if fn is None:
        raise RuntimeError(f"{_lib.LIB_PATH} has no hjd_debug_set_tuning: it cannot switch {name} in-process")
    check(fn(name.encode(), None if value is None else str(value).encode()), "hjd_debug_set_tuning")


@contextlib.contextmanager
def debug_tuning(name: str, value):
    """Switch one HJD_* override in-process (hjd_debug_set_tuning): `value` is
    what the environment variable would hold (None: what the process started
    with).  On exit the override goes back to what the process started with,
    so blocks for one name do not nest.  The overrides are process-wide."""
    _set_tuning(name, value)
    try:
        yield
    finally:
        _set_tuning(name, None)


def decode_frame(ctx: Context, coefs, qt: np.ndarray, width: int, height: int, sampling: int,
                 input_format: int = IN_Q16_ZIGZAG, stream=None, scale: int = 1, roi=None,
                 out_format: int = OUT_BGRX, normalize=None):
    """Decode one frame already resident on the device; returns an int32 (H, W)
    device tensor holding BGRX words (0x00RRGGBB); scale 2, 4 or 8: (H', W') =
    scaled_size(width, height, scale), reversed; roi (x, y, w, h) on that
    grid: an (h, w) tensor.  out_format OUT_RGB_PLANAR_F16 / _F32: a (3, H, W)
    float16 / float32 tensor normalised with normalize = (a, b)
    (norm_constants(); None: a = 1, b = 0)."""
    import torch
    if out_format not in (OUT_BGRX, OUT_RGB_PLANAR_F16, OUT_RGB_PLANAR_F32):
        raise ValueError("decode_frame gives BGRX words or float planes")
    if normalize is not None and out_format == OUT_BGRX:
        raise ValueError("normalize needs out_format OUT_RGB_PLANAR_F16 or OUT_RGB_PLANAR_F32")
    spec = FrameSpec(width, height, sampling, qt_index=(0, 1, 2), roi=roi, out_format=out_format)
    plan = Plan(ctx, [spec], input_format, qtables=qt if input_format == IN_Q16_ZIGZAG else None, scale=scale,
                normalize=normalize)
    width, height = spec.out_size(scale)
    if out_format == OUT_BGRX:
        out = torch.empty((height, width), dtype=torch.int32, device=coefs.device)
    else:
        out = torch.empty((3, height, width), device=coefs.device,
                          dtype=torch.float16 if out_format == OUT_RGB_PLANAR_F16 else torch.float32)
    plan.launch(coefs, out, stream)
    return out, plan
