"""ocljpegdecoder_amd -- MI355X-native JPEG pixel back-end.

Drop-in replacement for the OpenCL IDCT/colour back-end of
xinfushe/oclJPEGDecoder (src/oclDCT8x8.cpp + src/idct8x8.cl behind src/idct.h).
The hot path is the fused HIP kernel in csrc/hjd_kernels.hpp, reached through
the C ABI in include/hjd.h (libhjd.so).  Importing this package loads the
native library and fails loudly if it is missing.
"""
from . import _lib

_lib.load()

from .backend import (  # noqa: E402
    IN_I32_NATURAL,
    IN_Q16_ZIGZAG,
    OTHER,
    KERNEL_AUTO,
    KERNEL_LATENCY,
    KERNEL_PERSISTENT,
    OUT_BGR24,
    OUT_BGRX,
    OUT_BYTES,
    OUT_RGB24,
    OUT_RGB_PLANAR,
    OUT_RGB_PLANAR_F16,
    OUT_RGB_PLANAR_F32,
    GRAY,
    YUV411_H4V1,
    YUV420,
    YUV422,
    YUV440,
    YUV444,
    autotune_cache_clear,
    block_components,
    Color,
    COLOR_IDENTITY,
    color_matrix,
    Tone,
    TONE_AUTOCONTRAST,
    TONE_EQUALIZE,
    TONE_IDENTITY,
    TONE_TABLE,
    tone_curve,
    Conv,
    CONV_IDENTITY,
    CONV_KEEP,
    CONV_REFLECT,
    CONV_REPLICATE,
    conv_filter,
    conv_gaussian,
    conv_sharpness,
    conv_unsharp,
    Context,
    cpu_share,
    debug_tuning,
    FrameSpec,
    Plan,
    decode_frame,
    default_pitch,
    device_count,
    device_worker_cpus,
    frame_blocks,
    frame_check,
    mcu_geometry,
    norm_constants,
    Orient,
    oriented_roi,
    oriented_size,
    Resize,
    RESIZE_FLIP_H,
    RESIZE_BILINEAR,
    RESIZE_TRIANGLE_AA,
    resize_scale,
    roi_geometry,
    scaled_size,
    stream_worker_threads,
    Warp,
    WARP_REPLICATE,
    warp_orient,
    warp_roi,
    warp_xform,
    worker_cpus,
)

from .jpeg import (GpuDecoder, GpuJpegStream, JpegInfo, JpegStream, bmp_bytes, bmp_header,  # noqa: E402
                   decode_coefs, decode_coefs_batch, decode_coefs_into, decode_jpeg, emulate_entropy,
                   exif_orientation, parse, pinned_bytes)

__all__ = [
    "GpuDecoder", "GpuJpegStream", "JpegInfo", "JpegStream", "bmp_bytes", "bmp_header", "decode_coefs",
    "decode_coefs_batch", "decode_coefs_into", "decode_jpeg", "emulate_entropy",
    "parse", "pinned_bytes",
    "Context", "FrameSpec", "Plan", "autotune_cache_clear", "decode_frame", "device_count", "frame_blocks", "mcu_geometry", "worker_cpus", "cpu_share", "debug_tuning",
    "device_worker_cpus", "stream_worker_threads", "scaled_size", "roi_geometry", "norm_constants", "frame_check",
    "OUT_RGB_PLANAR_F16", "OUT_RGB_PLANAR_F32", "Resize", "RESIZE_FLIP_H", "RESIZE_BILINEAR", "RESIZE_TRIANGLE_AA", "resize_scale",
    "Orient", "oriented_roi", "oriented_size", "exif_orientation",
    "Warp", "WARP_REPLICATE", "warp_roi", "warp_orient", "warp_xform",
    "Color", "COLOR_IDENTITY", "color_matrix",
    "Tone", "TONE_TABLE", "TONE_AUTOCONTRAST", "TONE_EQUALIZE", "TONE_IDENTITY", "tone_curve",
    "Conv", "CONV_KEEP", "CONV_REFLECT", "CONV_REPLICATE", "CONV_IDENTITY", "conv_filter", "conv_sharpness", "conv_gaussian",
    "conv_unsharp",
    "YUV444", "YUV420", "YUV422", "GRAY", "YUV411_H4V1", "YUV440", "OTHER", "block_components", "KERNEL_AUTO", "KERNEL_PERSISTENT", "KERNEL_LATENCY", "OUT_BGRX", "OUT_BGR24", "OUT_RGB24", "OUT_RGB_PLANAR", "OUT_BYTES", "default_pitch", "IN_Q16_ZIGZAG", "IN_I32_NATURAL",
]
