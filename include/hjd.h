/*
 * hjd.h -- C ABI of the MI355X (gfx950) JPEG pixel back-end.
 *
 * Hot path (one fused HIP kernel): zigzag + dequant -> 8x8 integer IDCT ->
 * chroma upsample (nearest, 2x2) -> YCbCr->RGB (JFIF, truncating) -> BGRX store,
 * bit-exact to the reference CPU path (src/cpuIDCT8x8.cpp + src/decoder.cpp:367-491
 * of xinfushe/oclJPEGDecoder).  Plain C types only; every device pointer is a
 * HIP device address, every `stream` a hipStream_t (NULL = default stream).
 *
 * The reference's own entry points (src/idct.h:4-18) are provided with their
 * original C++ signatures by include/idct.h on top of this ABI.
 *
 * Errors: functions return HJD_OK (0) or a negative HJD_E_* code and never
 * throw; hjd_last_error() returns a description of the last failure on the
 * calling thread.
 */
#ifndef HJD_H
#define HJD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HJD_ABI_VERSION 1

enum hjd_status {
    HJD_OK = 0,
    HJD_E_INVALID = -1,   /* bad argument / unsupported geometry */
    HJD_E_NO_DEVICE = -2, /* no HIP device (or index out of range) */
    HJD_E_HIP = -3,       /* a HIP runtime call failed */
    HJD_E_NOMEM = -4,     /* host or device allocation failed */
    HJD_E_STATE = -5      /* call out of sequence (e.g. run before upload) */
};

/* Chroma sampling.  0..2 are numerically equal to the reference's ColorSpace
 * enum (src/macro.h:114-119: YUV444 = 0, YUV411 = 1 (really H2V2 4:2:0),
 * Other = 2).  HJD_YUV422 (Y H2V1, chroma H1V1) and HJD_GRAY (one component)
 * are extensions the reference rejects (src/decoder.cpp:58-69; SURVEY.md
 * s8(f) rank 4): the same IDCT and the same colour arithmetic with nearest
 * (horizontal) chroma replication, and R = G = B = clamp(Y + 128) for gray
 * (the reference's formula with U = V = 0).  HJD_YUV411_H4V1 (true 4:1:1:
 * Y H4V1, chroma H1V1; not the reference's "YUV411", which is H2V2) and
 * HJD_YUV440 (Y H1V2) are further extensions with nearest replication along
 * the subsampled axis. */
enum hjd_sampling {
    HJD_YUV444 = 0, HJD_YUV420 = 1, HJD_OTHER = 2, HJD_YUV422 = 3, HJD_GRAY = 4, HJD_YUV411_H4V1 = 5, HJD_YUV440 = 6
};

/* Output pixel format. */
enum hjd_out_format {
    /* 4 bytes per pixel: B, G, R, 0 (the reference's RGB32 buffer and its
     * 32-bpp BMP rows, src/decoder.cpp:367-395). */
    HJD_OUT_BGRX = 0,
    /* 3 bytes per pixel: B, G, R (a 24-bpp BMP row; extension, SURVEY.md
     * s8(f) rank 4).  Same values as BGRX without the pad byte; the kernel
     * writes 25 % fewer bytes. */
    HJD_OUT_BGR24 = 1,
    /* 3 bytes per pixel: R, G, B, interleaved (HWC: what PIL / numpy callers
     * hold).  Same values as BGR24 with R and B exchanged. */
    HJD_OUT_RGB24 = 2,
    /* Three uint8 planes R, G, B, each `height` rows of `out_pitch` bytes
     * (CHW: what tensor pipelines hold).  Plane c of a frame starts at
     * out_offset + c * out_pitch * height; with out_pitch == width a frame is
     * a contiguous (3, H, W) array, and equal frames at consecutive offsets
     * form (N, 3, H, W).  HJD_GRAY frames write three identical planes.
     *
     * HJD_OUT_RGB24 and HJD_OUT_RGB_PLANAR take ANY out_pitch >= 3*width
     * (planar: >= width) up to HJD_MAX_OUT_PITCH (2^28, the bound of every
     * format: a larger pitch is HJD_E_INVALID, see hjd_frame.out_pitch), any
     * out_offset and any per-image output pointer, so
     * a contiguous array of any width can be the destination.  A frame whose
     * out_pitch, out_offset (and output pointer) are all multiples of 4 is
     * written with full-width vector stores; any other frame takes the
     * guarded byte-store path for every strip: correct, but slower.  (The
     * buffer passed to hjd_plan_launch stays 16-byte aligned for every
     * format; frames sit in it at any out_offset.) */
    HJD_OUT_RGB_PLANAR = 3,
    /* Normalised float planes (extension): three planes R, G, B of IEEE half
     * (F16, 2 bytes) or float (F32, 4 bytes) elements, laid out as
     * HJD_OUT_RGB_PLANAR's with out_pitch the BYTES of one plane's row (>= 2*w
     * or 4*w; plane c at out_offset + c * out_pitch * h, 64-bit).  Let u8 be
     * the byte HJD_OUT_RGB_PLANAR writes for that channel and pixel (under the
     * same scale and ROI) and a[c], b[c] the plan's six fp32 constants
     * (hjd_plan_set_normalize; default a = 1, b = 0):
     *     F32: out = fma((float)u8, a[c], b[c])   -- ONE correctly rounded fp32
     *          operation, round-to-nearest-even; not a multiply, then an add;
     *     F16: that fp32 value converted to half, round-to-nearest-even;
     *          overflow gives +-inf, half subnormals are kept.  Both roundings
     *          are part of the definition.
     * (An fp32-subnormal result follows the kernels' default mode, which keeps
     * fp32 subnormals.)  The integer pipeline is untouched: the converted
     * bytes are the bit-exact ones of the byte formats.
     *
     * out_offset and out_pitch must be multiples of the element size
     * (HJD_E_INVALID otherwise).  Frames whose out_offset and out_pitch (and
     * output pointer) are multiples of 8 (F16) or 16 (F32) take full-width
     * vector stores on interior strips (with a ROI: and dx % 4 == 0, as the
     * other formats); any other frame takes the guarded element stores.
     *
     * HJD_IN_Q16_ZIGZAG input only; every sampling at scale 1 (persistent and
     * latency kernel), 4:4:4 / 4:2:0 / gray scaled, ROIs as the other formats.
     * Refused with HJD_E_INVALID: HJD_IN_I32_NATURAL, kernel variants, the
     * stream pipelines (hjd_stream / hjd_gstream set_output_format) and the
     * idct.h shim.  There is no interleaved (H, W, 3) float layout. */
    HJD_OUT_RGB_PLANAR_F16 = 5,   /* 4 is not a format: it stays HJD_E_INVALID, as before these two */
    HJD_OUT_RGB_PLANAR_F32 = 6
};

/* Kernel selection of a plan (hjd_plan_set_kernel).  Both kernels produce
 * identical pixels; AUTO takes the latency kernel (one workgroup per 48-block
 * task, six waves sharing it) for launches of few tasks -- a single frame --
 * and the persistent streaming kernel for batches. */
enum hjd_kernel_mode { HJD_KERNEL_AUTO = 0, HJD_KERNEL_PERSISTENT = 1, HJD_KERNEL_LATENCY = 2 };

/* Coefficient input format. */
enum hjd_input_format {
    /* int16 quantised coefficients in zigzag order, exactly as Huffman decoding
     * produces them (src/decoder.cpp:221-260); dequant + de-zigzag happen in
     * the kernel load (src/decoder.cpp:338-342). 128 B per block. */
    HJD_IN_Q16_ZIGZAG = 0,
    /* int32 dequantised coefficients in natural order: the reference's
     * jpg.mcu_data layout (src/jpeg.h:76) accepted by
     * clidct_transfer_data_to_device. 256 B per block. */
    HJD_IN_I32_NATURAL = 1
};

/* The largest out_pitch of a frame, in bytes, for every sampling, scale and
 * output format (also of hjd_gdec_decode's per-image pitches): the fused pixel
 * kernel adds up to 15 rows of out_pitch and one strip row in a 32-bit lane
 * offset, and 2^28 is the largest power of two for which that fits.  A larger
 * pitch is refused with HJD_E_INVALID ("frame N: out_pitch P is above
 * HJD_MAX_OUT_PITCH (268435456)").  Pinned on the device at the bound for
 * every sampling and format (tests/test_gpu_pitch_limits.py). */
#define HJD_MAX_OUT_PITCH (1 << 28)

/*
 * One frame of a batch.  Blocks are MCU-major in raster MCU order; per MCU the
 * Y blocks in HxV raster order, then Cb, then Cr (src/decoder.cpp:286-344).
 * MCU grid: ceil(W/8)xceil(H/8) (4:4:4, 3 blocks; gray, 1 block),
 * ceil(W/16)xceil(H/16) (4:2:0, 6 blocks), ceil(W/16)xceil(H/8) (4:2:2,
 * 4 blocks), ceil(W/32)xceil(H/8) (4:1:1, 6 blocks) or ceil(W/8)xceil(H/16)
 * (4:4:0, 4 blocks).
 */
typedef struct hjd_frame {
    uint64_t coef_offset; /* first block's offset in the coef buffer, in BLOCKS */
    uint64_t out_offset;  /* byte offset of pixel (0,0) in the output buffer */
    int32_t width;        /* visible pixels (output is cropped to W x H) */
    int32_t height;
    int32_t out_pitch;    /* bytes per output row, >= 4*width (BGR24: 3*width), multiple of 4;
                           * RGB24: >= 3*width, planar RGB: >= width, any value; float planar: >= 2*width
                           * (F16) or 4*width (F32), multiple of the element size (see hjd_out_format);
                           * every format: <= HJD_MAX_OUT_PITCH */
    int32_t sampling;     /* enum hjd_sampling (not HJD_OTHER) */
    int32_t qt_index[3];  /* per component (Y, Cb, Cr): index into the qtable set */
    int32_t out_format;   /* enum hjd_out_format (HJD_OUT_BGRX = 0); the same for all frames of a plan */
} hjd_frame;

typedef struct hjd_ctx hjd_ctx;
typedef struct hjd_plan hjd_plan;

/* ---- library / device ---- */
int hjd_abi_version(void);
const char* hjd_last_error(void);
int hjd_device_count(int* count);

/* Context = one device + one stream of work.  Not thread-safe; use one context
 * per host thread (or per GPU). */
int hjd_ctx_create(int device, hjd_ctx** out);
int hjd_ctx_destroy(hjd_ctx* ctx);
int hjd_ctx_device(const hjd_ctx* ctx);

/* ---- sizes ---- */
int hjd_frame_blocks(int width, int height, int sampling, int64_t* nblocks);
/* Output size of a width x height source decoded at `scale` (1, 2, 4 or 8):
 * ceil(width/scale) x ceil(height/scale).  Host only: needs no device. */
int hjd_scaled_size(int width, int height, int scale, int* out_w, int* out_h);

/*
 * Plan: validates a batch of frames, computes the work decomposition and
 * uploads the frame table and de-zigzagged quantisation tables to the device
 * (synchronously, outside any timed region).  qtables: nq tables of 64 values
 * each in FILE (zigzag) order, as DQT stores them (src/parser.cpp:65-89);
 * ignored (may be NULL) for HJD_IN_I32_NATURAL.
 */
int hjd_plan_create(hjd_ctx* ctx, const hjd_frame* frames, int nframes, int input_format,
                    const int32_t* qtables, int nq, hjd_plan** out);
/*
 * Scaled decode: the plan's frames come out at 1/scale of their size, scale =
 * 1, 2, 4 or 8 (scale 1 is exactly hjd_plan_create).  Definition (exact,
 * integer): every 8x8 block's IDCT samples -- the full 8-point IDCT, after its
 * [-256,255] clamp -- are reduced to (8/scale)^2 box means,
 *     m = (sum of the scale x scale box + scale*scale/2) >> (2 * log2 scale)
 * (arithmetic shift: floor); boxes never cross a block.  The scaled blocks
 * form the component planes in the same MCU order as the full-size ones,
 * chroma is replicated nearest by the sampling's own factors on the scaled
 * grids (4:2:0 at scale 8: an MCU is 2x2 luma samples over one chroma sample),
 * and the colour conversion is the full-size one applied to the means.  This
 * is a box filter of the bit-exact full-size samples, not a reduced-size IDCT.
 *
 * Frames carry the SOURCE width and height.  The output is
 * ceil(width/scale) x ceil(height/scale) pixels (hjd_scaled_size), cropped as
 * at full size: the boxes on the right and bottom edges include the encoder's
 * padding samples past the visible edge, as libjpeg's scaled decode does.
 * out_pitch, its minimum and alignment rules and the planar plane stride
 * (out_pitch * scaled height) all refer to the scaled size.
 *
 * scale > 1 serves HJD_YUV444, HJD_YUV420 and HJD_GRAY with HJD_IN_Q16_ZIGZAG
 * input, all four output formats, through the persistent kernel only (however
 * few tasks the plan has): 4:2:2, 4:1:1, 4:4:0, HJD_IN_I32_NATURAL, a non-zero
 * hjd_plan_set_variant, hjd_plan_set_kernel(HJD_KERNEL_LATENCY) and
 * hjd_debug_plan_launch_stages return HJD_E_INVALID.  hjd_plan_set_chunk and
 * hjd_plan_autotune (chunks only; the cache key includes the scale) work.
 */
int hjd_plan_create_scaled(hjd_ctx* ctx, const hjd_frame* frames, int nframes, int input_format,
                           const int32_t* qtables, int nq, int scale, hjd_plan** out);
int hjd_plan_scale(const hjd_plan* plan);          /* 1, 2, 4 or 8 */

/*
 * Region-of-interest decode.  A ROI is a rectangle (x, y, w, h) on the
 * frame's output grid W' x H': the frame's own W x H in a scale-1 plan,
 * hjd_scaled_size(W, H, scale) in a scaled one.  It must satisfy x, y >= 0,
 * w, h >= 1, x + w <= W', y + h <= H'; anything else is HJD_E_INVALID.  The
 * output of a ROI frame is exactly full[y:y+h, x:x+w], where `full` is what
 * the same plan without the ROI writes: bit-exact in every output format, no
 * new arithmetic.  Pixel (x, y) of the frame lands at out_offset; out_pitch,
 * its minimum (row bytes x w) and its alignment rules refer to the ROI width;
 * the planar plane stride is out_pitch * h; no byte outside the w x h payload
 * is written.
 *
 * Only the strips (tasks of 48 blocks of one MCU row) that touch the
 * rectangle are decoded, and the strips are anchored at the ROI's first MCU
 * column: hjd_roi_geometry gives the count.  Coefficients of other strips are
 * never read.
 *
 * Vector stores: let dx be x minus the first pixel column of the MCU that
 * holds x (on the output grid).  Strips wholly inside the ROI keep the
 * full-width vector stores when dx % 4 == 0 (at scale 1, and wherever the
 * scaled MCU is >= 4 px wide, that is x % 4 == 0) and out_pitch and
 * out_offset meet the format's present alignment (16 bytes BGRX, 4 bytes the
 * 3-byte and planar formats).  Any other x is legal and takes the guarded
 * stores for every strip, as an unaligned pitch does today.
 *
 * A ROI plan takes HJD_IN_Q16_ZIGZAG input, all four output formats, every
 * sampling at scale 1 and 4:4:4 / 4:2:0 / gray at scale 2, 4, 8, through the
 * persistent kernel only (HJD_KERNEL_AUTO takes it however few tasks there
 * are).  HJD_IN_I32_NATURAL, a non-zero hjd_plan_set_variant,
 * hjd_plan_set_kernel(HJD_KERNEL_LATENCY) and hjd_debug_plan_launch_stages
 * return HJD_E_INVALID.  hjd_plan_set_chunk and hjd_plan_autotune work (the
 * cache key includes the ROI flag).
 */
typedef struct hjd_rect { int32_t x, y, w, h; } hjd_rect;
/* Validates `roi` against a width x height source of `sampling` at `scale`
 * and returns the ROI's task count and the coefficient blocks those tasks
 * read (strips are clipped at the MCU-row end).  Host only: needs no device. */
int hjd_roi_geometry(int width, int height, int sampling, int scale, const hjd_rect* roi, int64_t* tasks,
                     int64_t* blocks);
/* rois == NULL: exactly hjd_plan_create_scaled.  Otherwise one rectangle per
 * frame; frames carry the source size.  hjd_plan_pixels is then the sum of
 * w * h, hjd_plan_tasks the ROI task count and hjd_plan_coef_bytes 128 x the
 * blocks read. */
int hjd_plan_create_roi(hjd_ctx* ctx, const hjd_frame* frames, int nframes, int input_format,
                        const int32_t* qtables, int nq, int scale, const hjd_rect* rois, hjd_plan** out);
int hjd_plan_has_roi(const hjd_plan* plan);        /* 1: created with rois */
/* Validates one frame's geometry and output layout (format, out_pitch,
 * out_offset, the input format it can take) exactly as hjd_plan_create_roi
 * would for a plan of `scale` with `roi` (NULL: none).  Host only: needs no
 * device. */
int hjd_frame_check(const hjd_frame* frame, int input_format, int scale, const hjd_rect* roi);
/* The constants of a HJD_OUT_RGB_PLANAR_F16 / _F32 plan, per channel R, G, B
 * (see hjd_out_format): out = fma((float)u8, a[c], b[c]).  A new plan has
 * a = 1, b = 0.  ToTensor is a = 1/255, b = 0; mean/std normalisation
 * a = 1/(255 std), b = -mean/std.  Synchronous (waits for the device, then
 * updates the plan's table); applies to the launches that follow.
 * HJD_E_INVALID for non-finite constants and for a plan of a byte format. */
int hjd_plan_set_normalize(hjd_plan* plan, const float a[3], const float b[3]);
int hjd_plan_destroy(hjd_plan* plan);
/* Tuning hook: kernel variant bits (0 = default).  bit 0: plain instead of
 * non-temporal output stores; bit 1: workgroup-interleaved task order.
 * Results are identical for every variant.  BGRX only: a BGR24 plan fails at
 * launch, an RGB24 / planar RGB plan here (HJD_E_INVALID). */
int hjd_plan_set_variant(hjd_plan* plan, int variant);
int hjd_plan_set_kernel(hjd_plan* plan, int mode);   /* hjd_kernel_mode */
/* Pin the persistent kernel's task chunk without hjd_plan_autotune: exactly
 * `tasks` consecutive tasks per wave (1..4096, no occupancy floor; 0 restores
 * the shape default, which never drops below ~4 waves per SIMD).  Applies to
 * launches that take the persistent kernel: an HJD_KERNEL_AUTO plan small
 * enough for the latency kernel keeps it.  Identical pixels either way. */
int hjd_plan_set_chunk(hjd_plan* plan, int tasks);
int64_t hjd_plan_tasks(const hjd_plan* plan);      /* work items (strips) */
int64_t hjd_plan_pixels(const hjd_plan* plan);     /* visible output pixels (a scaled plan: of the scaled size) */
int64_t hjd_plan_coef_bytes(const hjd_plan* plan); /* algorithmic input bytes */

/*
 * Enqueue the fused decode of every frame of the plan on `stream` (async).
 * d_coefs: coefficient buffer (int16 or int32 per the plan's format);
 * d_out: output buffer (frames at their out_offset).  Both 16-byte aligned.
 * grid_blocks: grid size in 256-thread workgroups; 0 = default (short task
 * chunks per wave over many more groups than are resident, which keeps the
 * resident waves inside a narrow window of the batch).
 * The input is never modified (the reference kernel's in-place IDCT,
 * src/idct8x8.cl:136-155, is not reproduced).
 */
int hjd_plan_launch(hjd_plan* plan, const void* d_coefs, void* d_out, void* stream, int grid_blocks);

/*
 * Adapt the plan's launch to this device (synchronous, setup time): times
 * every candidate launch shape -- chunks of 1, 2, 4, 8 or 16 tasks per wave,
 * each with nt or plain output stores (BGRX) -- with the plan's own buffers,
 * `rounds`
 * interleaved rounds (0 = 2) of one warm and two timed launches each, and
 * keeps the fastest for the plan's later launches with grid_blocks = 0.
 * Every candidate writes identical pixels (d_out holds a valid decode on
 * return unless the choice came from the cache, below).  Plans the latency
 * kernel serves are left unchanged.  Optional
 * outputs: the chosen tasks per wave (0 = unchanged) and the variant bits.
 */
int hjd_plan_autotune(hjd_plan* plan, const void* d_coefs, void* d_out, void* stream, int rounds,
                      int32_t* tasks_per_wave, int32_t* variant);
/* hjd_plan_autotune's choice is cached per process (device x sampling x
 * input format x output format x the other variant bits x frame count x
 * task count x scale):
 * a later plan of the same key takes it with no launch (and d_out is then NOT
 * written).  HJD_AUTOTUNE_CACHE=0 disables the cache; this empties it. */
int hjd_autotune_cache_clear(void);

/* The launch shape a plan's next hjd_plan_launch(grid_blocks = 0) uses. */
typedef struct hjd_launch_shape {
    int32_t kernel;             /* HJD_KERNEL_PERSISTENT or HJD_KERNEL_LATENCY */
    int32_t tasks_per_wave;     /* persistent: the chunk asked for (pinned, tuned or the shape default) */
    int32_t max_tasks_per_wave; /* persistent: the most tasks one wave takes with that grid */
    int32_t grid;               /* workgroups (latency: one per task) */
    int32_t variant;            /* variant bits */
    int32_t autotune_launches;  /* kernel launches the last hjd_plan_autotune made (0: none or cached) */
    int32_t autotune_cached;    /* 1: the last hjd_plan_autotune reused a cached choice */
} hjd_launch_shape;
int hjd_plan_launch_shape(const hjd_plan* plan, hjd_launch_shape* out);

/*
 * Resize (extension; the reference has none): n planar uint8 RGB images, each
 * of its own size, resampled to one common out_w x out_h in ONE launch, so
 * that crops of different sizes become one (N, 3, out_h, out_w) batch.
 *
 * Source: three uint8 planes R, G, B of src_w x src_h as HJD_OUT_RGB_PLANAR
 * writes them: rows src_pitch bytes apart, planes src_pitch * src_h apart;
 * any pointer and any src_pitch >= src_w.  All four dimensions lie in
 * 1..16384 (every expression below then fits 32-bit arithmetic).  Pinned on
 * the device for the resize, its antialiased filter, hjd_orient_* and
 * hjd_warp_* (tests/test_gpu_stage_limits.py): dimensions of 16384, the
 * antialiased filter's edge, and src_pitch / out_pitch of 2^30 bytes, whose row
 * and plane offsets (64-bit in these kernels: no upper bound on their pitches)
 * pass 2^32 inside one image.
 *
 * Definition (exact, integer): bilinear with half-pixel centres
 * (align_corners = false), 11-bit weights, no antialiasing.  Per axis (x
 * shown; y the same with src_h, out_h, i), for output column j:
 *     n  = max((2j + 1) * src_w - out_w, 0)       den = 2 * out_w
 *     x0 = n / den (floor)      fx = ((n mod den) * 2048) / den (floor)
 *     x1 = min(x0 + 1, src_w - 1)
 * and per channel, with A = src[y0][x0], B = src[y0][x1], C = src[y1][x0],
 * D = src[y1][x1]:
 *     u8 = (A (2048-fx)(2048-fy) + B fx (2048-fy) + C (2048-fx) fy + D fx fy
 *           + 2^21) >> 22
 * -- one rounding.  With out_w == src_w and out_h == src_h the result is the
 * source, byte for byte.  flags bit 0 (horizontal flip): output column j
 * holds the unflipped result's column out_w - 1 - j.  Other bits must be 0.
 * Plain bilinear aliases beyond a 2x reduction: decode at the scale (1/2,
 * 1/4, 1/8 box means, hjd_plan_create_scaled) that leaves the crop at most
 * 2x the target, then resize.
 *
 * Output: out_format is HJD_OUT_RGB_PLANAR (the bytes u8),
 * HJD_OUT_RGB_PLANAR_F16 or _F32 (fma((float)u8, a[c], b[c]) as hjd_out_format
 * defines it, both roundings of F16 included; hjd_resize_set_normalize, default
 * a = 1, b = 0); anything else is HJD_E_INVALID.  Item i's plane R starts at
 * dst, rows out_pitch bytes apart (>= out_w x the element size and a multiple
 * of it, like dst), planes out_pitch * out_h apart.  An item whose dst and
 * out_pitch are multiples of 4 (bytes), 8 (F16) or 16 (F32), with out_w % 4 ==
 * 0, is written with one dword / dwordx2 / dwordx4 store per plane and four
 * pixels; any other with guarded element stores.  Sources and outputs must
 * not overlap.
 */
typedef struct hjd_resize_item {
    const void* src;   /* device: plane R of the source */
    void* dst;         /* device: plane R of this item's output */
    int32_t src_w, src_h, src_pitch, flags;
} hjd_resize_item;
typedef struct hjd_resize hjd_resize;
/* Validates what hjd_resize_create would take.  HJD_E_INVALID (with a message)
 * for n outside 1..2^20, a NULL items / src / dst, a dimension outside
 * 1..16384, src_pitch < src_w, a bad out_pitch or dst alignment, a non-planar
 * or unknown format and unknown flag bits.  Host only: needs no device. */
int hjd_resize_check(const hjd_resize_item* items, int n, int out_w, int out_h, int out_pitch, int out_format);
/* Validates and uploads the item table (synchronously). */
int hjd_resize_create(hjd_ctx* ctx, const hjd_resize_item* items, int n, int out_w, int out_h, int out_pitch,
                      int out_format, hjd_resize** out);
/* The float formats' constants for the launches that follow (an enqueued
 * launch keeps its own).  HJD_E_INVALID for non-finite constants and for a
 * byte-format object. */
int hjd_resize_set_normalize(hjd_resize* r, const float a[3], const float b[3]);
/* Enqueue the resize of all n items on `stream` (asynchronous, one kernel). */
int hjd_resize_launch(hjd_resize* r, void* stream);
int hjd_resize_destroy(hjd_resize* r);

/*
 * The antialiased filter (HJD_RESIZE_TRIANGLE_AA): what Resize(antialias=True)
 * of an image library computes, as an exact integer definition.  Sources,
 * flags, output formats, pitches and store forms are those above; only the
 * resampling differs.
 *
 * Definition: the triangle (bilinear) filter widened to the reduction,
 * separable -- a horizontal pass over every source row, its result rounded to
 * uint8, then a vertical pass, rounded again (as Pillow's and torch's uint8
 * paths).  One axis, source size w, output size Wo, output index j (y the
 * same with src_h, out_h, i):
 *     S   = max(w, Wo)
 *     d_k = (2k + 1) Wo - (2j + 1) w            for source index k, 0 <= k < w
 *     t_k = 2S - |d_k|                          the taps are exactly the k with t_k > 0
 *     T   = sum of t_k over the taps
 *     u8  = floor((sum of t_k p_k + floor(T / 2)) / T)
 * -- the triangle centred at (2j + 1) w / (2 Wo) with support max(w / Wo, 1),
 * its weights exact rationals renormalised over the taps inside the image:
 * interpolate(mode = "bilinear", antialias = true, align_corners = false)
 * without its float rounding.  For Wo >= w it is exact two-tap bilinear
 * (T = 2 Wo where neither tap falls outside the image), for Wo == w the
 * identity; the centre tap always lies inside the image, so T > 0.  flags
 * bit 0: output column j holds the unflipped result's column out_w - 1 - j
 * (applied in the horizontal pass).  The float formats are
 * fma((float)u8, a[c], b[c]) of the final bytes.
 *
 * 32-bit bound: (2j + 1) w + 2S < 2^31 for dimensions up to 16384, and
 * T <= 2 S^2 / Wo + 2S, so the accumulator 255 T + T / 2 stays below 2^31
 * whenever S^2 <= 2^21 Wo.  That is the filter's one extra rule, per axis,
 * compared in 64 bits: src_w^2 <= 2^21 out_w and src_h^2 <= 2^21 out_h, else
 * HJD_E_INVALID with a message naming the axis (a 16384-wide source needs
 * out_w >= 128; everything up to 1448 wide may go to 1 pixel).
 *
 * Two launches on the same stream through a uint8 intermediate in device
 * memory (per item three planes of src_h rows x out_w bytes, the pitch out_w
 * rounded up to 4, each item 16-byte aligned).  An hjd_resize object of this
 * filter allocates its intermediate at create (HJD_E_NOMEM if that fails;
 * nothing is leaked) and hjd_resize_destroy frees it; set_normalize, launch
 * and destroy work on it unchanged.  All launches of one such object share
 * that intermediate: the caller orders them (the same stream, or events).
 *
 * hjd_resize_check_filter / hjd_resize_create_filter with filter ==
 * HJD_RESIZE_BILINEAR are exactly hjd_resize_check / hjd_resize_create; any
 * filter other than the two is HJD_E_INVALID.
 */
enum { HJD_RESIZE_BILINEAR = 0, HJD_RESIZE_TRIANGLE_AA = 1 };
int hjd_resize_check_filter(const hjd_resize_item* items, int n, int out_w, int out_h, int out_pitch, int out_format,
                            int filter);
int hjd_resize_create_filter(hjd_ctx* ctx, const hjd_resize_item* items, int n, int out_w, int out_h, int out_pitch,
                             int out_format, int filter, hjd_resize** out);

/*
 * Orientation (extension; the reference has none): n planar uint8 RGB images,
 * each of its own size, permuted by their EXIF Orientation value in ONE
 * launch.  What ImageOps.exif_transpose of an image library computes.
 *
 * Definition.  S is the stored image, h rows by w columns; D the displayed
 * (oriented) image, for orientation o:
 *
 *     o   D[i][j] =            size of D (rows x columns)
 *     1   S[i][j]              h x w
 *     2   S[i][w-1-j]          h x w
 *     3   S[h-1-i][w-1-j]      h x w
 *     4   S[h-1-i][j]          h x w
 *     5   S[j][i]              w x h
 *     6   S[h-1-j][i]          w x h
 *     7   S[h-1-j][w-1-i]      w x h
 *     8   S[j][w-1-i]          w x h
 *
 * per plane: a pure permutation of bytes, exact.  Under a decode scale S is
 * the scaled decode (ceil(W / s) x ceil(H / s)) and D its permutation.
 *
 * Source: as the resize's -- three uint8 planes R, G, B of src_w x src_h as
 * HJD_OUT_RGB_PLANAR writes them, rows src_pitch bytes apart, planes
 * src_pitch * src_h apart; any pointer and any src_pitch >= src_w; both
 * dimensions in 1..16384.  Orientation 1 is legal: a copy.
 *
 * Output: out_format is HJD_OUT_RGB_PLANAR (the bytes), HJD_OUT_RGB_PLANAR_F16
 * or _F32 (fma((float)u8, a[c], b[c]) as hjd_out_format defines it, both
 * roundings of F16 included; hjd_orient_set_normalize, default a = 1, b = 0);
 * anything else is HJD_E_INVALID.  Every item carries its own dst_pitch: plane
 * R of D starts at dst, rows dst_pitch bytes apart, planes dst_pitch * (D's
 * rows) apart; dst and dst_pitch are multiples of the element size and
 * dst_pitch >= D's columns x the element size.  reserved must be 0.  Whole
 * dwords move on the side (source, output) whose base and pitch are multiples
 * of 4 bytes (the output's: of 4 elements), in every 128 x 128 tile none of
 * whose dwords straddles the image's edge; every other tile takes guarded byte
 * loads / element stores.  Nothing outside D's own elements is written.
 * Sources may overlap each other; an output may overlap neither a source nor
 * another output (hjd_orient_check refuses it).
 *
 * hjd_orient_roi: the rectangle on S that holds the pixels of `display`, a
 * rectangle on D, for a stored frame of width x height (already scaled):
 * orient(S restricted to *stored, o) == orient(S, o) restricted to *display.
 * With (x, y, w, h) = *display, W = width, H = height:
 *     1 (x, y, w, h)            2 (W-x-w, y, w, h)
 *     3 (W-x-w, H-y-h, w, h)    4 (x, H-y-h, w, h)
 *     5 (y, x, h, w)            6 (y, H-x-w, h, w)
 *     7 (W-y-h, H-x-w, h, w)    8 (W-y-h, x, h, w)
 * HJD_E_INVALID for a NULL, width or height < 1, an orientation outside 1..8
 * and a rectangle that is empty or not inside D.  Host only.
 */
typedef struct hjd_orient_item {
    const void* src;   /* device: plane R of the stored image */
    void* dst;         /* device: plane R of the oriented image */
    int32_t src_w, src_h, src_pitch, orientation;
    int32_t dst_pitch; /* bytes between the oriented image's rows */
    int32_t reserved;  /* 0 */
} hjd_orient_item;
typedef struct hjd_orient hjd_orient;
int hjd_orient_roi(int width, int height, int orientation, const hjd_rect* display, hjd_rect* stored);
/* Validates what hjd_orient_create would take.  HJD_E_INVALID (with a message)
 * for n outside 1..2^20, a NULL items / src / dst, a dimension outside
 * 1..16384, src_pitch < src_w, an orientation outside 1..8, a bad dst_pitch or
 * dst alignment, a non-zero reserved, a non-planar or unknown format, more
 * than 2^31 - 1 tiles of 128 x 128 in all, and an output that overlaps a source
 * or another output.  Host only: needs no device. */
int hjd_orient_check(const hjd_orient_item* items, int n, int out_format);
/* Validates and uploads the item table (synchronously). */
int hjd_orient_create(hjd_ctx* ctx, const hjd_orient_item* items, int n, int out_format, hjd_orient** out);
/* The float formats' constants for the launches that follow (an enqueued
 * launch keeps its own).  HJD_E_INVALID for non-finite constants and for a
 * byte-format object. */
int hjd_orient_set_normalize(hjd_orient* r, const float a[3], const float b[3]);
/* Enqueue the orientation of all n items on `stream` (asynchronous, one kernel). */
int hjd_orient_launch(hjd_orient* r, void* stream);
int hjd_orient_destroy(hjd_orient* r);

/*
 * Affine warp (extension; the reference has none): n planar uint8 RGB images,
 * each of its own size, sampled through each image's own affine map to one
 * common out_w x out_h in ONE launch: rotation, shear, arbitrary zoom, flips
 * and translation -- the geometry of RandomAffine / RandomRotation -- into one
 * (N, 3, out_h, out_w) batch.  It subsumes the crop, the resize without
 * antialiasing, both flips and the eight orientations.
 *
 * Source and output: as the resize's.  Three uint8 planes R, G, B of src_w x
 * src_h, rows src_pitch bytes apart, planes src_pitch * src_h apart; any
 * pointer and any src_pitch >= src_w; dimensions in 1..16384.  A common out_w x
 * out_h and out_pitch for all n items; out_format HJD_OUT_RGB_PLANAR (the bytes
 * u8), HJD_OUT_RGB_PLANAR_F16 or _F32 (fma((float)u8, a[c], b[c]),
 * hjd_warp_set_normalize, default a = 1, b = 0); dst and out_pitch multiples of
 * the element size; the same rule decides between one vector store per plane
 * and four pixels and guarded element stores.  Sources and outputs must not
 * overlap.
 *
 * Definition (exact, integer).  m[6] is the INVERSE map, output to source, in
 * Q16 (units of 1/65536 source pixel).  For output column j and row i, in
 * 64-bit arithmetic:
 *     X  = m[0] * j + m[1] * i + m[2]        Y  = m[3] * j + m[4] * i + m[5]
 *     x0 = X >> 16 (floor)                   y0 = Y >> 16 (floor)
 *     fx = (X & 0xffff) >> 5                 fy = (Y & 0xffff) >> 5
 * X and Y are positions in source pixel INDICES: the centre of source pixel k
 * lies at k * 65536, so the caller folds the half-pixel offsets of a
 * centre-based map into m[2] and m[5].  fx, fy are the resize's 11-bit
 * weights.  With the taps A = (x0, y0), B = (x0 + 1, y0), C = (x0, y0 + 1),
 * D = (x0 + 1, y0 + 1), per channel:
 *     u8 = (A (2048-fx)(2048-fy) + B fx (2048-fy) + C (2048-fx) fy + D fx fy
 *           + 2^21) >> 22
 * -- the resize's expression, one rounding.
 *
 * Taps outside the image.  A tap whose column is outside 0 .. src_w - 1 or
 * whose row is outside 0 .. src_h - 1 is the channel's byte of `fill`
 * (0x00RRGGBB): grid_sample(padding_mode = "zeros") at fill 0, an image
 * library's masked fill otherwise.  With flags bit 0 (HJD_WARP_REPLICATE) the
 * tap's coordinates are clamped into the image instead (padding_mode =
 * "border").  A tap outside the image is never read from memory.  Other flag
 * bits and `reserved` must be 0, fill <= 0xFFFFFF.
 *
 * What it leaves out.  There is no antialiasing: beyond a 2x reduction, decode
 * at a scale first, as the resize says.  Q16 quantises a real matrix: with
 * every entry rounded to nearest, the position of output pixel (j, i) is off
 * by at most (j + i + 1) * 2^-17 source pixel per axis.  In terms of the
 * integer matrix the result is exact.
 *
 * Laws.  {65536, 0, tx << 16, 0, 65536, ty << 16} is the crop at (tx, ty), byte
 * for byte; {-65536, 0, (w - 1) << 16, 0, 65536, 0} the horizontal flip;
 * {0, 65536, 0, -65536, 0, (h - 1) << 16} with an h x w output orientation 6;
 * every orientation 1..8 is such an integer matrix (hjd_warp_orient of the
 * identity); an output wholly outside the image is all `fill`.
 *
 * hjd_warp_roi: the smallest rectangle of a width x height frame that holds
 * every tap an out_w x out_h output reads through m, after the tap range is
 * clamped into the frame.  X and Y are affine, so their extrema Xmin, Xmax,
 * Ymin, Ymax lie at the four output corners, and
 *     x_lo = clamp(Xmin >> 16, 0, width - 1)
 *     x_hi = clamp((Xmax >> 16) + 1, 0, width - 1)        (y the same)
 *     *out = (x_lo, y_lo, x_hi - x_lo + 1, y_hi - y_lo + 1)
 * The rectangle is never empty.  A tap inside the frame is inside it; a tap
 * outside the frame is outside it on a side where the rectangle touches the
 * frame's edge.  So, in both border modes, warping the frame's crop to *out
 * with m[2] - (x_lo << 16) and m[5] - (y_lo << 16) equals warping the frame.
 * HJD_E_INVALID for a NULL, width or height < 1 and an output dimension
 * outside 1..16384.  Host only.
 *
 * hjd_warp_orient: m addresses the DISPLAYED image of a stored_w x stored_h
 * image under `orientation` (the table above); out addresses the stored one.
 * With (x, y) a displayed position, the stored position (xs, ys) is
 *     1 (x, y)            2 (w - 1 - x, y)    3 (w - 1 - x, h - 1 - y)
 *     4 (x, h - 1 - y)    5 (y, x)            6 (y, h - 1 - x)
 *     7 (w - 1 - y, h - 1 - x)                8 (w - 1 - y, x)
 * so out's rows are rows of m, negated and offset by (w - 1) << 16 or
 * (h - 1) << 16: exact in integers.  HJD_E_INVALID if a composed entry leaves
 * int32, for an orientation outside 1..8, a NULL and a stored size < 1.  Because
 * fx and fy are truncated (a negated X rounds its weight the other way), the
 * oriented warp is DEFINED as the warp of the stored image by the composed
 * matrix.  It equals warp(orient(image)) exactly wherever X and Y are whole
 * pixels (integer-translation matrices); elsewhere each lies within
 * 0.5 + 2 * 255 / 2048 of the real-valued bilinear sample at the same position
 * (the weight truncation moves a position by less than 1/2048 pixel per axis,
 * bilinear is 255-Lipschitz per axis, the rounding adds 0.5).  Host only.
 */
enum { HJD_WARP_REPLICATE = 1 };
typedef struct hjd_warp_item {
    const void* src;   /* device: plane R of the source */
    void* dst;         /* device: plane R of this item's output */
    int32_t src_w, src_h, src_pitch, flags;   /* bit 0: HJD_WARP_REPLICATE; other bits 0 */
    int32_t m[6];      /* inverse map, Q16 (1/65536 source pixel) */
    uint32_t fill;     /* 0x00RRGGBB, <= 0xFFFFFF */
    int32_t reserved;  /* 0 */
} hjd_warp_item;       /* 64 bytes */
typedef struct hjd_warp hjd_warp;
int hjd_warp_roi(int width, int height, const int32_t m[6], int out_w, int out_h, hjd_rect* out);
int hjd_warp_orient(const int32_t m[6], int stored_w, int stored_h, int orientation, int32_t out[6]);
/* Validates what hjd_warp_create would take.  HJD_E_INVALID (with a message)
 * for n outside 1..2^20, a NULL items / src / dst, a dimension outside
 * 1..16384, src_pitch < src_w, unknown flag bits, fill > 0xFFFFFF, a non-zero
 * reserved, a bad out_pitch or dst alignment and a non-planar or unknown
 * format.  Host only: needs no device. */
int hjd_warp_check(const hjd_warp_item* items, int n, int out_w, int out_h, int out_pitch, int out_format);
/* Validates and uploads the item table (synchronously). */
int hjd_warp_create(hjd_ctx* ctx, const hjd_warp_item* items, int n, int out_w, int out_h, int out_pitch,
                    int out_format, hjd_warp** out);
/* The float formats' constants for the launches that follow (an enqueued
 * launch keeps its own).  HJD_E_INVALID for non-finite constants and for a
 * byte-format object. */
int hjd_warp_set_normalize(hjd_warp* w, const float a[3], const float b[3]);
/* Enqueue the warp of all n items on `stream` (asynchronous, one kernel). */
int hjd_warp_launch(hjd_warp* w, void* stream);
int hjd_warp_destroy(hjd_warp* w);

/*
 * Colour (extension; the reference has none): n planar uint8 RGB images, each
 * of its own size, each through its own affine colour map in ONE launch (two
 * where a map reads the image's means): brightness, contrast, saturation, a
 * hue rotation, grayscale and inversion -- the photometric half of ColorJitter
 * / RandomGrayscale -- composed into one record per image.
 *
 * Source: as the resize's -- three uint8 planes R, G, B of w x h, rows
 * src_pitch bytes apart, planes src_pitch * h apart; any pointer and any
 * src_pitch >= w; both dimensions in 1..16384.  Output: the same w x h, as
 * hjd_orient's: out_format HJD_OUT_RGB_PLANAR (the bytes u8),
 * HJD_OUT_RGB_PLANAR_F16 or _F32 (fma((float)u8, a[c], b[c]),
 * hjd_color_set_normalize, default a = 1, b = 0); every item its own dst and
 * dst_pitch, multiples of the element size, dst_pitch >= w x the element size;
 * planes dst_pitch * h apart.  One dword is read per plane and four pixels
 * where src and src_pitch are multiples of 4 and the four lie inside the row,
 * and one dword / dwordx2 / dwordx4 written where dst and dst_pitch are
 * multiples of 4 elements and w of 4; guarded byte loads / element stores
 * elsewhere.  Nothing outside the image's own elements is written.
 *
 * Definition (exact, integer).  A record is 21 int32: m[9], p[9], t[3].  m and
 * p are row-major 3 x 3 matrices, output channel x input channel in the order
 * R, G, B, in Q12 (4096 is 1.0), every entry in -32767..32767
 * (HJD_COLOR_MAX_COEF); t is in Q12 grey levels, |t| <= 2^23
 * (HJD_COLOR_MAX_OFFSET).  For an image of w x h, N = w * h, pixel (r, g, b):
 *     S_k  = the sum of channel k's bytes over the image           (exact, < 2^36)
 *     mq_k = (S_k * 256 + (N >> 1)) / N                            (floor: the mean in Q8)
 *     T_c  = t[c] + ((p[c][0] mq_0 + p[c][1] mq_1 + p[c][2] mq_2 + 128) >> 8)
 *     u8_c = clamp((m[c][0] r + m[c][1] g + m[c][2] b + T_c + 2048) >> 12, 0, 255)
 * with arithmetic (flooring) shifts; T_c in 64 bits, once per image.  Every
 * product of the last line fits a 24-bit multiply (|m| < 2^15, a byte < 2^8)
 * and the line fits int32: |m x| sums to at most 3 * 32767 * 255 < 2^25,
 * |T_c| <= 2^23 + (3 * 32767 * 65280 + 128) / 256 < 2^23 + 2^25.  The float
 * formats are fma((float)u8, a[c], b[c]) of those bytes.
 *
 * Laws.  m = 4096 I with p = t = 0 is a byte-for-byte copy; m = -4096 I with
 * t = 255 * 4096 is the inverse 255 - x; a record with p = 0 never reads the
 * sums (and its launch has no summing kernel).
 *
 * Error bound.  Against the real-valued map of the integer record,
 * y_c = (m[c] . x + p[c] . xbar) / 4096 + t[c] / 4096 with xbar = S / N, u8 is
 * within
 *     0.5 + 2^-13 + (sum over k of |p[c][k]| / 4096) * 2^-9
 * of clamp(y_c, 0, 255): mq_k / 256 is within 2^-9 of xbar_k (a rounding to
 * nearest in Q8), which p scales; the shift by 8 rounds T_c to nearest in Q12,
 * half a unit, 2^-13 grey level; the last shift rounds to nearest, 0.5; and the
 * clamp commutes with that rounding.  Where m, p, t are real coefficients
 * rounded to nearest in Q12, add (3 * 255 + 3 * 255 + 1) * 2^-13.
 *
 * What it leaves out.  The map is composed without clamping in between: an
 * image library that clamps after each operation agrees only while no
 * intermediate leaves 0..255.  A hue change is a rotation about the grey axis
 * in YIQ, not an HSV shift.  Operations that are not affine in RGB (posterize,
 * solarize, gamma, equalize) are not records: they, and autocontrast, are the
 * curves of hjd_tone below, which can run behind this stage.
 *
 * In place: for HJD_OUT_RGB_PLANAR an item with dst == src and dst_pitch ==
 * src_pitch is legal -- a thread reads its four pixels before it writes them
 * and the sums are taken by an earlier launch.  Any other overlap of an output
 * with a source or another output is the caller's error; it is not looked for.
 * An object whose records read the sums owns a table of partial sums (n x 256
 * x 3 uint32, allocated at create, HJD_E_NOMEM if that fails) which all its
 * launches share: the caller orders them (the same stream, or events).
 */
#define HJD_COLOR_MAX_COEF 32767
#define HJD_COLOR_MAX_OFFSET (1 << 23)
typedef struct hjd_color_item {
    const void* src;   /* device: plane R of the source */
    void* dst;         /* device: plane R of the output */
    int32_t w, h, src_pitch, dst_pitch;
    int32_t m[9], p[9], t[3];
    int32_t reserved;   /* 0 */
} hjd_color_item;       /* 120 bytes */
typedef struct hjd_color hjd_color;
/* Validates what hjd_color_create would take.  HJD_E_INVALID (with a message)
 * for n outside 1..2^20, a NULL items / src / dst, a dimension outside
 * 1..16384, src_pitch < w, a bad dst_pitch or dst alignment, an entry of m or
 * p outside +-32767, |t| > 2^23, a non-zero reserved and a non-planar or
 * unknown format.  Host only: needs no device. */
int hjd_color_check(const hjd_color_item* items, int n, int out_format);
/* Validates and uploads the item table (synchronously). */
int hjd_color_create(hjd_ctx* ctx, const hjd_color_item* items, int n, int out_format, hjd_color** out);
/* The float formats' constants for the launches that follow (an enqueued
 * launch keeps its own).  HJD_E_INVALID for non-finite constants and for a
 * byte-format object. */
int hjd_color_set_normalize(hjd_color* c, const float a[3], const float b[3]);
/* Enqueue the colour maps of all n items on `stream` (asynchronous; one
 * kernel, or two where a record's p is not 0). */
int hjd_color_launch(hjd_color* c, void* stream);
int hjd_color_destroy(hjd_color* c);

/*
 * Tone curves (extension; the reference has none): n planar uint8 RGB images,
 * each of its own size, each through its own pointwise map of a byte per
 * channel in ONE launch (three where a map is built from the image's
 * histogram): a 3 x 256 lookup table per image -- solarize, posterize, gamma,
 * inversion, any curve -- optionally preceded by autocontrast or equalize, the
 * photometric operations of RandAugment / AutoAugment / TrivialAugment that
 * are not affine in RGB.
 *
 * Source and output: exactly as hjd_color's -- three uint8 planes R, G, B of
 * w x h, rows src_pitch bytes apart, planes src_pitch * h apart, any pointer
 * and any src_pitch >= w, both dimensions in 1..16384; the same w x h out, in
 * HJD_OUT_RGB_PLANAR (the bytes u8), HJD_OUT_RGB_PLANAR_F16 or _F32
 * (fma((float)u8, a[c], b[c]), hjd_tone_set_normalize, default a = 1, b = 0);
 * every item its own dst and dst_pitch, multiples of the element size,
 * dst_pitch >= w x the element size, planes dst_pitch * h apart; dword loads
 * and vector stores under hjd_color's conditions, guarded byte loads and
 * element stores elsewhere.  Nothing outside the image's own elements is
 * written.
 *
 * Definition (exact, integer).  A curve is a mode and a table lut[3][256],
 * one row per channel R, G, B.  For an image of w x h, N = w * h <= 2^28, and
 * channel c:
 *     h_c[v] = the number of pixels of plane c whose byte is v   (v = 0..255)
 * over the image's own w columns of its h rows -- no padding, and not the
 * zeros a guarded load returns past column w.  The data curve D_c:
 *   mode 0, HJD_TONE_TABLE:  D_c[v] = v.
 *   mode 1, HJD_TONE_AUTOCONTRAST:  lo, hi the smallest and largest v with
 *     h_c[v] > 0.  hi == lo: D_c[v] = v.  Else D_c[v] = 0 for v <= lo, 255 for
 *     v >= hi, and floor(255 * (v - lo) / (hi - lo)) in between.
 *   mode 2, HJD_TONE_EQUALIZE:  last = h_c[hi], step = floor((N - last) / 255).
 *     Fewer than two non-empty bins (hi == lo), or step == 0: D_c[v] = v.
 *     Else D_c[v] = min(255, floor((floor(step / 2) + sum over k < v of h_c[k]) / step)).
 *     All of it fits uint32: step / 2 + the sum < 2^27 + 2^28.
 * The output byte is
 *     u8_c = lut[c][ D_c[x_c] ]
 * -- the data curve first, the table second -- and the float formats are
 * fma((float)u8, a[c], b[c]) of those bytes.
 *
 * Laws.  Mode 0 with lut[c][v] = v is a byte-for-byte copy.  A mode-0 record
 * never reads a histogram (and a launch whose records are all mode 0 is one
 * kernel).  A histogram is a sum of integer counts, which does not depend on
 * the order they are added in: every launch of the same images gives the same
 * bytes.
 *
 * Agreement with Pillow (12.2.0, checked on the CPU by tests/test_tone_cpu.py
 * where Pillow is installed).  ImageOps.equalize is mode 2 with the identity
 * table, bit for bit (the step == 0 and the few-valued cases included);
 * ImageOps.solarize and .posterize are mode-0 tables, bit for bit.
 * ImageOps.autocontrast evaluates int(v * (255.0 / (hi - lo)) - lo * scale) in
 * float64, which differs from the exact floor above by one grey level in
 * 12,094 of the 2,828,800 triples (lo, hi, v), never by more: mode 1 is the
 * exact floor, and that is the documented difference.
 *
 * What it leaves out.  autocontrast's `cutoff` (lo and hi are the extreme
 * non-empty bins); sharpness and blur, which are not pointwise (they are the
 * filters of hjd_conv below); and any order other than colour (hjd_color,
 * where a caller runs it first) -> data curve -> table: a table in front of
 * the data curve is not a record.
 *
 * In place: for HJD_OUT_RGB_PLANAR an item with dst == src and dst_pitch ==
 * src_pitch is legal -- a thread reads its four pixels before it writes them
 * and the histogram is taken by an earlier launch.  Any other overlap of an
 * output with a source or another output is the caller's error; it is not
 * looked for.  An object with a record of mode 1 or 2 owns a table of partial
 * histograms (n x 16 x 3 x 256 uint32) and one of curves (n x 768 bytes),
 * allocated at create (HJD_E_NOMEM if that fails), which all its launches
 * share: the caller orders them (the same stream, or events).  Every launch
 * writes what it reads of them: they are never cleared.
 */
enum { HJD_TONE_TABLE = 0, HJD_TONE_AUTOCONTRAST = 1, HJD_TONE_EQUALIZE = 2 };
typedef struct hjd_tone_curve {
    int32_t mode;       /* HJD_TONE_* */
    int32_t reserved;   /* 0 */
    uint8_t lut[3][256];
} hjd_tone_curve;       /* 776 bytes */
typedef struct hjd_tone_item {
    const void* src;   /* device: plane R of the source */
    void* dst;         /* device: plane R of the output */
    int32_t w, h, src_pitch, dst_pitch;
    hjd_tone_curve curve;
} hjd_tone_item;       /* 808 bytes */
typedef struct hjd_tone hjd_tone;
/* Validates what hjd_tone_create would take.  HJD_E_INVALID (with a message)
 * for n outside 1..2^20, a NULL items / src / dst, a dimension outside
 * 1..16384, src_pitch < w, a bad dst_pitch or dst alignment, a mode outside
 * 0..2, a non-zero reserved and a non-planar or unknown format.  Host only:
 * needs no device. */
int hjd_tone_check(const hjd_tone_item* items, int n, int out_format);
/* Validates and uploads the item table (synchronously). */
int hjd_tone_create(hjd_ctx* ctx, const hjd_tone_item* items, int n, int out_format, hjd_tone** out);
/* The float formats' constants for the launches that follow (an enqueued
 * launch keeps its own).  HJD_E_INVALID for non-finite constants and for a
 * byte-format object. */
int hjd_tone_set_normalize(hjd_tone* t, const float a[3], const float b[3]);
/* Enqueue the curves of all n items on `stream` (asynchronous; one kernel, or
 * three where a record's mode is not 0). */
int hjd_tone_launch(hjd_tone* t, void* stream);
int hjd_tone_destroy(hjd_tone* t);
/* The composed table lut_out[c][v] = lut_in[c][ D_c[v] ] of a curve of `mode`
 * on an image whose channel histograms are hist[c][.]: the arithmetic of the
 * definition above, by the one function the device's curve-building kernel
 * calls.  lut_in NULL: the identity table.  HJD_E_INVALID for a mode outside
 * 0..2, a NULL hist or lut_out and a channel whose counts sum above 2^28.
 * Host only: needs no device. */
int hjd_tone_curve_from_histogram(int mode, const uint32_t hist[3][256], const uint8_t lut_in[3][256],
                                  uint8_t lut_out[3][256]);

/*
 * Neighbourhood filters (extension; the reference has none): n planar uint8
 * RGB images, each of its own size, each through its own small separable
 * filter with a blend against the centre pixel, in ONE launch: sharpness (the
 * one operation of RandAugment / AutoAugment / TrivialAugment that is not
 * pointwise), Gaussian blur (SimCLR / BYOL / DINO: up to 23 taps), unsharp
 * masking.
 *
 * Source and output: exactly as hjd_color's and hjd_tone's -- three uint8
 * planes R, G, B of w x h, rows src_pitch bytes apart, planes src_pitch * h
 * apart, any pointer and any src_pitch >= w, both dimensions in 1..16384; the
 * same w x h out, in HJD_OUT_RGB_PLANAR (the bytes u8), HJD_OUT_RGB_PLANAR_F16
 * or _F32 (fma((float)u8, a[c], b[c]), hjd_conv_set_normalize, default a = 1,
 * b = 0); every item its own dst and dst_pitch, multiples of the element size,
 * dst_pitch >= w x the element size, planes dst_pitch * h apart.  Nothing
 * outside the image's own elements is written.
 *
 * Definition (exact, integer).  A filter is two radii rx, ry in 0..11, a
 * border rule, two rows of Q12 taps kh[0..2 rx], kv[0..2 ry] (the entries
 * beyond are 0; each row sums to 1..4096) and two Q12 gains a, b, |a|, |b| <=
 * 2^20.  Per plane, x the source byte at column j of row i:
 *     S  = sum over q = -ry..ry, p = -rx..rx of
 *          kv[q + ry] * kh[p + rx] * X(j + p, i + q)
 *          (<= 255 * 2^24: it fits uint32 and not int32)
 *     T  = a * (x << 24) + b * S            (int64, |T| < 2^53)
 *     u8 = clamp((T + 2^35) >> 36, 0, 255)  (an arithmetic shift: one rounding)
 * What X is outside the image, by `border`:
 *   HJD_CONV_REFLECT:  index -k -> k and n - 1 + k -> n - 1 - k (torch's
 *     "reflect", scipy's "mirror").  Needs rx < w and ry < h.
 *   HJD_CONV_REPLICATE:  the index is clamped to the edge.
 *   HJD_CONV_KEEP:  a pixel with j < rx, j >= w - rx, i < ry or i >= h - ry is
 *     copied (u8 = x); the others never read outside.  This is what Pillow's
 *     3 x 3 filters and torchvision's adjust_sharpness do.  With 2 rx >= w or
 *     2 ry >= h the whole image is copied.
 *
 * Laws.  rx = ry = 0, a = 4096, b = 0 (kh[0] = kv[0] = 4096) is the identity
 * record: a byte-for-byte copy.  Taps that sum to 4096 on both axes with a =
 * 0, b = 4096 give (S + 2^23) >> 24: a flat image stays flat, 255 included.
 * Channels are independent.  Every sum is of integers: no result depends on
 * the launch's shape or the order of the additions.
 *
 * Agreement with Pillow (12.2.0, checked on the CPU by tests/test_conv_cpu.py
 * where Pillow is installed).  ImageEnhance.Sharpness(im).enhance(f) blends
 * im with its SMOOTH filter ((box + 4 x) / 13 under KEEP): the record rx = ry
 * = 1, taps 1024 x 3 on both axes, a = round(4096 (4 + 9 f) / 13), b =
 * round(65536 (1 - f) / 13) is that real map f x + (1 - f) (box + 4 x) / 13
 * with one rounding, within 0.55 grey level of it.  Pillow rounds the smoothed
 * image and then truncates the blend, so the two differ by at most 2 for f in
 * 0..2 (asserted); measured over f in {0, 0.1, 0.5, 1, 1.5, 1.9, 2} on random,
 * checkerboard and 0/255 images the largest difference is 1, in 14.06 % of the
 * pixels overall (45.8 % at worst: f = 0.1 on a checkerboard), and none at
 * f = 0, 1 and 2.
 *
 * What it leaves out.  Pillow's ImageFilter.GaussianBlur, which is a repeated
 * box blur and not this map (the taps here are torchvision's sampled
 * Gaussian); kernels that are not "separable + centre"; radii above 11; median
 * and rank filters.
 *
 * Overlap: a filter cannot run in place, so dst == src is refused; any other
 * overlap of an output with a source or another output is the caller's error;
 * it is not looked for.  The tiles of all items of one object, 64 x 32 pixels
 * each, must number below 2^31.
 */
enum { HJD_CONV_KEEP = 0, HJD_CONV_REFLECT = 1, HJD_CONV_REPLICATE = 2 };
#define HJD_CONV_MAX_RADIUS 11            /* 23 taps per axis */
#define HJD_CONV_MAX_GAIN   (1 << 20)     /* |a|, |b| in Q12: up to +-256.0 */
typedef struct hjd_conv_filter {
    int32_t rx, ry;        /* 0..HJD_CONV_MAX_RADIUS */
    int32_t border;        /* HJD_CONV_* */
    int32_t a, b;          /* Q12 */
    int32_t reserved;      /* 0 */
    uint16_t kh[24], kv[24];   /* kh[0..2rx], kv[0..2ry]; the rest 0; each row sums to 1..4096 */
} hjd_conv_filter;         /* 120 bytes */
typedef struct hjd_conv_item {
    const void* src;   /* device: plane R of the source */
    void* dst;         /* device: plane R of the output */
    int32_t w, h, src_pitch, dst_pitch;
    hjd_conv_filter filter;
} hjd_conv_item;       /* 152 bytes */
typedef struct hjd_conv hjd_conv;
/* Validates what hjd_conv_create would take.  HJD_E_INVALID (with a message)
 * for n outside 1..2^20, a NULL items / src / dst, a dimension outside
 * 1..16384, src_pitch < w, a bad dst_pitch or dst alignment, dst == src, a
 * radius outside 0..11, a border outside 0..2, HJD_CONV_REFLECT with a radius
 * >= the dimension, a tap row summing to 0 or above 4096, a non-zero tap
 * beyond 2 r, |a| or |b| above 2^20, a non-zero reserved, a non-planar or
 * unknown format, and 2^31 tiles or more in all.  Host only: needs no device. */
int hjd_conv_check(const hjd_conv_item* items, int n, int out_format);
/* Validates and uploads the item table (synchronously). */
int hjd_conv_create(hjd_ctx* ctx, const hjd_conv_item* items, int n, int out_format, hjd_conv** out);
/* The float formats' constants for the launches that follow (an enqueued
 * launch keeps its own).  HJD_E_INVALID for non-finite constants and for a
 * byte-format object. */
int hjd_conv_set_normalize(hjd_conv* c, const float a[3], const float b[3]);
/* Enqueue the filters of all n items on `stream` (asynchronous; one kernel). */
int hjd_conv_launch(hjd_conv* c, void* stream);
int hjd_conv_destroy(hjd_conv* c);
/* The filter *f on one image of three planes on the host: src and dst as an
 * item's (planes src_pitch * h and dst_pitch * h apart, uint8 out), by the two
 * functions the device's kernel calls for the border and the finish.
 * HJD_E_INVALID for what hjd_conv_check refuses of the filter and the sizes.
 * Host only: needs no device. */
int hjd_conv_apply_host(const uint8_t* src, int w, int h, int src_pitch, const hjd_conv_filter* f, uint8_t* dst,
                        int dst_pitch);

/* IDCT only (the reference's batch_idct, src/idct8x8.cl:157-166), out of
 * place: int32 natural-order dequantised blocks -> int32 samples [-256,255]. */
int hjd_idct_blocks(hjd_ctx* ctx, const int32_t* d_in, int32_t* d_out, int64_t nblocks, void* stream);

/* The idct.h shim (include/idct.h) keeps its context, stream, grow-only device
 * buffers, plan cache and pinned staging alive across images: the reference
 * caller's clidct_clean_up (src/decoder.cpp:518-521) ends one image only.
 * This frees all of it (HJD_COMPAT_TEARDOWN=1 does so after every image, as
 * src/oclDCT8x8.cpp:316-341 did). */
int hjd_compat_release(void);

/* ---- test / measurement hooks (same device code as the fused kernel) ---- */
/* Colour stage alone over n (Y,U,V) triples: out[i] = BGRX.  mode 0 = the
 * kernel's exact-integer formulation, 1 = literal fp64 formulation. */
int hjd_debug_csc(hjd_ctx* ctx, const int32_t* d_y, const int32_t* d_u, const int32_t* d_v,
                  uint32_t* d_out, int64_t n, int mode, void* stream);
/* Exhaustive colour check: evaluates every (Y,U,V) in [-256,255]^3 on the
 * device and writes the 2^27 BGRX words to d_out (512 MiB). */
int hjd_debug_csc_exhaustive(hjd_ctx* ctx, uint32_t* d_out, int mode, void* stream);

/* Same-run measurement of the fused kernel's stages (bench.py): launch the
 * plan's persistent kernel with stages skipped.  Outputs are WRONG by design
 * (timing only).  stages: 80 = memory only (coefficient loads, staging, LDS
 * reads and BGRX stores kept; no IDCT, no colour math), 4 = no stores,
 * 16 = no IDCT, 64 = no colour math, 20 = no IDCT and no stores, 8 = no colour
 * stage, 24 = neither IDCT nor colour stage, 256 = every lane gathers row 0
 * of its block (the product's instructions without the zigzag gather's LDS
 * bank conflicts).  4:2:0 / 4:4:4, int16 zigzag
 * input, BGRX output only.  grid_blocks as hjd_plan_launch (0 = the plan's launch shape,
 * hjd_plan_autotune's if it ran). */
int hjd_debug_plan_launch_stages(hjd_plan* plan, int stages, const void* d_coefs, void* d_out, void* stream,
                                 int grid_blocks);

/* The box's streaming ceiling for a read:write byte mix (bench.py's
 * frac_of_box_ceiling): units of read_kib KiB read + write_kib KiB written
 * (16 B per lane, coalesced), units_per_wave consecutive units per wave, one
 * launch over min(src_bytes / read_kib KiB, dst_bytes / write_kib KiB) units.
 * flags bit 0: non-temporal loads and stores; bit 1: XCD-contiguous group
 * order (the fused kernel's); bit 2: pipelined (the next unit's loads issued
 * before this unit's stores, as the fused kernel prefetches its next task);
 * bit 3: image-row stores (the fused kernel's store geometry: dst as 3840-px
 * BGRX rows, pitch 15360 B, each unit one 512-B-wide strip of 2*write_kib
 * rows, two row segments per wave store instruction).  Mixes (KiB): 6:8 (4:2:0 task), 6:4 (4:4:4
 * task), 0:8, 6:0, 4:4, 3:4.  *units_out = units moved (bytes = units *
 * (read_kib + write_kib) KiB).  dst_bytes >= 1 KiB. */
int hjd_debug_rw_mix(hjd_ctx* ctx, const void* d_src, void* d_dst, int64_t src_bytes, int64_t dst_bytes,
                     int read_kib, int write_kib, int units_per_wave, int flags, void* stream, int64_t* units_out);

/* Clock probe: one wave on `stream` samples the shader clock counter and the
 * 100-MHz real-time counter every interval_ticks (>= 100) real-time ticks,
 * nsamples times: d_out[2i] = real-time ticks, d_out[2i+1] = shader cycles
 * (2 * nsamples uint64 words).  Launched beside a kernel on another stream,
 * consecutive samples give the clock the chip holds under that load
 * (delta cycles / delta ticks * 100 MHz).  Ends after nsamples intervals. */
int hjd_debug_clock_probe(hjd_ctx* ctx, uint64_t* d_out, int nsamples, int interval_ticks, void* stream);

/* The 4:4:4 kernels' d16 gather (ds_read_u16_d16_hi) is valid only where that
 * load zeroes the low half of its destination.  *probe_zeroes: the one-wave
 * hardware probe's answer for `device` (hjd_ctx_create runs it; a completed
 * run is cached per device, a failed one reads 0 and is retried; HJD_D16_PROBE=
 * fail forces 0); *selected: whether the 4:4:4 launches take the d16 kernels
 * (the cached probe passed, and HJD_D16 is not 0). */
int hjd_debug_d16_gather(int device, int* probe_zeroes, int* selected);

/* The library reads its HJD_* environment overrides once, at its first use
 * (the list: INTEGRATION.md s7, and the kTuning table in csrc/hjd_runtime.hip).
 * This switches one of them in-process, for tests and tools: `name` is the
 * environment variable's name, `value` is parsed as that variable's string
 * would be, and value = NULL restores what the process started with.  The
 * overrides are process-wide; any thread may call this at any time.  An
 * unknown name returns HJD_E_INVALID. */
int hjd_debug_set_tuning(const char* name, const char* value);

/* The library's pixel kernels are one table keyed by their template arguments
 * {latency (1: decode_kernel_lat, 0: decode_kernel), sampling index S, input
 * format F, variant word V}.  hjd_debug_kernel_key checks a launch shape as a
 * launch would and selects its entry, with `d16` in place of the device's
 * probe (hjd_debug_d16_gather's `selected`); it launches nothing.  stages: as
 * hjd_debug_plan_launch_stages, or 0.  key[4] = the entry's {latency, S, F, V};
 * HJD_E_INVALID for a shape no kernel serves.  hjd_debug_kernel_table writes
 * the keys of the table, four ints each and at most `cap` of them (keys may be
 * NULL), and returns their count.  Neither needs a GPU. */
int hjd_debug_kernel_key(int sampling, int input_format, int out_format, int scale, int roi, int variant, int stages,
                         int kernel_mode, int64_t tasks, int grid_blocks, int d16, int32_t key[4]);
int hjd_debug_kernel_table(int32_t* keys, int cap);

/* Timing only: enqueue ONE of the two launches of an HJD_RESIZE_TRIANGLE_AA
 * object -- pass 0 the horizontal kernel (sources -> intermediate), pass 1 the
 * vertical one (intermediate -> outputs, reading whatever the intermediate
 * holds).  HJD_E_INVALID for another pass or a bilinear object. */
int hjd_debug_resize_launch_pass(hjd_resize* r, int pass, void* stream);

/* Timing only: hjd_warp_launch with the way the output is dealt to the waves
 * given -- 0: a wave takes 64 consecutive quads of a row (the resize's way),
 * 1: a wave takes a tile of 8 quads x 8 rows.  The results are the same bytes.
 * HJD_E_INVALID for another value. */
int hjd_debug_warp_launch_form(hjd_warp* w, int tiled, void* stream);

#ifdef __cplusplus
}
#endif
#endif
