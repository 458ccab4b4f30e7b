/*
 * hjd_host.h -- host JPEG front end of the MI355X pixel back-end (C ABI).
 *
 * Baseline-JPEG marker parsing and Huffman (entropy) decoding on the CPU,
 * producing exactly the input of the fused kernel: int16 quantised
 * coefficients in zigzag order, MCU-major, with DC prediction applied
 * (src/decoder.cpp:221-346 of xinfushe/oclJPEGDecoder), plus the frame's
 * quantisation tables in file order.  Supports what the reference supports
 * (src/decoder.cpp:18-70): 8-bit samples, 3 components, 4:2:0 (H2V2,H1V1,H1V1)
 * or 4:4:4, restart intervals (DRI/RSTn).  Deliberate differences from the
 * reference parser, all of them fixes: 16-bit DQT entries are read big-endian
 * (src/parser.cpp:83-86 reads them native-endian); scan components are matched
 * to frame components by id (src/decoder.cpp:315 assumes equal order); APPn,
 * COM and other non-frame markers are skipped anywhere before SOS.
 *
 * Also: a stream object that pipelines host Huffman decoding (worker
 * threads), pinned host staging, hipMemcpyAsync H2D on a copy stream and the
 * fused kernel on a compute stream (double/triple buffering).
 */
#ifndef HJD_HOST_H
#define HJD_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "hjd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hjd_jpeg_info {
    int32_t width;
    int32_t height;
    int32_t sampling;          /* HJD_YUV444, HJD_YUV420, HJD_YUV422 or HJD_GRAY */
    int32_t restart_interval;  /* MCUs per restart interval, 0 = none */
    int32_t mcu_w;             /* MCU grid */
    int32_t mcu_h;
    int64_t nblocks;           /* coefficient blocks (64 int16 each) */
    int32_t qt[3][64];         /* quantisation table of each component, file (zigzag) order */
    int32_t qt_precision[3];   /* 0 = 8-bit DQT entries, 1 = 16-bit */
    int64_t scan_offset;       /* byte offset of the (first) entropy-coded segment */
    int32_t process;           /* 0 = baseline (SOF0), 1 = extended sequential (SOF1), 2 = progressive (SOF2) */
    int32_t single_scan;       /* 1: one interleaved sequential scan holds the image (0: several scans, or progressive;
                                  the GPU entropy decoder takes every sequential file, process 0 or 1) */
} hjd_jpeg_info;

/* Besides the reference's single interleaved baseline scan, the host decoder
 * takes sequential files with several scans (SOF0/SOF1: non-interleaved or
 * partly interleaved components) and progressive files (SOF2: spectral
 * selection + successive approximation, EOB runs, restarts); the result is the
 * same coefficient layout.  For those, qt[] is final after decode (tables
 * latch at each component's first scan). */

/* Parse headers up to SOS.  Returns HJD_OK, or HJD_E_INVALID for malformed or
 * unsupported files (hjd_last_error() says why). */
int hjd_jpeg_parse(const uint8_t* data, size_t size, hjd_jpeg_info* info);

/* The EXIF Orientation of a file (include/hjd.h hjd_orient_item defines what
 * the values 1..8 mean): the marker segments before the first SOS are walked,
 * the first APP1 whose payload starts with "Exif\0\0" is taken, its TIFF
 * header read ("II" or "MM", magic 42, the offset of IFD0) and IFD0's 12-byte
 * entries searched for tag 0x0112 of type SHORT and count 1, in the header's
 * byte order.  A value in 1..8 is returned in *orientation.  Everything else
 * gives 1 and HJD_OK, never an error -- no APP1, none with Exif, a bad byte
 * order or magic, an offset, entry count or entry past the segment, another
 * type or count, a value outside 1..8 -- so a broken EXIF block never makes an
 * image undecodable; every read is checked against the segment.  Only a file
 * that is not a JPEG up to there (SOI missing, a truncated segment or bad
 * segment length, no SOS) returns the parser's HJD_E_INVALID. */
int hjd_jpeg_orientation(const uint8_t* data, size_t size, int32_t* orientation);

/* Parse + Huffman-decode one file into coefs (capacity in blocks). */
int hjd_jpeg_decode_coefs(const uint8_t* data, size_t size, hjd_jpeg_info* info, int16_t* coefs,
                          int64_t capacity_blocks);

/* The calling process's CPU share: the CPUs in its affinity mask, capped by
 * its cgroup's CPU quota, rounded up (the cgroup of /proc/self/cgroup and its
 * ancestors; v2 cpu.max or v1 cpu.cfs_quota_us / cpu.cfs_period_us; computed
 * once per process).  A container granted 16 CPUs of time on a 256-CPU host
 * gets 16, not 256.  The default thread count (nthreads = 0) of
 * hjd_jpeg_decode_batch; hjd_stream_create and hjd_gstream_create cap it by
 * the device's CPU slice (hjd_device_worker_cpus). */
int hjd_host_cpu_share(void);
/* hjd_host_cpu_share computed from the tree at `root` ("/proc/self/cgroup",
 * "/sys/fs/cgroup/..." under it; NULL = the real one, not cached): tests. */
int hjd_debug_cpu_share(const char* root);
/* The host CPUs the stream workers of HIP device `device` bind to: its NUMA
 * node's CPUs this process may use, split evenly among the node's visible
 * GPUs (hjd_debug_worker_cpus on the real topology).  Writes up to `capacity`
 * ids; *ncpus = how many (0: unknown topology, no binding). */
int hjd_device_worker_cpus(int device, int32_t* cpus, int capacity, int32_t* ncpus);

/* Decode n files on `nthreads` host threads (0 = hjd_host_cpu_share());
 * status[i] receives each file's return code.  Returns HJD_OK if all
 * succeeded. */
int hjd_jpeg_decode_batch(const uint8_t* const* datas, const size_t* sizes, int n, int16_t* const* coefs,
                          int64_t capacity_blocks, int nthreads, int32_t* status);

/* ---- streaming decode (host Huffman || H2D || kernel) ------------------- */
typedef struct hjd_stream hjd_stream;

/* nslots pinned staging slots of max_blocks coefficient blocks each (>= 2;
 * 3 = triple buffering); nthreads host Huffman workers (0 = hjd_host_cpu_share()
 * capped by the device's CPU slice, hjd_device_worker_cpus). */
int hjd_stream_create(hjd_ctx* ctx, int64_t max_blocks, int nslots, int nthreads, hjd_stream** out);
int hjd_stream_destroy(hjd_stream* s);

/* Queue one JPEG (the bytes must stay valid until hjd_stream_sync returns).
 * Its BGRX pixels are written to d_out (device memory, row pitch out_pitch
 * bytes) by the fused kernel once its coefficients reach the device. */
int hjd_stream_submit(hjd_stream* s, const uint8_t* data, size_t size, void* d_out, int32_t out_pitch);

/* Wait for every submitted image; returns the first error, if any.  stats (may
 * be NULL) receives {images, pixels, host_decode_ns, h2d_bytes, kernel_launches}. */
int hjd_stream_sync(hjd_stream* s, int64_t stats[5]);
/* Cumulative GPU-side busy time of the stream's jobs, complete as of the last
 * hjd_stream_sync: the sum of every upload's duration on the copy stream and
 * of every fused-kernel launch on the compute stream (HIP timing events).
 * Divided by a wall-clock interval it is the fraction of the time the host
 * Huffman workers kept the copy engine / the kernel fed. */
int hjd_stream_busy(hjd_stream* s, int64_t* h2d_busy_ns, int64_t* kernel_busy_ns);

/* Host CPUs of one GPU's worker pool (both stream kinds bind their workers to
 * them; HJD_NUMA=0 disables the binding): the GPUs on the same NUMA node, in
 * PCI bus-id order, split that node's CPUs into equal contiguous slices; with
 * fewer CPUs than GPUs they share the node.  This hook computes the split for
 * GPU `bus` among `gpus` from a sysfs tree at `sysfs_root` ("" or NULL: the
 * real one; a test passes a fake topology), optionally intersected with this
 * process's affinity.  Writes up to `capacity` CPU ids; *ncpus = how many
 * (0: unknown topology, no binding). */
int hjd_debug_worker_cpus(const char* sysfs_root, const char* bus, const char* const* gpus, int ngpus,
                          int only_allowed, int32_t* cpus, int capacity, int32_t* ncpus);
/* Pixel format of subsequent submits: HJD_OUT_BGRX (default), HJD_OUT_BGR24
 * (d_out 4-byte aligned, pitch >= 3*width), HJD_OUT_RGB24 (any d_out, any
 * pitch >= 3*width) or HJD_OUT_RGB_PLANAR (any d_out, any pitch >= width; the
 * three planes at d_out + c * pitch * height); jobs already queued keep theirs.
 * The float formats (HJD_OUT_RGB_PLANAR_F16 / _F32) are not served by streams:
 * HJD_E_INVALID. */
int hjd_stream_set_output_format(hjd_stream* s, int out_format);

/* ---- GPU entropy decoding ----------------------
 * Replaces the single-threaded scan decode of the reference
 * (src/decoder.cpp:221-365) with a parallel one on the GPU.  The host only
 * parses headers and copies each scan into pinned memory without byte
 * stuffing / RST markers (memcpy speed); the Huffman decode runs on the GPU as
 * a self-synchronising parallel decode verified from the frame start, so its
 * coefficients are identical to hjd_jpeg_decode_coefs on every valid file
 * (DESIGN.md s10).  The fused pixel kernel follows on the same stream. */
typedef struct hjd_gdec hjd_gdec;

/* Capacity: max_frames JPEGs per call whose coefficient blocks total at most
 * max_blocks.  max_scan_bytes = the total size of the files of a call (the
 * sum of sizes[]) is always enough, wherever the files lie in memory.  The
 * sum of their entropy-coded bytes is enough too: pinned files then take the
 * host destuff path where their raw scans (stuffing, restart markers and the
 * bytes after EOI included) would not fit, unless HJD_DESTUFF=device, which
 * reports the overflow.
 * sub_bits = bits per parallel subsequence (0 = default 1024; >= 32). */
int hjd_gdec_create(hjd_ctx* ctx, int max_frames, int64_t max_scan_bytes, int64_t max_blocks, int sub_bits,
                    hjd_gdec** out);
int hjd_gdec_destroy(hjd_gdec* g);

/* Decode n JPEGs to BGRX in device memory (d_outs[i], row pitch pitches[i];
 * 16-byte aligned).  Asynchronous on `stream` (hipStream_t, NULL = default);
 * the input bytes may be reused as soon as the call returns (for pinned input,
 * which the DMA reads in place, the call returns once those uploads have
 * landed; the kernels stay asynchronous).  A later call on
 * the same object waits (on the host) for this call's uploads and is ordered
 * (on the device) after its kernels, whatever stream it uses; hjd_gdec_sync
 * reports the statuses of the most recent call. */
int hjd_gdec_decode(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, void* const* d_outs,
                    const int32_t* pitches, void* stream);

/* Entropy decode only: int16 quantised zigzag coefficients (the HJD_IN_Q16_ZIGZAG
 * layout), frame i at block block_offsets[i] of d_coefs (16-byte aligned). */
int hjd_gdec_decode_coefs(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, int16_t* d_coefs,
                          int64_t* block_offsets, void* stream);

/* Wait for the last call.  status[i] (may be NULL): 0 = ok, else
 * HJD_GDEC_CORRUPT / HJD_GDEC_COUNT bits (HJD_GDEC_SEQUENTIAL is informational).
 * Returns HJD_E_INVALID if any frame's entropy data was corrupt. */
int hjd_gdec_sync(hjd_gdec* g, int32_t* status);

/* Pixel format of the following hjd_gdec_decode calls: HJD_OUT_BGRX (default),
 * HJD_OUT_BGR24 (include/hjd.h; 3-byte pixels, d_outs 4-byte aligned,
 * pitches >= 3*width, multiple of 4), HJD_OUT_RGB24 (any d_outs, any pitches
 * >= 3*width) or HJD_OUT_RGB_PLANAR (any d_outs, any pitches >= width; image
 * i's planes at d_outs[i] + c * pitches[i] * height).  The two RGB formats
 * take vector stores where pointer and pitch are multiples of 4 and byte
 * stores otherwise (include/hjd.h).  HJD_OUT_RGB_PLANAR_F16 / _F32: planes of
 * half / float elements normalised with the decoder's constants
 * (hjd_gdec_set_normalize); d_outs and pitches multiples of the element size,
 * pitches >= 2*width / 4*width bytes, vector stores where both are multiples
 * of 8 / 16. */
int hjd_gdec_set_output_format(hjd_gdec* g, int out_format);
/* The constants a[c], b[c] (R, G, B) of the float formats for the following
 * hjd_gdec_decode and hjd_gdec_decode_roi calls: out = fma((float)u8, a[c],
 * b[c]) (include/hjd.h, hjd_out_format).  Default a = 1, b = 0; they are kept
 * across format changes and ignored by the byte formats.  An issued call
 * keeps its constants.  HJD_E_INVALID for non-finite values. */
int hjd_gdec_set_normalize(hjd_gdec* g, const float a[3], const float b[3]);
/* Decode scale of the following hjd_gdec_decode calls: 1 (default), 2, 4 or 8
 * (the scaled decode of include/hjd.h, hjd_plan_create_scaled).  Image i comes
 * out ceil(width/scale) x ceil(height/scale); pitches[] and the planar plane
 * stride refer to that size.  An issued call keeps its scale.  A scaled call
 * holding a 4:2:2, 4:1:1 or 4:4:0 file fails (HJD_E_INVALID) before anything
 * is enqueued.  hjd_gdec_decode_coefs is unaffected. */
int hjd_gdec_set_scale(hjd_gdec* g, int scale);
/* hjd_gdec_decode with one region of interest per image (include/hjd.h,
 * hjd_plan_create_roi): rois[i] is a rectangle on image i's output grid at the
 * decoder's current scale, image i comes out rois[i].w x rois[i].h with its
 * pixel (x, y) at d_outs[i], and pitches[] and the planar plane stride refer
 * to the ROI.  The entropy decode still covers the whole scan; only the pixel
 * kernel and the output shrink.  A call with an invalid rectangle, or one
 * combining scale > 1 with a 4:2:2, 4:1:1 or 4:4:0 file, fails
 * (HJD_E_INVALID) before anything is enqueued. */
int hjd_gdec_decode_roi(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                        void* const* d_outs, const int32_t* pitches, void* stream);
/* Decode n JPEGs, crop each (rois[i] as hjd_gdec_decode_roi's; rois == NULL:
 * the whole frames at the decoder's scale), resize every crop to out_w x
 * out_h (include/hjd.h, hjd_resize_*: bilinear, 11-bit weights, no
 * antialiasing, dimensions 1..16384) and flip it where flags[i] bit 0 is set
 * (flags == NULL: none; other bits are HJD_E_INVALID).  Image i lands at
 * d_out + i * 3 * out_pitch * out_h: with out_pitch == out_w x the element
 * size, d_out is one contiguous (n, 3, out_h, out_w) batch.  The format is
 * the decoder's current one and must be planar (HJD_OUT_RGB_PLANAR, _F16 or
 * _F32: out_pitch and d_out follow hjd_resize_check's rules; any other format
 * is HJD_E_INVALID); the constants and the scale are the decoder's current
 * ones too.  A refused call (format, sizes, pitch, a rectangle, a scale the
 * file's sampling does not serve) enqueues nothing.
 *
 * The pixel kernels run as for hjd_gdec_decode_roi with HJD_OUT_RGB_PLANAR,
 * into a scratch buffer the decoder owns (each crop 16-byte aligned, its
 * pitch rounded up to 4, so whole strips keep their vector stores); one
 * resize launch for all n images follows on the same stream.  The scratch
 * only grows: a call that needs more than the decoder holds waits for the
 * previous call (a host synchronisation) and reallocates; calls that fit are
 * asynchronous as hjd_gdec_decode.  hjd_gdec_destroy frees it.  The streams
 * (hjd_stream, hjd_gstream) do not serve a resized decode. */
int hjd_gdec_decode_resized(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                            const int32_t* flags, void* d_out, int out_w, int out_h, int32_t out_pitch, void* stream);
/* hjd_gdec_decode_resized with the resize's filter (include/hjd.h):
 * HJD_RESIZE_BILINEAR is exactly the call above, HJD_RESIZE_TRIANGLE_AA the
 * antialiased triangle filter, any other value HJD_E_INVALID.  The
 * antialiased filter adds its ratio rule per image (crop_w^2 <= 2^21 out_w,
 * crop_h^2 <= 2^21 out_h), refused like everything else before anything is
 * staged, allocated or enqueued, and follows the pixel kernels with two
 * launches; their intermediate (hjd.h) lies behind the crops in the same
 * grow-only scratch, under the same rule: a call that must grow it waits for
 * the previous call and reallocates, calls that fit stay asynchronous. */
int hjd_gdec_decode_resized_filter(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                   const hjd_rect* rois, const int32_t* flags, void* d_out, int out_w, int out_h,
                                   int32_t out_pitch, int filter, void* stream);
/* hjd_gdec_decode / hjd_gdec_decode_roi with an EXIF orientation per frame
 * (include/hjd.h hjd_orient_item defines the values 1..8 and the oriented
 * image D; hjd_jpeg_orientation reads a file's): d_outs[i] receives D of frame
 * i in the decoder's format, which must be HJD_OUT_RGB_PLANAR, _F16 or _F32
 * (any other is HJD_E_INVALID), rows pitches[i] apart (>= D's columns x the
 * element size).  rois may be NULL; if given, rois[i] is a rectangle on D
 * (display coordinates) and d_outs[i] receives that part of D: the stored
 * rectangle that holds it (hjd_orient_roi) is what is decoded.  Under a scale
 * D is the permutation of the scaled decode.
 *
 * A call whose orientations are all 1 is exactly hjd_gdec_decode /
 * hjd_gdec_decode_roi: no scratch, no extra launch.  In any other call every
 * frame, those of orientation 1 included, is decoded as planar bytes into the
 * decoder's grow-only scratch (as hjd_gdec_decode_resized's crops, under the
 * same growth rule) and one orient launch for all n frames follows on the same
 * stream and writes the outputs.  Everything that can refuse the call -- an
 * orientation outside 1..8, the format, a rectangle outside D, a scale the
 * file's sampling does not serve, an output pointer or pitch -- is checked
 * before anything is staged, allocated or enqueued. */
int hjd_gdec_decode_oriented(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                             const int32_t* orientations, void* const* d_outs, const int32_t* pitches, void* stream);
/* hjd_gdec_decode_resized_filter of the oriented images: the result is
 * resize(orient(decode)) for either filter; rois are rectangles on D, flags
 * flip D, and the antialiased filter's ratio rule applies to D's crop.  Built
 * as that composition: the stored crops are decoded into the scratch, one
 * orient launch writes the oriented crops (planar bytes) into a second region
 * of it, and the resize launches read those, unchanged.  All orientations 1:
 * exactly hjd_gdec_decode_resized_filter. */
int hjd_gdec_decode_resized_oriented(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                     const hjd_rect* rois, const int32_t* orientations, const int32_t* flags, void* d_out,
                                     int out_w, int out_h, int32_t out_pitch, int filter, void* stream);
/* Decode and warp (include/hjd.h hjd_warp_item defines the warp): frame i is
 * sampled through m[i], its inverse map in Q16, into image i of the batch at
 * d_out + i * 3 * out_pitch * out_h, under hjd_gdec_decode_resized's rules for
 * d_out, out_pitch, the format (the decoder's current one, planar), the
 * constants and the scale.  m[i] addresses the grid of the decoder's scale
 * (source pixel indices of the scaled decode), and of the DISPLAYED image where
 * orientations are given (orientations[i] in 1..8, NULL: all 1): the
 * orientation is folded into the matrix on the host (hjd_warp_orient), so an
 * oriented call costs no launch and no second scratch, and is defined as
 * hjd_warp_orient defines it.  flags[i] is hjd_warp_item's (bit 0
 * HJD_WARP_REPLICATE; NULL: all 0), fills[i] its fill (NULL: all 0).
 *
 * Only the part of a frame the warp reads is decoded: per frame the header is
 * parsed, the orientation composed, hjd_warp_roi taken on the scaled stored
 * frame and that rectangle decoded as hjd_gdec_decode_roi decodes one, as
 * planar bytes into the decoder's grow-only scratch (as
 * hjd_gdec_decode_resized's crops: 16-byte aligned, pitch rounded up to 4, the
 * same growth rule); the matrix's translation is shifted to the crop and ONE
 * warp launch for all n frames follows on the same stream.  Everything that
 * can refuse the call -- the format, sizes, pitch, an orientation, flag bits,
 * a fill above 0xFFFFFF, a composed or shifted entry that leaves int32
 * (HJD_E_INVALID naming the frame), a crop above 16384, a scale the file's
 * sampling does not serve -- is checked before anything is staged, allocated
 * or enqueued.  The streams do not serve a warped decode. */
int hjd_gdec_decode_warped(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const int32_t (*m)[6],
                           const int32_t* orientations, const int32_t* flags, const uint32_t* fills, void* d_out,
                           int out_w, int out_h, int32_t out_pitch, void* stream);
/* hjd_gdec_decode_resized_oriented / hjd_gdec_decode_warped with a colour
 * record per frame (include/hjd.h hjd_color_item defines the 21 words m[9],
 * p[9], t[3] and the map): image i of the batch is color(resize(orient(decode)))
 * or color(warp(decode)), the means of a record with p != 0 being those of the
 * resized or warped image.  orientations may be NULL in both (all 1).
 *
 * Built as that composition: the resize or warp launch writes planar bytes
 * (HJD_OUT_RGB_PLANAR) into one more region of the decoder's grow-only scratch,
 * laid out as one batch (pitch out_w rounded up to 4, images 3 * pitch * out_h
 * apart), and the colour launch reads that region and writes d_out in the
 * decoder's format with the decoder's constants.  Where a record's p is not 0
 * the table of partial sums lies in the same scratch and the summing kernel
 * runs between the two.  A call whose records are all the identity (m = 4096 I,
 * p = t = 0) is exactly the call without colours: no region, no launch.
 * Everything that can refuse the call -- all that the call without colours
 * refuses, a NULL colors, an entry of m or p outside +-32767 or |t| > 2^23
 * (HJD_E_INVALID naming the frame) -- is checked before anything is staged,
 * allocated or enqueued. */
int hjd_gdec_decode_resized_color(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                  const hjd_rect* rois, const int32_t* orientations, const int32_t* flags,
                                  const int32_t (*colors)[21], void* d_out, int out_w, int out_h, int32_t out_pitch,
                                  int filter, void* stream);
int hjd_gdec_decode_warped_color(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                 const int32_t (*m)[6], const int32_t* orientations, const int32_t* flags,
                                 const uint32_t* fills, const int32_t (*colors)[21], void* d_out, int out_w, int out_h,
                                 int32_t out_pitch, void* stream);
/* hjd_gdec_decode_resized_color / hjd_gdec_decode_warped_color with a tone
 * curve per frame behind the colour record (include/hjd.h hjd_tone_curve
 * defines the mode, the table and the map): image i of the batch is
 * tone(color(resize(orient(decode)))) or tone(color(warp(decode))), the
 * histogram of a curve of mode 1 or 2 being that of the image the tone stage
 * reads: resized or warped, its fill included, and behind the colour record.
 * colors may be NULL (no colour stage), orientations too (all 1).
 *
 * Built as that composition: the resize or warp launch writes planar bytes
 * into the region of the scratch the colour calls use, a colour stage runs on
 * that region in place, and the tone launch reads it and writes d_out in the
 * decoder's format with the decoder's constants.  Where a curve's mode is not
 * 0 the partial histograms (n x 16 x 3 KiB) and the composed curves (n x 768
 * bytes) lie in the same scratch and two more kernels run in front of the tone
 * kernel; they write all they read, so a reused scratch needs no clearing.  A
 * call whose curves are all mode 0 with the identity table is exactly the call
 * without tones: no region, no launch.  Everything that can refuse the call --
 * all that the call without tones refuses, a NULL tones, a mode outside 0..2
 * or a non-zero reserved (HJD_E_INVALID naming the frame) -- is checked before
 * anything is staged, allocated or enqueued. */
int hjd_gdec_decode_resized_tone(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                 const hjd_rect* rois, const int32_t* orientations, const int32_t* flags,
                                 const int32_t (*colors)[21], const hjd_tone_curve* tones, void* d_out, int out_w,
                                 int out_h, int32_t out_pitch, int filter, void* stream);
int hjd_gdec_decode_warped_tone(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                const int32_t (*m)[6], const int32_t* orientations, const int32_t* flags,
                                const uint32_t* fills, const int32_t (*colors)[21], const hjd_tone_curve* tones,
                                void* d_out, int out_w, int out_h, int32_t out_pitch, void* stream);
/* The calls that take every optional stage: a colour record, a filter
 * (include/hjd.h hjd_conv_filter: sharpness, Gaussian blur, unsharp masking)
 * and a tone curve per frame, each of colors, convs and tones NULL for none.
 * Image i of the batch is tone(conv(color(resize(orient(decode))))) or
 * tone(conv(color(warp(decode)))) -- jitter, blur, solarize: BYOL's order --
 * the filter's borders those of the out_w x out_h image the resize or warp
 * wrote (its fill included), a tone curve's histogram that of the filtered
 * image.
 *
 * Built as that composition: the resize or warp launch writes planar bytes
 * into the region of the scratch the colour and tone calls use, a colour stage
 * runs on that region in place, the filter launch reads it and writes d_out in
 * the decoder's format with the decoder's constants -- or, where a tone stage
 * follows, a second region of the same layout (a filter cannot run in place),
 * which the tone launch reads.  A call whose filters are all the identity
 * record (rx = ry = 0, a = 4096, b = 0) has no filter stage and no second
 * region: it is exactly hjd_gdec_decode_resized_tone / _warped_tone, and with
 * colors and tones NULL or the identity as well the call without stages.
 * Everything that can refuse the call -- all that the call without filters
 * refuses and all that hjd_conv_check refuses of a filter for an image of
 * out_w x out_h, HJD_CONV_REFLECT with a radius >= out_w or out_h included
 * (HJD_E_INVALID naming the frame) -- is checked before anything is staged,
 * allocated or enqueued. */
int hjd_gdec_decode_resized_aug(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                const hjd_rect* rois, const int32_t* orientations, const int32_t* flags,
                                const int32_t (*colors)[21], const hjd_conv_filter* convs, const hjd_tone_curve* tones,
                                void* d_out, int out_w, int out_h, int32_t out_pitch, int filter, void* stream);
int hjd_gdec_decode_warped_aug(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                               const int32_t (*m)[6], const int32_t* orientations, const int32_t* flags,
                               const uint32_t* fills, const int32_t (*colors)[21], const hjd_conv_filter* convs,
                               const hjd_tone_curve* tones, void* d_out, int out_w, int out_h, int32_t out_pitch,
                               void* stream);
/* Bytes of the most recent decode call: scan bytes the host CPU read + wrote
 * (0 when every scan was destuffed on the GPU) and bytes moved host -> device. */
int hjd_gdec_last_bytes(hjd_gdec* g, int64_t* host_scan_bytes, int64_t* h2d_bytes);

#define HJD_GDEC_SEQUENTIAL 1   /* verification needed the sequential path (round-based sync) or a
                                   serial chain repair (speculative sync: the decoder then moves its
                                   next calls to a longer lead-in) */
#define HJD_GDEC_CORRUPT 2      /* invalid Huffman data on the decoded chain */
#define HJD_GDEC_COUNT 4        /* fewer blocks than the frame needs */

/* ---- GPU-entropy stream: JPEG bytes in, BGRX in HBM out -----------------
 * Like hjd_stream, but the Huffman decode runs on the GPU: worker threads only
 * parse + destuff each JPEG into the pinned staging of the open batch (up to
 * max_frames JPEGs / max_scan_bytes / max_blocks per batch); nslots (2..16)
 * batches rotate on their own HIP streams so uploads overlap kernels. */
typedef struct hjd_gstream hjd_gstream;
int hjd_gstream_create(hjd_ctx* ctx, int max_frames, int64_t max_scan_bytes, int64_t max_blocks, int nslots,
                       int nthreads, hjd_gstream** out);
int hjd_gstream_destroy(hjd_gstream* s);
/* Queue one JPEG (bytes valid until hjd_gstream_sync returns); pixels go to
 * d_out (device, row pitch out_pitch bytes, 16-byte aligned).  submit and sync
 * may be called from several threads (they are serialised internally). */
int hjd_gstream_submit(hjd_gstream* s, const uint8_t* data, size_t size, void* d_out, int32_t out_pitch);
/* D2H sink (SURVEY.md s8(e) "D2H-on", s8(f) rank 4): same, but the pixels are
 * copied back into host memory h_out (row pitch out_pitch bytes; pinned memory
 * keeps the copy asynchronous) once the frame is decoded. */
int hjd_gstream_submit_host(hjd_gstream* s, const uint8_t* data, size_t size, void* h_out, int32_t out_pitch);
/* Flush and wait; returns the first error.  stats (may be NULL):
 * {images, pixels, host_prep_ns, h2d_bytes, batches}. */
int hjd_gstream_sync(hjd_gstream* s, int64_t stats[5]);
/* Pixel format of the stream's outputs (device and host sinks alike):
 * HJD_OUT_BGRX (default), HJD_OUT_BGR24, HJD_OUT_RGB24 or
 * HJD_OUT_RGB_PLANAR; with the 3-byte formats the D2H sink moves 3 bytes per
 * pixel (planar: 3 * height rows of width bytes, the planes out_pitch *
 * height apart in h_out).  Only between hjd_gstream_sync and the next submit
 * (HJD_E_STATE otherwise).  The float formats are not served by streams:
 * HJD_E_INVALID. */
int hjd_gstream_set_output_format(hjd_gstream* s, int out_format);
/* Scan bytes the host CPU has read + written so far (destuffing into pinned
 * staging: 2 per scan byte; a frame whose bytes are pinned host memory is
 * destuffed on the GPU and costs 0: only its header is parsed on the host). */
int hjd_gstream_host_bytes(hjd_gstream* s, int64_t* host_scan_bytes);

/* Pin (page-lock) a caller's host range so the GPU can DMA from it: JPEG bytes
 * in pinned memory (this, or hipHostMalloc) reach the device raw and are
 * destuffed there (HJD_DESTUFF=auto, the default; "host" / "device" force one
 * path).  The range must stay registered while frames submitted from it are in
 * flight (until hjd_gstream_sync / hjd_gdec_sync). */
int hjd_host_register(void* ptr, size_t size);
/* Host-side stream preparation alone, no GPU (measurement hook for the
 * multi-GPU host ceiling, one call = one per-GPU pool): nthreads threads on
 * NUMA node `node` (-1: unbound) prepare `frames` JPEGs read in order from an
 * arena of arena_bytes (datas replicated) into a staging ring of ring_bytes.
 * mode 0 host destuff, 1 header + tables only (the GPU-destuff path), 2 plain
 * memcpy of each file.  Calls sharing `barrier` (parties > 1) start their timed
 * phase together.  out: wall ns, summed thread CPU ns, JPEG bytes, frames. */
int hjd_debug_host_prep(const uint8_t* const* datas, const size_t* sizes, int n, int mode, int nthreads, int node,
                        int64_t frames, int64_t arena_bytes, int64_t ring_bytes, int32_t* barrier, int parties,
                        int64_t out[4]);
int hjd_host_unregister(void* ptr);

/* The 54-byte header of the reference's output BMP (src/decoder.cpp:372-394):
 * 32 bpp, top-down; the file is this header followed by the W*H*4 BGRX bytes. */
int hjd_bmp_header(int32_t width, int32_t height, uint8_t header[54]);
/* The 24-bpp counterpart (SURVEY.md s8(f) rank 4 "RGB24 writer"): top-down,
 * rows padded to 4 bytes; the file is this header followed by the rows of an
 * HJD_OUT_BGR24 image at pitch (3*W+3)&~3. */
int hjd_bmp_header_bgr24(int32_t width, int32_t height, uint8_t header[54]);

/* Test hook: the reader of the host decoder's single-scan files, process-wide.
 * 0 (default) the de-stuffed reader wherever the scan admits it, 1 the
 * byte-wise reader always (the cross-check); -1 queries.  Returns the previous
 * mode. */
int hjd_debug_host_reader(int mode);
/* Test hook (no GPU): runs the same parallel algorithm on the host, one frame,
 * and writes its coefficients.  Not a decode path. */
/* Destuff step alone (test hooks): the host routine, and the device kernels on
 * one raw scan of n bytes with nseg restart intervals expected (out: >= n+64
 * bytes; status: kStatusCorrupt bit 2 for malformed scans). */
int hjd_debug_destuff_host(const uint8_t* scan, size_t n, uint8_t* out, size_t cap, uint32_t* seg_end, int max_seg,
                           int* nseg, int64_t* out_bytes);
int hjd_debug_destuff_gpu(hjd_ctx* ctx, const uint8_t* scan, size_t n, int nseg, uint8_t* out, size_t cap,
                          uint32_t* seg_end, int64_t* out_bytes, uint32_t* status);
int hjd_debug_entropy_emulate(const uint8_t* data, size_t size, int sub_bits, int16_t* coefs, int64_t capacity_blocks,
                              int32_t* status);
/* Test hook (no GPU): the sync kernels' step decode (AC step tables, several
 * units per lookup) against the unit-by-unit decode, from guessed and true
 * entries of the first scan; *runs compared, *mismatches in exit state or
 * statistics. */
int hjd_debug_entropy_sync_check(const uint8_t* data, size_t size, int sub_bits, int64_t* runs, int64_t* mismatches);
/* Test hook (no GPU, nothing staged): the uploads a GPU decoder would issue for
 * a batch of n frames given as numbers, frames[i][8] = {destuff mode (0 host,
 * 1 raw from the caller's pinned memory, 2 raw from the staging), data_off,
 * data_bits, raw_len, raw_off, raw_src (the address), a further scan's data_off
 * and data_bits (< 0: none)}; data_base: where the data area starts in staging
 * and blob; hdr_used: the header's bytes; latency: a latency decoder, which
 * pulls a batch destuffed on the host throughout; prepulled: bytes of frame 0
 * an early pull moved.  rows[k][6] = {kind (0 header, 1 data run, 2 raw from
 * the staging, 3 raw span from the caller), destination offset (0, 1: in the
 * blob; 2, 3: in the raw area), source (staging offset; 3: the address), bytes,
 * first, last: the frames [first, last) it covers}, in issue order; segs[k][2]
 * = {offset, length} of the pull's segments in 16-byte words (room for 4);
 * totals = {bytes moved host to device, scan bytes the host CPU read + wrote},
 * as hjd_gdec_last_bytes reports them. */
int hjd_debug_upload_plan(const int64_t* frames, int n, int64_t data_base, int64_t hdr_used, int latency,
                          int64_t prepulled, int64_t* rows, int cap_rows, int* nrows, int64_t* segs, int* nsegs,
                          int* pull, int64_t totals[2]);

/* Test hook: the state a decoder carries from call to call (read-only; the
 * batch_* fields describe the most recent issued call, the lead_* fields the
 * lead-in ladder as hjd_gdec_sync last left it). */
typedef struct hjd_gdec_debug_state {
    uint32_t chain_epoch;        /* look-back tag of the last call that ran ent_chain_lb_kernel (0: none yet) */
    int32_t batch_spec;          /* the call took the speculative sync (0: the round-based one) */
    int32_t batch_lookback;      /* the call ran the look-back chain kernel (ent_chain_lb_kernel) */
    uint32_t batch_chain_chunks; /* chunks of its frame with the most subsequences (that kernel's grid width) */
    uint32_t batch_sub_bits;     /* its S: the dense tier's, or the decoder's own */
    uint32_t batch_lead_bits;    /* lead-in of its spec runs (0: round-based sync) */
    uint32_t lead_step;          /* ladder step of the next speculative call */
    uint32_t lead_left;          /* clean calls before the ladder steps down */
    uint32_t lead_hold;          /* the clean run a step down waits for */
    int32_t lead_stepped_down;   /* the last synced call ended a clean run: the next runs one step lower */
} hjd_gdec_debug_state;
int hjd_debug_gdec_state(hjd_gdec* g, hjd_gdec_debug_state* out);
/* Test hook: sets the host's look-back tag counter (0 .. 2^24 - 1), so a test
 * reaches the tag's wrap through the ordinary increment of the next calls.
 * Only the counter: the look-back words on the device keep their tags, and the
 * next call still advances the counter before it uses it.  HJD_E_STATE while a
 * call is pending (before hjd_gdec_sync). */
int hjd_debug_gdec_set_chain_epoch(hjd_gdec* g, uint32_t value);

#ifdef __cplusplus
}
#endif
#endif
