// hjd_internal.h -- helpers shared by the translation units of libhjd.so.
#pragma once
#include <stdint.h>

#include <atomic>
#include <vector>

#include "hjd.h"
#include "hjd_records.h"

struct hjd_jpeg_info;

namespace hjd_internal {

// Record the calling thread's last error (returned by hjd_last_error()) and
// return `code`.  Defined in hjd_runtime.hip.
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// JPEG zigzag: natural index of zigzag position k (src/zigzag.h:15-40).
constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                             12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                             58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Per-sampling geometry shared by the parser, the plans and the kernels.  A
// pixel-kernel task is always 48 coefficient blocks (hjd::kTaskBlocks).
struct SamplingGeom {
    int index;          // kernel template index: 0 4:4:4, 1 4:2:0, 2 4:2:2, 3 gray, 4 4:1:1, 5 4:4:0
    int mcu_px_w, mcu_px_h;
    int bpm;            // blocks per MCU
    int mcus_per_task;  // 48 / bpm
};
constexpr int kSamplingClasses = 6;   // values of SamplingGeom::index
inline bool sampling_geom(int sampling, SamplingGeom* g)
{
    switch (sampling) {
    case 0: *g = {0, 8, 8, 3, 16}; return true;    // HJD_YUV444
    case 1: *g = {1, 16, 16, 6, 8}; return true;   // HJD_YUV420
    case 3: *g = {2, 16, 8, 4, 12}; return true;   // HJD_YUV422
    case 4: *g = {3, 8, 8, 1, 48}; return true;    // HJD_GRAY
    case 5: *g = {4, 32, 8, 6, 8}; return true;    // HJD_YUV411_H4V1
    case 6: *g = {5, 8, 16, 4, 12}; return true;   // HJD_YUV440
    default: return false;
    }
}

// Device frame record of the fused kernel (layout of hjd::FrameDev).
struct FrameRecord {
    int64_t coef_base, out_base, task_begin;
    int32_t width, height, pitch, sampling, mcu_w, strips;
    int32_t qt[3];
    int32_t vec_ok;
};

// Second per-frame record of a ROI launch (layout of hjd::RoiDev): the table
// of them follows the frame records, at d_frames + nframes.
struct RoiRecord {
    int32_t row_stride, dx, dy, reserved;
};

// A ROI on a frame's output grid (the grid of `scale`), validated, in the
// terms the kernel needs.
struct RoiGeom {
    int mxf, myf;       // first MCU column / row the ROI touches
    int strips, rows;   // tasks per MCU row, MCU rows
    int dx, dy;         // the ROI's origin relative to MCU (mxf, myf)'s pixel (0,0)
    int mcu_w, rem_w;   // the frame's MCUs per row; those from mxf to the row end
    int bpm;
    int64_t tasks, blocks;   // blocks: the coefficient blocks the tasks read
};
// HJD_OK, or HJD_E_INVALID with the cause in the error string.
int roi_geom(int width, int height, int sampling, int scale, const ::hjd_rect* roi, RoiGeom* g);

// Fill a one-frame record (task_begin 0); returns the frame's task count, or
// a negative status for an unsupported geometry.  out_format: HJD_OUT_*;
// base_bits: low bits of the address out_base is relative to (out_vector_ok).
// scale (1, 2, 4, 8): width and height are the source's; the record holds the
// scaled size (scaled_dim) and `pitch` refers to it.
// roi (with `side`): the record is re-anchored at the ROI's first MCU, `side`
// gets its RoiRecord, out_base is where the ROI's first pixel lands and
// `pitch` refers to the ROI width.
int64_t make_frame_record(int width, int height, int sampling, int64_t coef_base, int64_t out_base, int pitch,
                          const int qt_index[3], FrameRecord* rec, int out_format = 0, uintptr_t base_bits = 0,
                          int scale = 1, const ::hjd_rect* roi = nullptr, RoiRecord* side = nullptr);

// Scaled decode (hjd_plan_create_scaled): log2 of a legal scale, or -1.
inline int scale_log2(int scale) { return scale == 1 ? 0 : scale == 2 ? 1 : scale == 4 ? 2 : scale == 8 ? 3 : -1; }
// Output size of a source dimension at a scale: ceil(d / scale).
inline int scaled_dim(int d, int scale) { return (d + scale - 1) / scale; }
// Samplings (enum hjd_sampling) the scaled kernels serve: 4:4:4, 4:2:0, gray.
inline bool scaled_sampling_ok(int sampling) { return sampling == 0 || sampling == 1 || sampling == 4; }

// What a launch of the fused pixel kernel decodes, apart from its buffers: the
// shape the legality rules (shape_check) and the kernel selection
//  are functions of.
struct DecodeShape {
    int sampling = HJD_YUV420;             // enum hjd_sampling
    int input_format = HJD_IN_Q16_ZIGZAG;
    int out_format = HJD_OUT_BGRX;
    int scale = 1;                         // 1, 2, 4 or 8
    bool roi = false;                      // the RoiRecord table follows d_frames[nframes - 1]
    int variant = 0;                       // kernel variant bits 0-1 (hjd_plan_set_variant)
    int stages = 0;                        // stage-skipping measurement variant (hjd_debug_plan_launch_stages), or 0
    int kernel_mode = HJD_KERNEL_AUTO;
    int64_t tasks = 0;
    int grid_blocks = 0;                   // workgroups of the persistent kernel; 0: the shape's default
};
// HJD_OK, or HJD_E_INVALID with the cause in the error string: the one
// statement of which shapes the kernels serve.  tasks and grid_blocks count
// only where variant bits meet a byte format other than BGRX: such a launch
// is legal if it takes the latency kernel, which ignores the bits.
int shape_check(const DecodeShape& s);

// One launch: the shape, the device and its buffers.  d_frames: nframes frame
// records, then (roi) their RoiRecord table, then (a float out_format) the
// NormRecord; d_qt_nat: natural-order tables.
struct DecodeLaunch : DecodeShape {
    int device = 0;
    const void* d_coefs = nullptr;
    const int32_t* d_qt_nat = nullptr;
    const FrameRecord* d_frames = nullptr;
    int nframes = 0;
    void* d_out = nullptr;
    void* stream = nullptr;
};
// Check the shape, select its kernel from the table and launch it (no host
// synchronisation, safe to call from any host thread).
int launch_decode(const DecodeLaunch& l);

// Properties of the output formats: one row per HJD_OUT_* value.
struct OutFormat {
    int bytes;         // per pixel overall (0: not a format)
    int row_bytes;     // per pixel within one output row: planar rows hold one component
    bool planar;       // three planes R, G, B at out_pitch * height (uint8 or float elements)
    int float_bytes;   // element bytes of a float planar format (else 0)
    int pitch_mask;    // a pitch and an offset must be clear of it
    int align_mask;    // an output pointer / offset must be clear of it
    int vector_mask;   // rows clear of it can take the kernel's full-width vector stores
};
constexpr OutFormat kNoOutFormat = {0, 0, false, 0, 3, 0, 3};
constexpr OutFormat kOutFormats[] = {
    {4, 4, false, 0, 3, 15, 15},   // HJD_OUT_BGRX: 4-byte pitches, 16-byte aligned rows
    {3, 3, false, 0, 3, 3, 3},     // HJD_OUT_BGR24: 4-byte pitches and rows
    {3, 3, false, 0, 0, 0, 3},     // HJD_OUT_RGB24: any pitch, offset and pointer
    {3, 1, true, 0, 0, 0, 3},      // HJD_OUT_RGB_PLANAR: any
    kNoOutFormat,                  // 4 is not a format
    {6, 2, true, 2, 1, 1, 7},      // HJD_OUT_RGB_PLANAR_F16: multiples of the element size
    {12, 4, true, 4, 3, 3, 15},    // HJD_OUT_RGB_PLANAR_F32
};
constexpr int kOutFormatRows = sizeof(kOutFormats) / sizeof(kOutFormats[0]);
static_assert(kOutFormatRows == HJD_OUT_RGB_PLANAR_F32 + 1 && HJD_OUT_RGB_PLANAR == 3 && HJD_OUT_RGB_PLANAR_F16 == 5,
              "one row per HJD_OUT_* value");
inline const OutFormat& out_format_row(int out_format)   // 7 and above (and below 0): unknown
{
    return out_format >= 0 && out_format < kOutFormatRows ? kOutFormats[out_format] : kNoOutFormat;
}

// Element bytes of a float planar format (else 0).
inline int out_format_float_bytes(int out_format) { return out_format_row(out_format).float_bytes; }
// Bytes per output pixel of an HJD_OUT_* format overall (0 if unknown).
inline int out_format_bytes(int out_format) { return out_format_row(out_format).bytes; }
inline bool out_format_planar(int out_format) { return out_format_row(out_format).planar; }
// Bytes per pixel within one output row.
inline int out_format_row_bytes(int out_format) { return out_format_row(out_format).row_bytes; }

// Rows of `out_pitch` bytes a frame of `height` pixel rows occupies (planar:
// the three planes follow each other at out_pitch * height).
inline int64_t out_format_rows(int out_format, int height)
{
    return out_format_planar(out_format) ? 3 * static_cast<int64_t>(height) : height;
}

// HJD_OUT_RGB24 / HJD_OUT_RGB_PLANAR: any pitch, offset and pointer are legal.
inline bool out_format_any_alignment(int out_format)
{
    return out_format_bytes(out_format) && !out_format_row(out_format).pitch_mask;
}
inline int out_format_pitch_mask(int out_format) { return out_format_row(out_format).pitch_mask; }
inline uintptr_t out_format_align_mask(int out_format) { return out_format_row(out_format).align_mask; }

// The largest out_pitch of the fused pixel kernel (HJD_MAX_OUT_PITCH, include/hjd.h).
// The kernel adds a 32-bit per-lane byte offset to a 64-bit wave-uniform row
// base (store4, hjd_kernels.hpp); the offset is rows * pitch + the lane's bytes
// within the strip row, with `rows` the row of the strip the base does not
// already hold.  Per branch of colour_stage / colour_stage_scaled, the most
// rows and the strip row's bytes at 4 bytes per pixel or element (BGRX, F32):
//     4:2:0, 4:4:4   2 (ylane; the row pair is in the base)       128 px   512
//     4:2:2          7 (y = u / 48, u <= 383)                     192 px   768
//     4:1:1          7 (y)                                        256 px  1024
//     4:4:0         15 (y0 = 2p <= 14, then lo + pitch)            96 px   384
//     gray           7 (y = u / 96, u <= 767)                     384 px  1536
//     scaled         7 (y < kMcuH >> kLog <= 8)               <= 192 px   768
// A ROI moves the 64-bit strip base only.  The offset stays below 2^32 when
// 15 * pitch + 1536 <= 2^32 - 1, that is pitch <= 286331050; the largest power
// of two is 2^28 (15 * 2^28 + 1536 = 4026533376 < 4294967296; 15 * 2^29 is
// not).  One bound for every sampling, scale and format.
constexpr int32_t kMaxOutPitch = HJD_MAX_OUT_PITCH;
static_assert(15ll * kMaxOutPitch + 1536 <= 0xffffffffll && 15ll * 2 * kMaxOutPitch + 1536 > 0xffffffffll &&
                  (kMaxOutPitch & (kMaxOutPitch - 1)) == 0,
              "the largest power of two whose 15 rows and one strip row fit a 32-bit lane offset");

// Rows of this format can take the kernel's full-width vector stores.
// out_base: the frame's offset; base_bits: low bits of the address out_base
// is relative to, where that address is not known to be 16-byte aligned.
inline bool out_vector_ok(int out_format, int64_t pitch, int64_t out_base, uintptr_t base_bits = 0)
{
    const int64_t bits = pitch | out_base | static_cast<int64_t>(base_bits & 15);
    return (bits & out_format_row(out_format).vector_mask) == 0;
}

// The records the host writes as the kernels read them (hjd_records.h): the
// float formats' constants, which follow the frame table (and a ROI plan's
// RoiRecord table), and one image of each stage kernel.
using NormRecord = hjd::NormDev;
using ResizeRecord = hjd::ResizeDev;   // (the layout of hjd_resize_item, too)
using OrientRecord = hjd::OrientDev;   // (of hjd_orient_item, whose reserved word is tile_begin here)
using WarpRecord = hjd::WarpDev;       // (of hjd_warp_item)
using ColorRecord = hjd::ColorDev;     // (of hjd_color_item, whose reserved word is use_sums here)
using ToneRecord = hjd::ToneDev;       // (of hjd_tone_item)
using ConvRecord = hjd::ConvDev;       // (of hjd_conv_item, whose filter's reserved word is tile_begin here)
// a = 1, b = 0: the C default (out = (float)u8).
inline NormRecord norm_identity() { return NormRecord{{1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}, {0.f, 0.f}}; }
// HJD_OK, or HJD_E_INVALID (NULL or non-finite constants) with the cause in the error string.
int norm_check(const float* a, const float* b);

// The one statement of a launch's frame table (DecodeLaunch::d_frames):
// nframes FrameRecords, then with a ROI their RoiRecords at `side`, then for a
// float format the NormRecord at `norm`; `bytes` in all.
struct FrameTable {
    size_t side, norm, bytes;
};
inline FrameTable frame_table(int nframes, bool roi, bool norm)
{
    FrameTable t;
    t.side = sizeof(FrameRecord) * static_cast<size_t>(nframes);
    t.norm = t.side + (roi ? sizeof(RoiRecord) * static_cast<size_t>(nframes) : 0);
    t.bytes = t.norm + (norm ? sizeof(NormRecord) : 0);
    return t;
}

// The resize kernel (hjd_resize.hip; include/hjd.h hjd_resize_*).
constexpr int kResizeMaxDim = 16384;      // source and output dimensions: 1..16384 (32-bit arithmetic)
constexpr int kResizeMaxItems = 1 << 20;  // images per launch
// HJD_OK, or HJD_E_INVALID with the cause in the error string: the output's
// side of hjd_resize_check (n, format, size, pitch), and one item's.
int resize_out_check(int n, int out_w, int out_h, int out_pitch, int out_format);
int resize_item_check(const ResizeRecord& it, int index, int out_format);
// One resize_kernel launch over n records in device memory (no host
// synchronisation); the arguments have passed the two checks.
int launch_resize(int device, const ResizeRecord* d_items, int n, int out_w, int out_h, int out_pitch, int out_format,
                  const NormRecord& norm, void* stream);

// The antialiased filter (HJD_RESIZE_TRIANGLE_AA; hjd_resize_aa.hpp): two
// launches through a uint8 intermediate, per item three planes of src_h rows at
// resize_aa_pitch(out_w), the item's resize_aa_item_bytes a multiple of 16.
inline int resize_aa_pitch(int out_w) { return (out_w + 3) & ~3; }
inline size_t resize_aa_item_bytes(int out_w, int src_h)
{
    return align_up(3 * static_cast<size_t>(resize_aa_pitch(out_w)) * static_cast<size_t>(src_h), 16);
}
// HJD_OK, or HJD_E_INVALID: `filter` is neither HJD_RESIZE_BILINEAR nor HJD_RESIZE_TRIANGLE_AA.
int resize_filter_check(int filter);
// The filter's one rule of its own, per axis: src^2 <= 2^21 * out (its 32-bit
// accumulator).  HJD_OK, or HJD_E_INVALID with a message naming the axis.
int resize_aa_ratio_check(int src_w, int src_h, int out_w, int out_h, int index);
// Both launches over n record pairs in device memory: d_h[i] = {the source,
// dst = item i's intermediate}, d_v[i] = {src = that intermediate, the output,
// w = out_w, h = src_h, pitch = resize_aa_pitch(out_w)}.  max_src_h: the
// largest src_h, which sizes the horizontal launch.  passes: bit 0 the
// horizontal launch, bit 1 the vertical one (hjd_debug_resize_launch_pass
// takes one).  No host synchronisation.
int launch_resize_aa(int device, const ResizeRecord* d_h, const ResizeRecord* d_v, int n, int max_src_h, int out_w,
                     int out_h, int out_pitch, int out_format, const NormRecord& norm, void* stream, int passes = 3);

// The orientation kernel (hjd_orient.hip; include/hjd.h hjd_orient_*).
constexpr int64_t kOrientMaxTiles = INT32_MAX;   // tiles per launch (the grid)
inline bool orientation_ok(int o) { return o >= 1 && o <= 8; }
inline bool orientation_transposes(int o) { return o >= 5; }
// Tiles (workgroups) of one w x h image: 128 x 128 bytes of one plane each.
inline int64_t orient_tiles(int w, int h) { return 3 * static_cast<int64_t>((w + 127) / 128) * ((h + 127) / 128); }
// HJD_OK, or HJD_E_INVALID with the cause in the error string: n and the
// format, and one item's side of hjd_orient_check (tile_begin is not looked at).
int orient_out_check(int n, int out_format);
int orient_item_check(const OrientRecord& it, int index, int out_format);
// The stored rectangle of a display rectangle (hjd_orient_roi without the NULL checks).
int orient_roi(int width, int height, int orientation, const ::hjd_rect& display, ::hjd_rect* stored);
// One orient_kernel launch over n records in device memory, `tiles` their
// tile total (no host synchronisation); the records have passed the checks
// and carry their tile_begin prefix.
int launch_orient(int device, const OrientRecord* d_items, int n, int64_t tiles, int out_format, const NormRecord& norm,
                  void* stream);

// The affine warp kernel (hjd_warp.hip; include/hjd.h hjd_warp_*).
// HJD_OK, or HJD_E_INVALID with the cause in the error string: one item's side
// of hjd_warp_check (the output's side is resize_out_check).
int warp_item_check(const WarpRecord& it, int index, int out_format);
// hjd_warp_roi and hjd_warp_orient without the NULL checks.
int warp_roi(int width, int height, const int32_t m[6], int out_w, int out_h, ::hjd_rect* out);
int warp_orient(const int32_t m[6], int stored_w, int stored_h, int orientation, int32_t out[6]);
// One warp_kernel launch over n records in device memory (no host
// synchronisation); the arguments have passed the two checks.  tiled: 1 a
// wave takes 8 quads x 8 rows, 0 it takes 64 consecutive quads; -1 the
// library's choice (hjd::kWarpTiled).
int launch_warp(int device, const WarpRecord* d_items, int n, int out_w, int out_h, int out_pitch, int out_format,
                const NormRecord& norm, void* stream, int tiled = -1);

// The colour kernels (hjd_color.hip; include/hjd.h hjd_color_*).
// HJD_OK, or HJD_E_INVALID with the cause in the error string: n and the
// format; the words m[9], p[9], t[3] of one record (*uses_sums, if asked: some
// p is not 0); and one item's side of hjd_color_check (use_sums is not looked at).
// A caller's flat record c[21] is (c, c + 9, c + 18).
int color_out_check(int n, int out_format);
int color_coef_check(const int32_t m[9], const int32_t p[9], const int32_t t[3], int index, bool* uses_sums);
int color_item_check(const ColorRecord& it, int index, int out_format);
// Groups of one w x h image (a launch takes the largest of its images'), and
// the bytes of the table of partial sums of n images: [n][kMaxGroups][3] uint32.
int color_groups(int w, int h);
constexpr size_t color_sums_bytes(int n) { return static_cast<size_t>(n) * 256 * 3 * sizeof(uint32_t); }
// color_sum_kernel (d_sums not null: some record's use_sums is set) and
// color_kernel over n records in device memory (no host synchronisation); the
// records have passed the checks and carry use_sums.
int launch_color(int device, const ColorRecord* d_items, int n, int groups, uint32_t* d_sums, int out_format,
                 const NormRecord& norm, void* stream);

// The tone kernels (hjd_tone.hip; include/hjd.h hjd_tone_*).
// HJD_OK, or HJD_E_INVALID with the cause in the error string: n and the
// format; the mode and the reserved word of one curve; and one item's side of
// hjd_tone_check (the table is not looked at: every table is legal).
int tone_out_check(int n, int out_format);
int tone_curve_check(int32_t mode, int32_t reserved, int index);
int tone_item_check(const ToneRecord& it, int index, int out_format);
// The bytes of the table of partial histograms of n images, [n][16][3][256]
// uint32, and of their composed curves, [n][3][256] bytes.
constexpr size_t tone_hist_bytes(int n) { return static_cast<size_t>(n) * 16 * 768 * sizeof(uint32_t); }
constexpr size_t tone_luts_bytes(int n) { return static_cast<size_t>(n) * 768; }
// tone_hist_kernel and tone_lut_kernel (d_hist and d_luts not null: some
// record's mode is not 0) and tone_kernel over n records in device memory (no
// host synchronisation); `groups` as color_groups gives them, the largest
// image's; the records have passed the checks.
int launch_tone(int device, const ToneRecord* d_items, int n, int groups, uint32_t* d_hist, uint8_t* d_luts,
                int out_format, const NormRecord& norm, void* stream);

// The filter kernel (hjd_conv.hip; include/hjd.h hjd_conv_*).
constexpr int64_t kConvMaxTiles = INT32_MAX;   // tiles per launch (the grid)
// Tiles (workgroups) of one w x h image: 64 x 32 pixels of the three planes each.
inline int64_t conv_tiles(int w, int h) { return static_cast<int64_t>((w + 63) / 64) * ((h + 31) / 32); }
// HJD_OK, or HJD_E_INVALID with the cause in the error string: n and the
// format; the filter of one record for an image of w x h (its radii, border,
// taps and gains; `reserved` is the caller's word, looked at by hjd_conv_check
// alone); and one item's side of hjd_conv_check (tile_begin is not looked at).
int conv_out_check(int n, int out_format);
int conv_filter_check(const ConvRecord& it, int index);
int conv_item_check(const ConvRecord& it, int index, int out_format);
// The identity record (include/hjd.h): it copies byte for byte.
inline bool conv_is_identity(const ConvRecord& it) { return it.rx == 0 && it.ry == 0 && it.a == 4096 && it.b == 0; }
// One conv_kernel launch over n records in device memory, `tiles` their tile
// total (no host synchronisation); the records have passed the checks and
// carry their tile_begin prefix.
int launch_conv(int device, const ConvRecord* d_items, int n, int64_t tiles, int out_format, const NormRecord& norm,
                void* stream);

// Parsed header of one sequential scan as the GPU entropy path needs it
// (jpeg_host.cpp).  File-level fields (width .. nblocks, out_bpm, qt) describe
// the whole image; the rest the scan.
struct ScanHeader {
    int width, height, sampling, restart_interval, mcu_w, mcu_h;
    int bpm;                     // blocks per MCU of this scan (1 for a non-interleaved scan)
    int out_bpm;                 // blocks per MCU of the image (the coefficient layout)
    int64_t nblocks;             // blocks of the image (mcu_w * mcu_h * out_bpm)
    int64_t scan_blocks;         // blocks this scan codes
    size_t scan_offset;          // first byte of entropy-coded data
    int32_t qt[3][64];           // per frame component, zigzag (file) order
    int jcomp[6], jdc[6], jac[6], jslot[6];   // per bitstream block of an MCU
    bool table_defined[2][4];    // [class: 0 DC, 1 AC][id]
    uint8_t counts[2][4][16];
    uint8_t symbols[2][4][256];
    int nsym[2][4];
    // Sequential files with several scans (T.81 B.2.3; an extension, the
    // reference takes one interleaved scan): `extra_scans` > 0 on the first
    // scan's header says how many more scans the frame can hold (<= 2, one per
    // component not in the first scan); parse_scan_headers() lists them.
    int extra_scans;
    int layout;                  // 0: MCU-interleaved; 1: one component in raster block order (A.2.2)
    int comp_bw, comp_bh;        // layout 1: the component's block grid
    int comp_lh, comp_lv;        // layout 1: log2 of its sampling factors
};
int parse_scan_header(const uint8_t* data, size_t size, ScanHeader* h);
// Every scan of a sequential file (hs[0] == what parse_scan_header gives).
// Progressive files fail.
int parse_scan_headers(const uint8_t* data, size_t size, std::vector<ScanHeader>* hs);

// Host Huffman decode of two files on the calling thread (jpeg_host.cpp): as
// two hjd_jpeg_decode_coefs calls, with the symbol steps of the two files
// interleaved when both are single-scan sequential files.  rc[i] per file.
int jpeg_decode_coefs_two(const uint8_t* const data[2], const size_t size[2], ::hjd_jpeg_info* const info[2],
                          int16_t* const coefs[2], const int64_t capacity[2], int rc[2]);

// hjd_ctx accessors for the other translation units
int ctx_num_cu(const struct ::hjd_ctx* ctx);

// d16 gather (hjd_probe.hip): d16_probe() is 1 if ds_read_u16_d16_hi zeroes
// the low half of its destination on `device` (one-wave probe; a completed run
// is cached per device, a failed one returns 0 and is retried next time;
// HJD_D16_PROBE=fail forces 0).  hjd_ctx_create runs it.  d16_probe_cached()
// never runs it: the cached answer, or -1.  d16_gather_selected(): whether
// the 4:4:4 launches take the kVarD16 kernels (the cached probe passed and
// HJD_D16 is not 0); a launch never runs the probe itself, so it stays legal
// inside stream capture.
int d16_probe(int device);
int d16_probe_cached(int device);
bool d16_gather_selected(int device);

// The HJD_* overrides, one field each (the list, with what each one does, is
// the table in hjd_runtime.hip).  tuning() parses the environment at its
// first call and never looks at it again; after that only
// hjd_debug_set_tuning() changes a field.  Every field is one relaxed atomic,
// so any thread may read it at any time.
constexpr int64_t kTuneUnset = INT64_MIN;   // an integer override nobody set: the call site's own choice applies
struct TuneField {
    std::atomic<int64_t> v{0};
    int64_t get() const { return v.load(std::memory_order_relaxed); }
    bool is_set() const { return get() != kTuneUnset; }
};
enum { kPolicyHost = 0, kPolicyAuto = 1, kPolicyDevice = 2 };      // HJD_DESTUFF
enum { kProbeRun = 0, kProbeFail = 1, kProbeHipFail = 2 };         // HJD_D16_PROBE
struct Tuning {
    TuneField destuff, spec_lead, dense_sub_bits, d16, autotune_cache, sub_bits, sync_spec, emu_rounds, sync_phases,
        sync_offsets, gdec_host_times, numa, stream_pair, lat_tasks, tasks_per_wave, d16_probe, compat_copy,
        compat_stats, compat_teardown;
};
const Tuning& tuning();

}  // namespace hjd_internal

namespace hjd_internal {

// NUMA locality of a device's host-side workers: the CPUs
// of the NUMA node the GPU's PCIe device hangs off (sysfs), or an empty set
// when unknown.  bind_current_thread() applies such a set (no-op if empty)
// and returns the previous mask so a caller can restore it.
struct CpuSet {
    std::vector<int> cpus;
};
CpuSet device_local_cpus(int device);
// Default host worker count of a stream on `device` (nthreads = 0): the
// process's CPU share (hjd_host_cpu_share) capped by the device's CPU slice
// (device_local_cpus; uncapped when the topology is unknown).
int default_worker_threads(int device);
CpuSet node_cpus(int node);   // CPUs of NUMA node `node` this process may use (empty: unknown)
std::vector<int> bind_current_thread(const CpuSet& s);
void restore_current_thread(const std::vector<int>& prev);

}  // namespace hjd_internal

#ifndef __HIP_DEVICE_COMPILE__   // host code only (the device pass parses, never emits, its callers)
#include <immintrin.h>
#endif

namespace hjd_internal {

// The scan-copy step of both host destuff routines (jpeg_host.cpp
// destuff_scan, hjd_entropy_prep.cpp destuff): copy the bytes of [s, end) before
// the first 0xFF to o (advanced) and return where that 0xFF is (or end).
// AVX2 compares, 64 bytes per test while none is an 0xFF, instead of a memchr
// + memcpy call pair per run: entropy-coded data has an 0xFF every ~200 bytes,
// so the calls' overhead dominated.  Vector steps store whole vectors (bytes
// past the 0xFF are overwritten later) only while they fit before oend; the
// rest is copied bytewise.  Returns a position that is not an 0xFF and not
// end only when the output is full (o == oend).
#ifndef __HIP_DEVICE_COMPILE__
__attribute__((target("avx2"))) inline const uint8_t* copy_until_ff_avx2(const uint8_t* s, const uint8_t* end,
                                                                          uint8_t*& o, uint8_t* oend)
{
    const __m256i ff = _mm256_set1_epi8(static_cast<char>(0xFF));
    while (end - s >= 64 && oend - o >= 64) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + 32));
        const uint32_t ma = static_cast<uint32_t>(_mm256_movemask_epi8(_mm256_cmpeq_epi8(a, ff)));
        const uint32_t mb = static_cast<uint32_t>(_mm256_movemask_epi8(_mm256_cmpeq_epi8(b, ff)));
        _mm256_storeu_si256(reinterpret_cast<__m256i*>(o), a);
        _mm256_storeu_si256(reinterpret_cast<__m256i*>(o + 32), b);
        if (ma | mb) {
            const uint64_t m = (static_cast<uint64_t>(mb) << 32) | ma;
            const int k = __builtin_ctzll(m);
            o += k;
            return s + k;
        }
        s += 64;
        o += 64;
    }
    return s;
}
#endif

inline const uint8_t* copy_until_ff(const uint8_t* s, const uint8_t* end, uint8_t*& o, uint8_t* oend)
{
#ifndef __HIP_DEVICE_COMPILE__
    static const bool avx2 = [] {
        __builtin_cpu_init();
        return __builtin_cpu_supports("avx2") != 0;
    }();
    if (avx2) {
        s = copy_until_ff_avx2(s, end, o, oend);
        if (s < end && *s == 0xFF) return s;
    }
#endif
    while (s < end && *s != 0xFF && o < oend) *o++ = *s++;
    return s;
}

}  // namespace hjd_internal
