// hjd_records.h -- the records the stage kernels and the float formats read, one
// declaration each for the host that writes them (hjd_internal.h) and the
// kernels (hjd_norm.hpp, hjd_resize.hpp, hjd_orient.hpp, hjd_warp.hpp, hjd_color.hpp,
// hjd_tone.hpp, hjd_conv.hpp).  No HIP.
#pragma once
#include <stdint.h>

namespace hjd {

// The plan-level constants of the float formats, per channel R, G, B: the
// 32-byte record that follows the frame table (and the RoiDev table of a ROI
// plan), and a launch argument of the stage kernels.  Only the float
// instantiations read it.
struct NormDev {
    float a[3], b[3];
    float reserved[2];   // 0
};
static_assert(sizeof(NormDev) == 32, "NormDev layout");

// One image of the resize kernels: the layout of hjd_resize_item.
struct ResizeDev {
    const void* src;   // plane R of the planar uint8 source; G and B follow at pitch * h
    void* dst;         // plane R of the output; G and B follow at out_pitch * out_h
    int32_t w, h, pitch, flags;
};
static_assert(sizeof(ResizeDev) == 32, "ResizeDev layout");

// One image of the orientation kernel: the layout of hjd_orient_item, whose
// reserved word the host fills with the image's first tile.
struct OrientDev {
    const void* src;   // plane R; G and B follow at pitch * h
    void* dst;         // plane R of the oriented image; G and B follow at dst_pitch * (its rows)
    int32_t w, h, pitch, orientation, dst_pitch;
    uint32_t tile_begin;
};
static_assert(sizeof(OrientDev) == 40, "OrientDev layout");

// One image of the warp kernel: the layout of hjd_warp_item.
struct WarpDev {
    const void* src;   // plane R; G and B follow at pitch * h
    void* dst;         // plane R of the output; G and B follow at out_pitch * out_h
    int32_t w, h, pitch, flags;
    int32_t m[6];      // X = m0 j + m1 i + m2, Y = m3 j + m4 i + m5 (Q16 source pixel indices)
    uint32_t fill;     // 0x00RRGGBB
    int32_t reserved;
};
static_assert(sizeof(WarpDev) == 64, "WarpDev layout");

// One image of the colour kernels: the layout of hjd_color_item, whose
// reserved word the host fills with whether the record reads the image's sums.
struct ColorDev {
    const void* src;   // plane R; G and B follow at pitch * h
    void* dst;         // plane R of the output; G and B follow at dst_pitch * h
    int32_t w, h, pitch, dst_pitch;
    int32_t m[9], p[9], t[3];   // Q12: u8 = clamp((m x + T + 2048) >> 12), T = t + ((p mq + 128) >> 8)
    int32_t use_sums;           // some p is not 0: color_sum_kernel ran before color_kernel
};
static_assert(sizeof(ColorDev) == 120, "ColorDev layout");

// One image of the tone kernels: the layout of hjd_tone_item.
struct ToneDev {
    const void* src;   // plane R; G and B follow at pitch * h
    void* dst;         // plane R of the output; G and B follow at dst_pitch * h
    int32_t w, h, pitch, dst_pitch;
    int32_t mode;      // 0 the table alone, 1 autocontrast, 2 equalize in front of it
    int32_t reserved;  // 0
    uint8_t lut[3][256];   // u8_c = lut[c][D_c[x_c]]
};
static_assert(sizeof(ToneDev) == 808, "ToneDev layout");

// One image of the filter kernel: the layout of hjd_conv_item, whose filter's
// reserved word the host fills with the image's first tile.
struct ConvDev {
    const void* src;   // plane R; G and B follow at pitch * h
    void* dst;         // plane R of the output; G and B follow at dst_pitch * h
    int32_t w, h, pitch, dst_pitch;
    int32_t rx, ry;    // 0..11: 2 r + 1 taps per axis
    int32_t border;    // 0 keep, 1 reflect, 2 replicate
    int32_t a, b;      // Q12: u8 = clamp((a (x << 24) + b S + 2^35) >> 36)
    uint32_t tile_begin;
    uint16_t kh[24], kv[24];   // Q12 taps, 0 beyond 2 r
};
static_assert(sizeof(ConvDev) == 152, "ConvDev layout");

}  // namespace hjd
