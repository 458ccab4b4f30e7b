// hjd_conv_math.h -- the arithmetic of include/hjd.h's filter section
// (hjd_conv_filter), two functions for the host (hjd_conv_apply_host, which the
// CPU suite calls) and the device (conv_kernel, hjd_conv.hpp): the arithmetic
// the GPU runs is the arithmetic the CPU tests exercise.  No HIP call.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HJD_CONV_HD __host__ __device__
#else
#define HJD_CONV_HD
#endif

namespace hjd {

// The source index X reads for position i of an axis of n pixels (n >= 1), i
// anywhere: REFLECT (border 1) mirrors about the first and the last pixel
// (-k -> k, n - 1 + k -> n - 1 - k; one reflection: the check demands radius
// < n), every border then clamps to 0..n - 1.  REPLICATE is that clamp; KEEP
// never uses a position outside the image, and a position further out than
// one reflection reaches belongs to a pixel nobody stores: the clamp only
// keeps their reads inside the image.
HJD_CONV_HD inline int32_t conv_src_index(int32_t i, int32_t n, int32_t border)
{
    if (border == 1) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
    }
    return i < 0 ? 0 : i >= n ? n - 1 : i;
}

// u8 = clamp((a (x << 24) + b S + 2^35) >> 36, 0, 255): a, b Q12 with |a|, |b|
// <= 2^20, x the centre byte, S <= 255 * 2^24 the sum of the window in Q24
// (uint32, above int32).  Both products stay below 2^52 in magnitude, T below
// 2^53; the shift is arithmetic (a floor), the one rounding of the stage.
HJD_CONV_HD inline uint32_t conv_finish(int32_t a, int32_t b, uint32_t x, uint32_t S)
{
    const int64_t T =
        static_cast<int64_t>(a) * (static_cast<int64_t>(x) << 24) + static_cast<int64_t>(b) * static_cast<int64_t>(S);
    const int64_t u = (T + (static_cast<int64_t>(1) << 35)) >> 36;
    return u < 0 ? 0u : u > 255 ? 255u : static_cast<uint32_t>(u);
}

}  // namespace hjd
