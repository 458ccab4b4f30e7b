// hjd_tone_curve.h -- the data curve of include/hjd.h's tone section, one
// function for the host (hjd_tone_curve_from_histogram, which the CPU suite
// calls) and the device (tone_lut_kernel, hjd_tone.hpp): the arithmetic the
// GPU runs is the arithmetic the CPU tests exercise.  No HIP call.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HJD_TONE_HD __host__ __device__
#else
#define HJD_TONE_HD
#endif

namespace hjd {

// D_c[v] of a channel (include/hjd.h): mode 0 the identity, 1 autocontrast, 2
// equalize.  below: the sum of h_c[k] over k < v; lo, hi: the smallest and
// largest non-empty bin (lo > hi: the histogram is empty); last = h_c[hi];
// n: the sum of all bins, at most 2^28.  Everything in uint32: 255 * (v - lo)
// < 2^16, step / 2 + below < 2^27 + 2^28.
HJD_TONE_HD inline uint32_t tone_data_curve(int mode, uint32_t v, uint32_t below, uint32_t lo, uint32_t hi, uint32_t last,
                                            uint32_t n)
{
    if (hi <= lo) return v;   // fewer than two non-empty bins: both modes are the identity
    if (mode == 1) {
        if (v <= lo) return 0;
        if (v >= hi) return 255;
        return 255u * (v - lo) / (hi - lo);
    }
    if (mode == 2) {
        const uint32_t step = (n - last) / 255u;
        if (step == 0) return v;
        const uint32_t q = (step / 2 + below) / step;
        return q < 255u ? q : 255u;
    }
    return v;
}

}  // namespace hjd
