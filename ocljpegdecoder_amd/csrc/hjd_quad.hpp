// hjd_quad.hpp -- the input side the colour and tone kernels share (hjd_color.hpp,
// hjd_tone.hpp): a lane's quad, four horizontally adjacent bytes of one plane's row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hjd {

// The four bytes of columns j0 .. j0 + 3 of the row at `row` (lowest first;
// 0 past column w): one dword where vec, else guarded byte loads.
__device__ __forceinline__ uint32_t load_quad(__attribute__((address_space(1))) const uint8_t* row, uint32_t j0, uint32_t w,
                                              bool vec)
{
    typedef __attribute__((address_space(1))) const uint32_t gcword;
    if (vec && j0 + 4 <= w) return *(gcword*)(row + j0);
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
        if (j0 + b < w) v |= static_cast<uint32_t>(row[j0 + b]) << (8 * b);
    return v;
}

}  // namespace hjd
