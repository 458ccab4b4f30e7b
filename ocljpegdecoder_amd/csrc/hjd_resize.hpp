// hjd_resize.hpp -- the resize kernel for gfx950 (include/hjd.h hjd_resize_*;
// DESIGN.md s3.9): n planar uint8 RGB images, each of its own size, resampled
// (bilinear, half-pixel centres, 11-bit integer weights, one rounding) to one
// common out_w x out_h, flipped where asked, and written as planar uint8 or
// normalised half / float planes.
//
// Work decomposition: every image has the same output, so every image gets the
// same number of 256-thread groups (gridDim.x = n * groups) and the image of
// a group is blockIdx.x / groups -- group-uniform, its record read with scalar
// loads.  A lane produces quads: 4 horizontally adjacent output pixels of one
// row, all three channels; the quads of an image are dealt to its groups'
// threads round-robin, so consecutive lanes write consecutive 4-pixel pieces
// of a row.  The 48 taps of a quad are read straight from the source planes
// (byte loads, any pointer and pitch): the crops are small and were written by
// the kernel before this one, so they sit in L2.  No LDS, no barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjd_store.hpp"

namespace hjd {

constexpr int kResizeThreads = 256;
constexpr int kResizeFlipH = 1;        // hjd_resize_item.flags bit 0
constexpr int kResizeWeightBits = 11;

// Source sample position of output index j on one axis (size -> out_size):
// the first tap p0 and the weight f (0..2047) of the second tap min(p0 + 1,
// size - 1).  Every product stays below 2^31 for sizes up to 16384.
__device__ __forceinline__ void resize_tap(uint32_t j, uint32_t size, uint32_t out_size, uint32_t& p0, uint32_t& f)
{
    const int32_t s = static_cast<int32_t>((2 * j + 1) * size) - static_cast<int32_t>(out_size);
    const uint32_t n = static_cast<uint32_t>(s > 0 ? s : 0), den = 2 * out_size;
    p0 = n / den;
    f = ((n - p0 * den) << kResizeWeightBits) / den;
}

// The bilinear blend's second step: top and bot, the rows' blends with the 11-bit
// horizontal weight, blended with fy (0..2047), the weight of bot; 22 fraction
// bits, one rounding.  The warp kernel's, too.
__device__ __forceinline__ uint32_t resize_blend(uint32_t top, uint32_t bot, uint32_t fy)
{
    return (top * (2048u - fy) + bot * fy + (1u << 21)) >> 22;
}

template <int kFormat>
__global__ __launch_bounds__(kResizeThreads) void resize_kernel(const ResizeDev* __restrict__ items, int groups,
                                                                 int out_w, int out_h, int out_pitch, NormDev nk)
{
    constexpr int kElem = out_elem_bytes(kFormat);
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    const uint32_t img = blockIdx.x / static_cast<uint32_t>(groups);
    const uint32_t grp = blockIdx.x - img * static_cast<uint32_t>(groups);
    const ResizeDev it = items[img];   // group-uniform: scalar loads
    const uint32_t w = static_cast<uint32_t>(it.w), h = static_cast<uint32_t>(it.h);
    const uint32_t wo = static_cast<uint32_t>(out_w), ho = static_cast<uint32_t>(out_h);
    const int64_t splane = static_cast<int64_t>(it.pitch) * it.h;
    const int64_t dplane = static_cast<int64_t>(out_pitch) * out_h;
    const bool flip = (it.flags & kResizeFlipH) != 0;
    const bool vec = store_vec_ok<kFormat>(it.dst, out_pitch) && (wo & 3) == 0;   // whole quads, one vector per plane
    const uint32_t qw = (wo + 3) >> 2, quads = qw * ho;
    for (uint32_t q = grp * kResizeThreads + threadIdx.x; q < quads; q += static_cast<uint32_t>(groups) * kResizeThreads) {
        const uint32_t i = q / qw, j0 = 4 * (q - i * qw);
        uint32_t y0, fy;
        resize_tap(i, h, ho, y0, fy);
        const uint32_t y1 = min(y0 + 1, h - 1);
        // (global, not flat, addresses: the record's pointers are device memory)
        const gcbyte* r0 = (const gcbyte*)it.src + static_cast<int64_t>(y0) * it.pitch;
        const gcbyte* r1 = (const gcbyte*)it.src + static_cast<int64_t>(y1) * it.pitch;
        uint32_t px[4];   // 0x00RRGGBB, as the pixel kernels' BGRX words
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // (a column past out_w on the guarded path: clamped, computed, not stored)
            const uint32_t j = min(j0 + k, wo - 1);
            uint32_t x0, fx;
            resize_tap(flip ? wo - 1 - j : j, w, wo, x0, fx);
            const uint32_t x1 = min(x0 + 1, w - 1);
            uint32_t p = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const gcbyte* a = r0 + c * splane;
                const gcbyte* b = r1 + c * splane;
                const uint32_t top = a[x0] * (2048u - fx) + a[x1] * fx;
                const uint32_t bot = b[x0] * (2048u - fx) + b[x1] * fx;
                p = (p << 8) | resize_blend(top, bot, fy);
            }
            px[k] = p;
        }
        gbyte* d = (gbyte*)it.dst + static_cast<int64_t>(i) * out_pitch + static_cast<int64_t>(j0) * kElem;
        store_quad<kFormat>(px, d, dplane, vec, j0, wo, nk);
    }
}

}  // namespace hjd
