// hjd_warp.hpp -- the affine warp kernel for gfx950 (include/hjd.h hjd_warp_*;
// DESIGN.md s3.12): n planar uint8 RGB images, each of its own size, sampled
// through each image's own inverse map (six Q16 integers: rotation, shear,
// zoom, flips, translation) to one common out_w x out_h, bilinear with the
// resize's 11-bit weights and one rounding, and written as planar uint8 or
// normalised half / float planes.  A tap outside the image is the item's fill
// colour, or (HJD_WARP_REPLICATE) the nearest pixel of the image.
//
// Work decomposition: as the resize's (hjd_resize.hpp) -- gridDim.x = n *
// groups, the image of a group is blockIdx.x / groups, group-uniform, its
// 64-byte record read with scalar loads; a lane produces quads of 4
// horizontally adjacent output pixels, all three channels; byte loads straight
// from the planes (the crops were written by the kernel before and sit in
// L2); no LDS, no barrier; store_quad (hjd_store.hpp) writes the quad.  What
// differs is how the quads are dealt.  Once the map rotates, the 256 output
// pixels of a wave that takes 64 consecutive quads of a row lie on one slanted
// line through the source, 256 source pixels long.  Tiled (kTiled), a wave takes 8
// quads x 8 rows -- 32 x 8 output pixels -- whose taps lie within a few dozen
// source rows and columns; a group's four waves take four consecutive tiles of
// a tile row.  DESIGN.md s3.12 has both forms' times.
//
// X and Y of a quad's first pixel are formed once in 64 bits (m * index stays
// below 2^46) and stepped by m[0], m[3]; X >> 16 then fits 32 bits.  Every
// load goes to the tap's coordinates clamped into the image, so no address
// outside the image is ever formed; without HJD_WARP_REPLICATE a tap whose
// coordinates were clamped is replaced by the fill byte after the load.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjd_resize.hpp"   // resize_blend
#include "hjd_store.hpp"

namespace hjd {

constexpr int kWarpThreads = 256;
constexpr int kWarpReplicate = 1;      // hjd_warp_item.flags bit 0
constexpr int kWarpTileQuads = 8;      // a wave's tile: 8 quads (32 pixels) x 8 rows
constexpr int kWarpTileRows = 8;
constexpr bool kWarpTiled = true;      // the form hjd_warp_launch takes

template <int kFormat, bool kTiled>
__device__ __forceinline__ void warp_image(const WarpDev* __restrict__ items, int groups, int out_w, int out_h,
                                           int out_pitch, const NormDev& nk)
{
    constexpr int kElem = out_elem_bytes(kFormat);
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    const uint32_t img = blockIdx.x / static_cast<uint32_t>(groups);
    const uint32_t grp = blockIdx.x - img * static_cast<uint32_t>(groups);
    const WarpDev it = items[img];   // group-uniform: scalar loads
    const int32_t wmax = it.w - 1, hmax = it.h - 1;
    const uint32_t wo = static_cast<uint32_t>(out_w), ho = static_cast<uint32_t>(out_h);
    const int64_t splane = static_cast<int64_t>(it.pitch) * it.h;
    const int64_t dplane = static_cast<int64_t>(out_pitch) * out_h;
    const bool replicate = (it.flags & kWarpReplicate) != 0;
    const bool vec = store_vec_ok<kFormat>(it.dst, out_pitch) && (wo & 3) == 0;   // whole quads, one vector per plane
    const uint32_t qw = (wo + 3) >> 2;
    // the units dealt round-robin: quads, or a thread's place in a wave's tile
    const uint32_t tiles_x = (qw + kWarpTileQuads - 1) / kWarpTileQuads;
    const uint32_t tiles_y = (ho + kWarpTileRows - 1) / kWarpTileRows;
    const uint32_t units = kTiled ? tiles_x * tiles_y * 64u : qw * ho;
    for (uint32_t u = grp * kWarpThreads + threadIdx.x; u < units; u += static_cast<uint32_t>(groups) * kWarpThreads) {
        uint32_t i, q;   // the quad: row i, quad column q
        if constexpr (kTiled) {
            const uint32_t tile = u >> 6, lane = u & 63u;
            const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
            i = ty * kWarpTileRows + (lane >> 3);
            q = tx * kWarpTileQuads + (lane & 7u);
            if (i >= ho || q >= qw) continue;
        } else {
            i = u / qw;
            q = u - i * qw;
        }
        const uint32_t j0 = 4 * q;
        int64_t X = static_cast<int64_t>(it.m[0]) * j0 + static_cast<int64_t>(it.m[1]) * i + it.m[2];
        int64_t Y = static_cast<int64_t>(it.m[3]) * j0 + static_cast<int64_t>(it.m[4]) * i + it.m[5];
        uint32_t px[4];   // 0x00RRGGBB, as the pixel kernels' BGRX words
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // (a column past out_w on the guarded path: computed, not stored)
            const int32_t x0 = static_cast<int32_t>(X >> 16), y0 = static_cast<int32_t>(Y >> 16);
            const uint32_t fx = (static_cast<uint32_t>(X) & 0xffffu) >> 5, fy = (static_cast<uint32_t>(Y) & 0xffffu) >> 5;
            const int32_t cx0 = min(max(x0, 0), wmax), cx1 = min(max(x0 + 1, 0), wmax);
            const int32_t cy0 = min(max(y0, 0), hmax), cy1 = min(max(y0 + 1, 0), hmax);
            // inside the image: the tap's own coordinates survived the clamp
            const bool ix0 = replicate || cx0 == x0, ix1 = replicate || cx1 == x0 + 1;
            const bool iy0 = replicate || cy0 == y0, iy1 = replicate || cy1 == y0 + 1;
            // (global, not flat, addresses: the record's pointers are device memory)
            const gcbyte* r0 = (const gcbyte*)it.src + static_cast<int64_t>(cy0) * it.pitch;
            const gcbyte* r1 = (const gcbyte*)it.src + static_cast<int64_t>(cy1) * it.pitch;
            uint32_t p = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const gcbyte* a = r0 + c * splane;
                const gcbyte* b = r1 + c * splane;
                const uint32_t fb = (it.fill >> (16 - 8 * c)) & 0xffu;
                const uint32_t A = ix0 && iy0 ? a[cx0] : fb, B = ix1 && iy0 ? a[cx1] : fb;
                const uint32_t C = ix0 && iy1 ? b[cx0] : fb, D = ix1 && iy1 ? b[cx1] : fb;
                const uint32_t top = A * (2048u - fx) + B * fx;
                const uint32_t bot = C * (2048u - fx) + D * fx;
                p = (p << 8) | resize_blend(top, bot, fy);
            }
            px[k] = p;
            X += it.m[0];
            Y += it.m[3];
        }
        gbyte* d = (gbyte*)it.dst + static_cast<int64_t>(i) * out_pitch + static_cast<int64_t>(j0) * kElem;
        store_quad<kFormat>(px, d, dplane, vec, j0, wo, nk);
    }
}

template <int kFormat>
__global__ __launch_bounds__(kWarpThreads) void warp_kernel(const WarpDev* __restrict__ items, int groups, int out_w,
                                                             int out_h, int out_pitch, NormDev nk)
{
    warp_image<kFormat, kWarpTiled>(items, groups, out_w, out_h, out_pitch, nk);
}

// Timing only (hjd_debug_warp_launch_form): the form hjd_warp_launch does not take.
template <int kFormat>
__global__ __launch_bounds__(kWarpThreads) void warp_other_form_kernel(const WarpDev* __restrict__ items, int groups,
                                                                        int out_w, int out_h, int out_pitch, NormDev nk)
{
    warp_image<kFormat, !kWarpTiled>(items, groups, out_w, out_h, out_pitch, nk);
}

}  // namespace hjd
