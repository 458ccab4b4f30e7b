// hjd_resize_aa.hpp -- the antialiased resize for gfx950 (include/hjd.h,
// HJD_RESIZE_TRIANGLE_AA): the exact triangle filter, separable,
// as two kernels through a uint8 intermediate in device memory.
//
//   resize_aa_h_kernel      source planes (any pointer and pitch) -> intermediate:
//                           per item three planes of src_h rows x out_w bytes, the
//                           pitch out_w rounded up to 4, the item 16-byte aligned
//   resize_aa_v_kernel<F>   intermediate -> the output planes, with the bilinear
//                           kernel's store forms (store_quad, hjd_store.hpp)
//
// Both keep resize_kernel's decomposition: every image gets the same number of
// 256-thread groups, blockIdx.x / groups is the group-uniform image (its 32-byte
// record read with scalar loads), a lane produces quads of 4 adjacent columns
// of one row, all three channels, and loops when an image has more quads than
// its groups have threads.  The horizontal kernel's records hold the source
// and, as dst, the item's intermediate; the vertical kernel's hold the
// intermediate as src (w = out_w, h = src_h, pitch = the intermediate's) and the
// output as dst.  A quad of the intermediate is one aligned dword per row and
// plane, on both sides.  The weights are computed in the tap loop; no tables,
// no LDS, no barrier.
#pragma once
#include "hjd_resize.hpp"   // kResizeThreads, kResizeFlipH
#include "hjd_store.hpp"

namespace hjd {

// The first tap k0 of output index j on one axis (size -> out_size) and its
// d = (2 k0 + 1) out_size - (2j + 1) size; s2 = 2 max(size, out_size).  Tap k
// weighs t = s2 - |d|, d advances by 2 out_size per tap, and the taps are
// the k < size with d < s2 (d > -s2 holds from k0 on).  Every value stays
// below 2^31 for sizes up to 16384.
__device__ __forceinline__ void resize_aa_first(uint32_t j, uint32_t size, uint32_t out_size, uint32_t s2, uint32_t& k0,
                                                int32_t& d)
{
    const int32_t c = static_cast<int32_t>((2 * j + 1) * size);
    const int32_t m = c - static_cast<int32_t>(s2);   // the taps are the k with (2k + 1) out_size > m
    k0 = m > 0 ? (static_cast<uint32_t>(m) / out_size + 1) >> 1 : 0;
    d = static_cast<int32_t>((2 * k0 + 1) * out_size) - c;
}

__device__ __forceinline__ uint32_t resize_aa_weight(uint32_t s2, int32_t d)
{
    return s2 - static_cast<uint32_t>(d < 0 ? -d : d);
}

__global__ __launch_bounds__(kResizeThreads) void resize_aa_h_kernel(const ResizeDev* __restrict__ items, int groups,
                                                                      int out_w)
{
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    typedef __attribute__((address_space(1))) uint32_t gword;
    const uint32_t img = blockIdx.x / static_cast<uint32_t>(groups);
    const uint32_t grp = blockIdx.x - img * static_cast<uint32_t>(groups);
    const ResizeDev it = items[img];   // group-uniform: scalar loads
    const uint32_t w = static_cast<uint32_t>(it.w), h = static_cast<uint32_t>(it.h);
    const uint32_t wo = static_cast<uint32_t>(out_w);
    const int64_t splane = static_cast<int64_t>(it.pitch) * it.h;
    const bool flip = (it.flags & kResizeFlipH) != 0;
    const uint32_t qw = (wo + 3) >> 2, quads = qw * h;   // (the intermediate's pitch: 4 * qw)
    const int64_t mplane = static_cast<int64_t>(4 * qw) * h;
    const uint32_t s2 = 2 * max(w, wo);
    const int32_t step = static_cast<int32_t>(2 * wo);
    for (uint32_t q = grp * kResizeThreads + threadIdx.x; q < quads; q += static_cast<uint32_t>(groups) * kResizeThreads) {
        const uint32_t y = q / qw, qx = q - y * qw;
        const gcbyte* row = (const gcbyte*)it.src + static_cast<int64_t>(y) * it.pitch;
        uint32_t out[3] = {0, 0, 0};   // the quad's four bytes, per plane
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // (a column past out_w lies in the pitch padding: clamped, computed, never read)
            const uint32_t j = min(4 * qx + k, wo - 1);
            uint32_t x;
            int32_t d;
            resize_aa_first(flip ? wo - 1 - j : j, w, wo, s2, x, d);
            uint32_t T = 0, acc[3] = {0, 0, 0};
            for (; x < w && d < static_cast<int32_t>(s2); ++x, d += step) {
                const uint32_t t = resize_aa_weight(s2, d);
                T += t;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += t * row[c * splane + x];
            }
            const uint32_t r = T >> 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] |= ((acc[c] + r) / T) << (8 * k);
        }
        // (plain stores: the vertical kernel reads them next, from L2)
        gword* m = (gword*)it.dst + (static_cast<int64_t>(y) * qw + qx);
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c * (mplane >> 2)] = out[c];
    }
}

template <int kFormat>
__global__ __launch_bounds__(kResizeThreads) void resize_aa_v_kernel(const ResizeDev* __restrict__ items, int groups,
                                                                      int out_w, int out_h, int out_pitch, NormDev nk)
{
    constexpr int kElem = out_elem_bytes(kFormat);
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    typedef __attribute__((address_space(1))) const uint32_t gcword;
    const uint32_t img = blockIdx.x / static_cast<uint32_t>(groups);
    const uint32_t grp = blockIdx.x - img * static_cast<uint32_t>(groups);
    const ResizeDev it = items[img];   // group-uniform: scalar loads
    const uint32_t h = static_cast<uint32_t>(it.h);
    const uint32_t wo = static_cast<uint32_t>(out_w), ho = static_cast<uint32_t>(out_h);
    const int64_t dplane = static_cast<int64_t>(out_pitch) * out_h;
    const bool vec = store_vec_ok<kFormat>(it.dst, out_pitch) && (wo & 3) == 0;   // whole quads, one vector per plane
    const uint32_t qw = (wo + 3) >> 2, quads = qw * ho;
    const int64_t mplane = static_cast<int64_t>(qw) * h;   // in dwords
    const uint32_t s2 = 2 * max(h, ho);
    const int32_t step = static_cast<int32_t>(2 * ho);
    for (uint32_t q = grp * kResizeThreads + threadIdx.x; q < quads; q += static_cast<uint32_t>(groups) * kResizeThreads) {
        const uint32_t i = q / qw, qx = q - i * qw;
        uint32_t y;
        int32_t d;
        resize_aa_first(i, h, ho, s2, y, d);
        const gcword* m = (const gcword*)it.src + (static_cast<int64_t>(y) * qw + qx);
        uint32_t T = 0, acc[3][4] = {};
        for (; y < h && d < static_cast<int32_t>(s2); ++y, d += step, m += qw) {
            const uint32_t t = resize_aa_weight(s2, d);
            T += t;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t v = m[c * mplane];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[c][k] += t * ((v >> (8 * k)) & 0xffu);
            }
        }
        const uint32_t r = T >> 1;
        uint32_t px[4];   // 0x00RRGGBB
#pragma unroll
        for (int k = 0; k < 4; ++k)
            px[k] = (((acc[0][k] + r) / T) << 16) | (((acc[1][k] + r) / T) << 8) | ((acc[2][k] + r) / T);
        const uint32_t j0 = 4 * qx;
        gbyte* dst = (gbyte*)it.dst + static_cast<int64_t>(i) * out_pitch + static_cast<int64_t>(j0) * kElem;
        store_quad<kFormat>(px, dst, dplane, vec, j0, wo, nk);
    }
}

}  // namespace hjd
