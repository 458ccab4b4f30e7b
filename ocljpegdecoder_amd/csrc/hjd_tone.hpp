// hjd_tone.hpp -- the tone-curve kernels for gfx950 (include/hjd.h hjd_tone_*;
// DESIGN.md s3.14): n planar uint8 RGB images, each of its own size, each
// through its own pointwise map u8_c = lut[c][D_c[x_c]] -- a 3 x 256 table
// behind a data curve D_c that is the identity (mode 0) or built from the
// image's histogram (autocontrast, equalize) -- written as planar uint8 or
// normalised half / float planes.
//
// Work decomposition: hjd_color.hpp's.  Every image gets the same number of
// 256-thread groups, the image of a group is blockIdx.x / groups, its record is
// read group-uniformly, a lane takes quads (load_quad, hjd_quad.hpp) and stores them by
// store_quad (hjd_store.hpp); a thread reads its quad before it writes it, so
// a uint8 launch may run in place.
//
// tone_hist_kernel (only where some record's mode is not 0; groups of mode-0
// images return at once): at most kToneHistGroups groups per image, the threads
// loop.  Each wave counts into its own 3 x 256 uint32 histogram in LDS with LDS
// integer adds (ds_add_u32: lanes on one bin are serialised by the LDS, never
// lost); the four are merged behind a barrier and every group writes its whole
// partial to hist[image * 16 + group][c][v] -- zeros where it had no quads -- so
// the table needs no memset and no global atomics, and a reused one no
// clearing.  The columns of a quad past w are not counted.
//
// tone_lut_kernel: one group of three waves per image, wave c channel c.  Lane
// l sums bins 4l .. 4l + 3 over the image's partials (one dwordx4 each), an
// inclusive scan over the wave gives the counts below each bin, a butterfly the
// extreme non-empty bins and the count of the highest; hjd::tone_data_curve
// (hjd_tone_curve.h, the host's function too) gives D_c, the record's table is
// read through it and the lane writes four bytes of luts[image][c].
//
// tone_kernel: a group stages its image's 768 bytes (luts[image], or the
// record's table where the mode is 0) into LDS, one dword per thread of the
// first 192, and after one barrier runs the quad loop: twelve byte lookups
// (ds_read_u8) a quad.  Each channel's table lies on a 256-byte boundary: one
// row of the 64 four-byte banks, so lanes reading one dword broadcast and lanes
// reading different dwords of a channel hit different banks.  A group without
// quads returns before the barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjd_quad.hpp"
#include "hjd_records.h"
#include "hjd_store.hpp"
#include "hjd_tone_curve.h"

namespace hjd {

constexpr int kToneThreads = 256;      // hjd_color.hpp kColorThreads: color_groups counts these groups
constexpr int kToneHistGroups = 16;   // the rows of an image in the table of partial histograms
constexpr int kToneLutThreads = 192;  // a wave per channel

__global__ __launch_bounds__(kToneThreads) void tone_hist_kernel(const ToneDev* __restrict__ items, int groups,
                                                                  uint32_t* __restrict__ hist)
{
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    __shared__ uint32_t bins[kToneThreads / 64][3][256];   // a histogram per wave: 12 KiB
    const uint32_t img = blockIdx.x / static_cast<uint32_t>(groups);
    const uint32_t grp = blockIdx.x - img * static_cast<uint32_t>(groups);
    const ToneDev* it = items + img;   // group-uniform: scalar loads
    if (it->mode == 0) return;         // (nobody reads this image's rows of the table)
    const uint32_t w = static_cast<uint32_t>(it->w), h = static_cast<uint32_t>(it->h);
    const int32_t pitch = it->pitch;
    const uint8_t* src = static_cast<const uint8_t*>(it->src);
    const int64_t splane = static_cast<int64_t>(pitch) * it->h;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | static_cast<uintptr_t>(pitch)) & 3u) == 0;
    const uint32_t qw = (w + 3) >> 2, quads = qw * h;
    uint32_t* flat = &bins[0][0][0];
#pragma unroll
    for (int k = 0; k < 12; ++k) flat[threadIdx.x + kToneThreads * k] = 0;
    __syncthreads();
    uint32_t(*mine)[256] = bins[threadIdx.x / 64];
    for (uint32_t q = grp * kToneThreads + threadIdx.x; q < quads; q += static_cast<uint32_t>(groups) * kToneThreads) {
        const uint32_t i = q / qw, j0 = 4 * (q - i * qw);
        const uint32_t cols = min(4u, w - j0);   // the quad's columns inside the image
        const gcbyte* row = (const gcbyte*)src + static_cast<int64_t>(i) * pitch;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t v4 = load_quad(row + c * splane, j0, w, vec);
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b)
                if (b < cols) atomicAdd(&mine[c][(v4 >> (8 * b)) & 0xffu], 1u);   // ds_add_u32
        }
    }
    __syncthreads();
    uint32_t* out = hist + (static_cast<size_t>(img) * kToneHistGroups + grp) * 768;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t e = threadIdx.x + kToneThreads * k;   // c * 256 + v
        out[e] = flat[e] + flat[768 + e] + flat[2 * 768 + e] + flat[3 * 768 + e];
    }
}

// max and min of v over the wave's 64 lanes, in every lane.
__device__ __forceinline__ uint32_t tone_wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), d, 64)));
    return v;
}
__device__ __forceinline__ uint32_t tone_wave_min(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), d, 64)));
    return v;
}

__global__ __launch_bounds__(kToneLutThreads) void tone_lut_kernel(const ToneDev* __restrict__ items, int groups,
                                                                    const uint32_t* __restrict__ hist,
                                                                    uint8_t* __restrict__ luts)
{
    const uint32_t img = blockIdx.x;
    const ToneDev* it = items + img;   // group-uniform: scalar loads
    const int mode = it->mode;
    if (mode == 0) return;
    const uint32_t c = threadIdx.x / 64, lane = threadIdx.x & 63;
    uint32_t b[4] = {0, 0, 0, 0};   // bins 4 lane .. 4 lane + 3 of channel c
    for (int g = 0; g < groups; ++g) {
        const uint4 p = *reinterpret_cast<const uint4*>(hist + (static_cast<size_t>(img) * kToneHistGroups + g) * 768 +
                                                        c * 256 + 4 * lane);
        b[0] += p.x;
        b[1] += p.y;
        b[2] += p.z;
        b[3] += p.w;
    }
    const uint32_t mine = b[0] + b[1] + b[2] + b[3];
    uint32_t incl = mine;   // the inclusive scan of the lanes' counts
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), d, 64));
        if (lane >= static_cast<uint32_t>(d)) incl += o;
    }
    const uint32_t n = static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63, 64));   // w * h
    uint32_t first = 256, top = 0, top_count = 0;   // this lane's non-empty bins: the lowest, the highest + 1
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if (b[k]) first = 4 * lane + k;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (b[k]) top = 4 * lane + k + 1;
    const uint32_t lo = tone_wave_min(first);
    const uint32_t hi = tone_wave_max(top) - 1;   // (n >= 1: some bin is not empty)
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * lane + k == hi) top_count = b[k];
    const uint32_t last = tone_wave_max(top_count);
    uint32_t below = incl - mine, packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t d = tone_data_curve(mode, 4 * lane + k, below, lo, hi, last, n);
        packed |= static_cast<uint32_t>(it->lut[c][d]) << (8 * k);
        below += b[k];
    }
    reinterpret_cast<uint32_t*>(luts + static_cast<size_t>(img) * 768 + c * 256)[lane] = packed;
}

template <int kFormat>
__global__ __launch_bounds__(kToneThreads) void tone_kernel(const ToneDev* __restrict__ items, int groups,
                                                             const uint8_t* __restrict__ luts, NormDev nk)
{
    constexpr int kElem = out_elem_bytes(kFormat);
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    // a channel's table on a 256-byte boundary: one row of the 64 banks
    __shared__ __attribute__((aligned(256))) uint8_t tab[3][256];
    const uint32_t img = blockIdx.x / static_cast<uint32_t>(groups);
    const uint32_t grp = blockIdx.x - img * static_cast<uint32_t>(groups);
    const ToneDev* it = items + img;   // group-uniform: scalar loads
    const uint32_t w = static_cast<uint32_t>(it->w), h = static_cast<uint32_t>(it->h);
    const uint32_t qw = (w + 3) >> 2, quads = qw * h;
    if (grp * kToneThreads >= quads) return;   // a smaller image than the launch's largest: nothing for this group

    if (threadIdx.x < 192) {
        const uint32_t* from = it->mode ? reinterpret_cast<const uint32_t*>(luts + static_cast<size_t>(img) * 768)
                                        : reinterpret_cast<const uint32_t*>(&it->lut[0][0]);
        reinterpret_cast<uint32_t*>(&tab[0][0])[threadIdx.x] = from[threadIdx.x];
    }
    __syncthreads();

    const int32_t pitch = it->pitch, dst_pitch = it->dst_pitch;
    const uint8_t* src = static_cast<const uint8_t*>(it->src);
    uint8_t* dst = static_cast<uint8_t*>(it->dst);
    const int64_t splane = static_cast<int64_t>(pitch) * it->h;
    const int64_t dplane = static_cast<int64_t>(dst_pitch) * it->h;
    const bool lvec = ((reinterpret_cast<uintptr_t>(src) | static_cast<uintptr_t>(pitch)) & 3u) == 0;
    const bool svec = store_vec_ok<kFormat>(dst, dst_pitch) && (w & 3) == 0;   // whole quads, one vector per plane
    for (uint32_t q = grp * kToneThreads + threadIdx.x; q < quads; q += static_cast<uint32_t>(groups) * kToneThreads) {
        const uint32_t i = q / qw, j0 = 4 * (q - i * qw);
        // (global, not flat, addresses: the record's pointers are device memory)
        const gcbyte* row = (const gcbyte*)src + static_cast<int64_t>(i) * pitch;
        const uint32_t r4 = load_quad(row, j0, w, lvec);
        const uint32_t g4 = load_quad(row + splane, j0, w, lvec);
        const uint32_t b4 = load_quad(row + 2 * splane, j0, w, lvec);
        uint32_t px[4];   // 0x00RRGGBB
#pragma unroll
        for (int k = 0; k < 4; ++k)
            px[k] = (static_cast<uint32_t>(tab[0][(r4 >> (8 * k)) & 0xffu]) << 16) |
                    (static_cast<uint32_t>(tab[1][(g4 >> (8 * k)) & 0xffu]) << 8) |
                    static_cast<uint32_t>(tab[2][(b4 >> (8 * k)) & 0xffu]);
        gbyte* d = (gbyte*)dst + static_cast<int64_t>(i) * dst_pitch + static_cast<int64_t>(j0) * kElem;
        store_quad<kFormat>(px, d, dplane, svec, j0, w, nk);
    }
}

}  // namespace hjd
