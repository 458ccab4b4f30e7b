// hjd_color.hpp -- the colour kernels for gfx950 (include/hjd.h hjd_color_*;
// DESIGN.md s3.13): n planar uint8 RGB images, each of its own size, each
// through its own affine colour map (a 3 x 3 matrix m, a matrix p on the image's
// channel means and an offset t, all Q12 integers), written as planar uint8 or
// normalised half / float planes.  Exact integer arithmetic, one rounding.
//
// Work decomposition: every image gets the same number of 256-thread groups
// (gridDim.x = n * groups, groups the largest image's groups_per_image), the
// image of a group is blockIdx.x / groups -- group-uniform, its record read
// with scalar loads.  A lane takes quads: 4 horizontally adjacent pixels of one
// row, all three channels; the quads of an image are dealt to its groups'
// threads round-robin and the threads loop once an image has more quads than
// its groups hold.  A quad is one dword load per plane where the source's base
// and pitch are multiples of 4 and the quad lies inside the row, else guarded
// byte loads; it is stored by store_quad (hjd_store.hpp).  A thread reads its
// quad before it writes it and no other thread touches it, so a uint8 launch
// may run in place.  No LDS, no barrier in color_kernel.
//
// The means.  color_sum_kernel, launched only where some record's p is not 0,
// deals the quads the same way and writes each group's three channel sums
// (uint32: a group's share is at most 2^28 / 256 = 2^20 pixels, its sum below
// 2^28) to sums[(image * kColorMaxGroups + group) * 3 + channel]; a group
// without work writes zeros, so the table needs no memset and no atomics, and
// integer sums do not depend on the order.  color_kernel's prologue, in every
// wave of a record that reads the sums: lane l loads the partials of groups l,
// l + 64, l + 128, l + 192 (four loads of three dwords), a butterfly over the
// 64 lanes (__shfl_xor, 6 steps) leaves the image's sums S_k in every lane, and
// mq and T are formed once, in 64 bits, and made wave-uniform.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjd_quad.hpp"
#include "hjd_store.hpp"

namespace hjd {

constexpr int kColorThreads = 256;
constexpr int kColorMaxGroups = 256;   // hjd_internal::kMaxGroups: the rows of an image in the table of sums
constexpr int kColorRound = 2048;      // half of Q12's 4096

// The sum of the four bytes of v.
__device__ __forceinline__ uint32_t color_byte_sum(uint32_t v)
{
    return (v & 0xffu) + ((v >> 8) & 0xffu) + ((v >> 16) & 0xffu) + (v >> 24);
}

// The sum of v over the wave's 64 lanes, in every lane.
__device__ __forceinline__ uint64_t color_wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v)), d, 64));
        const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v >> 32)), d, 64));
        v += (static_cast<uint64_t>(hi) << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(kColorThreads) void color_sum_kernel(const ColorDev* __restrict__ items, int groups,
                                                                   uint32_t* __restrict__ sums)
{
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    __shared__ uint32_t part[kColorThreads / 64][3];
    const uint32_t img = blockIdx.x / static_cast<uint32_t>(groups);
    const uint32_t grp = blockIdx.x - img * static_cast<uint32_t>(groups);
    const ColorDev it = items[img];   // group-uniform: scalar loads
    if (!it.use_sums) return;         // (nobody reads this image's rows of the table)
    const uint32_t w = static_cast<uint32_t>(it.w), h = static_cast<uint32_t>(it.h);
    const int64_t splane = static_cast<int64_t>(it.pitch) * it.h;
    const bool vec = ((reinterpret_cast<uintptr_t>(it.src) | static_cast<uintptr_t>(it.pitch)) & 3u) == 0;
    const uint32_t qw = (w + 3) >> 2, quads = qw * h;
    uint32_t s[3] = {0, 0, 0};   // a thread's share: at most 2^12 pixels
    for (uint32_t q = grp * kColorThreads + threadIdx.x; q < quads; q += static_cast<uint32_t>(groups) * kColorThreads) {
        const uint32_t i = q / qw, j0 = 4 * (q - i * qw);
        const gcbyte* row = (const gcbyte*)it.src + static_cast<int64_t>(i) * it.pitch;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += color_byte_sum(load_quad(row + c * splane, j0, w, vec));
    }
    const uint32_t wave = threadIdx.x / 64;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t ws = static_cast<uint32_t>(color_wave_sum(s[c]));   // below 2^28
        if ((threadIdx.x & 63) == 0) part[wave][c] = ws;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < kColorThreads / 64; ++k) v += part[k][threadIdx.x];
        sums[(static_cast<size_t>(img) * kColorMaxGroups + grp) * 3 + threadIdx.x] = v;
    }
}

template <int kFormat>
__global__ __launch_bounds__(kColorThreads) void color_kernel(const ColorDev* __restrict__ items, int groups,
                                                               const uint32_t* __restrict__ sums, NormDev nk)
{
    constexpr int kElem = out_elem_bytes(kFormat);
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    const uint32_t img = blockIdx.x / static_cast<uint32_t>(groups);
    const uint32_t grp = blockIdx.x - img * static_cast<uint32_t>(groups);
    const ColorDev it = items[img];   // group-uniform: scalar loads
    const uint32_t w = static_cast<uint32_t>(it.w), h = static_cast<uint32_t>(it.h);
    const uint32_t qw = (w + 3) >> 2, quads = qw * h;
    if (grp * kColorThreads >= quads) return;   // a smaller image than the launch's largest: nothing for this group

    // T_c + 2048, the constant of channel c's accumulator (below 2^26 in magnitude)
    int32_t T[3] = {it.t[0] + kColorRound, it.t[1] + kColorRound, it.t[2] + kColorRound};
    if (it.use_sums) {
        const uint32_t lane = threadIdx.x & 63;
        uint64_t S[3] = {0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < kColorMaxGroups / 64; ++k) {
            const uint32_t g = lane + 64 * k;
            if (g < static_cast<uint32_t>(groups)) {
                const uint32_t* ps = sums + (static_cast<size_t>(img) * kColorMaxGroups + g) * 3;
                S[0] += ps[0];
                S[1] += ps[1];
                S[2] += ps[2];
            }
        }
        const uint64_t N = static_cast<uint64_t>(w) * h;
        int64_t mq[3];   // the channel means in Q8: 0 .. 65280
#pragma unroll
        for (int c = 0; c < 3; ++c) mq[c] = static_cast<int64_t>((color_wave_sum(S[c]) * 256 + (N >> 1)) / N);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t pm = it.p[3 * c] * mq[0] + it.p[3 * c + 1] * mq[1] + it.p[3 * c + 2] * mq[2];
            T[c] = __builtin_amdgcn_readfirstlane(T[c] + static_cast<int32_t>((pm + 128) >> 8));
        }
    }

    const int64_t splane = static_cast<int64_t>(it.pitch) * it.h;
    const int64_t dplane = static_cast<int64_t>(it.dst_pitch) * it.h;
    const bool lvec = ((reinterpret_cast<uintptr_t>(it.src) | static_cast<uintptr_t>(it.pitch)) & 3u) == 0;
    const bool svec = store_vec_ok<kFormat>(it.dst, it.dst_pitch) && (w & 3) == 0;   // whole quads, one vector per plane
    for (uint32_t q = grp * kColorThreads + threadIdx.x; q < quads; q += static_cast<uint32_t>(groups) * kColorThreads) {
        const uint32_t i = q / qw, j0 = 4 * (q - i * qw);
        // (global, not flat, addresses: the record's pointers are device memory)
        const gcbyte* row = (const gcbyte*)it.src + static_cast<int64_t>(i) * it.pitch;
        const uint32_t r4 = load_quad(row, j0, w, lvec);
        const uint32_t g4 = load_quad(row + splane, j0, w, lvec);
        const uint32_t b4 = load_quad(row + 2 * splane, j0, w, lvec);
        uint32_t px[4];   // 0x00RRGGBB
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int32_t r = static_cast<int32_t>((r4 >> (8 * k)) & 0xffu), g = static_cast<int32_t>((g4 >> (8 * k)) & 0xffu),
                          b = static_cast<int32_t>((b4 >> (8 * k)) & 0xffu);
            uint32_t pk = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // 24-bit multiply-adds: |m| <= 32767, the bytes <= 255, the sum below 2^27
                const int32_t acc = __mul24(it.m[3 * c], r) + __mul24(it.m[3 * c + 1], g) + __mul24(it.m[3 * c + 2], b) + T[c];
                pk = (pk << 8) | static_cast<uint32_t>(min(max(acc >> 12, 0), 255));   // v_med3_i32
            }
            px[k] = pk;
        }
        gbyte* d = (gbyte*)it.dst + static_cast<int64_t>(i) * it.dst_pitch + static_cast<int64_t>(j0) * kElem;
        store_quad<kFormat>(px, d, dplane, svec, j0, w, nk);
    }
}

}  // namespace hjd
