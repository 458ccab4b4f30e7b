// hjd_conv.hpp -- the filter kernel for gfx950 (include/hjd.h hjd_conv_*;
// DESIGN.md s3.15): n planar uint8 RGB images, each of its own size, each
// through its own separable neighbourhood filter of radius (rx, ry) <= 11 with a
// blend against the centre pixel, u8 = clamp((a (x << 24) + b S + 2^35) >> 36),
// written as planar uint8 or normalised half / float planes.
//
// Work decomposition: a tile is 64 x 32 output pixels of the three planes, one
// 256-thread group per tile; an image has ceil(w / 64) * ceil(h / 32) of them
// and its record carries the prefix tile_begin, so a group finds its image by
// orient_kernel's bisection over the records (group-uniform: scalar loads).
// One launch serves all images.  A thread owns the quads (q, r) and (q, r + 16)
// of the tile, q = tid % 16, r = tid / 16, and stores each through store_quad.
//
// Per plane, three steps with a barrier behind each:
//   load   the (64 + 2 rx) x (32 + 2 ry) source bytes of the tile and its halo
//          go to LDS, rows kConvSrcPitch bytes apart, each position through
//          conv_src_index: the border is resolved here, and neither pass
//          branches on position.  A thread assembles a dword of four bytes
//          (guarded byte loads: rx is odd as often as not, so the halo's first
//          byte is on no dword) and writes it with one ds_write_b32.
//   rows   a thread takes a quad of one of the 32 + 2 ry rows: dwords d = 0 ..
//          of the row from column 4 q on, two in flight, v_alignbyte gives the
//          four bytes under tap 4 d + b for the quad's four columns; the taps
//          are scalar loads (kh[p] = 0 beyond 2 rx: the check demands it, so
//          the last dword's surplus bytes, whatever LDS holds there, count 0).
//          The four uint32 row sums (<= 255 * 4096) go out as one ds_write_b128.
//   cols   a thread reads its quads' row sums under the 2 ry + 1 taps of kv
//          (ds_read_b128 each) into uint32 (<= 255 * 2^24: above int32), reads
//          the centre bytes, and finishes in 64 bits by conv_finish
//          (hjd_conv_math.h, the host reference's function too).  The KEEP band
//          is a select of the centre byte per pixel.
// LDS: 54 rows x 92 bytes + 54 x 64 uint32 = 18.4 KiB at most, fixed.
//
// The source rows' pitch of 23 dwords: a half-wave of the row pass reads two
// rows of 16 consecutive dwords, whose banks (23 r + q) % 32 overlap in 7 of
// 32 (2-way there); the column pass reads whole 256-byte rows.  Counted at
// radius 11 on random bytes, a fifth of the LDS cycles are bank-conflict
// cycles.
//
// A record with rx = ry = 0 uses no LDS: S = kh[0] kv[0] x, a pointwise map,
// in color_kernel's quad loop over the tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjd_conv_math.h"
#include "hjd_quad.hpp"
#include "hjd_records.h"
#include "hjd_store.hpp"

namespace hjd {

constexpr int kConvThreads = 256;
constexpr int kConvTileW = 64, kConvTileH = 32;
constexpr int kConvMaxRadius = 11;
constexpr int kConvRows = kConvTileH + 2 * kConvMaxRadius;   // 54
// bytes of a source row in LDS: the 64 + 2 rx loaded ones, and what the row
// pass's last dword pair reaches past them (4 * 15 + 4 * 6 + 8 = 92)
constexpr int kConvSrcPitch = 92;
static_assert(kConvSrcPitch % 4 == 0 && kConvSrcPitch >= kConvTileW + 2 * kConvMaxRadius + 6, "the row pass reads dwords");

template <int kFormat>
__global__ __launch_bounds__(kConvThreads) void conv_kernel(const ConvDev* __restrict__ items, int n, NormDev nk)
{
    constexpr int kElem = out_elem_bytes(kFormat);
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    __shared__ __attribute__((aligned(16))) uint32_t src4[kConvRows * kConvSrcPitch / 4];
    __shared__ __attribute__((aligned(16))) uint32_t sums[kConvRows * kConvTileW];

    // the image of this group: the last record whose tile_begin <= blockIdx.x
    // (items[0].tile_begin == 0 and the grid is the tile total)
    uint32_t lo = 0, hi = static_cast<uint32_t>(n);
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (items[mid].tile_begin <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const ConvDev* it = items + lo;   // group-uniform: scalar loads
    const int32_t w = it->w, h = it->h, rx = it->rx, ry = it->ry, border = it->border;
    const int32_t fa = it->a, fb = it->b;
    const int32_t pitch = it->pitch, dst_pitch = it->dst_pitch;
    const uint32_t tiles_x = (static_cast<uint32_t>(w) + kConvTileW - 1) / kConvTileW;
    const uint32_t t = blockIdx.x - it->tile_begin;
    const uint32_t ty = t / tiles_x;
    const int32_t x0 = kConvTileW * static_cast<int32_t>(t - ty * tiles_x), y0 = kConvTileH * static_cast<int32_t>(ty);
    const int64_t splane = static_cast<int64_t>(pitch) * h;
    const int64_t dplane = static_cast<int64_t>(dst_pitch) * h;
    const gcbyte* src = (const gcbyte*)it->src;   // (global, not flat, addresses: the record's pointers are device memory)
    gbyte* dst = (gbyte*)it->dst;
    const bool svec = store_vec_ok<kFormat>(it->dst, dst_pitch) && (w & 3) == 0;   // whole quads, one vector per plane
    const bool keep = border == 0;

    const uint32_t q = threadIdx.x % 16, r = threadIdx.x / 16;   // this thread's quads: (q, r) and (q, r + 16)
    const int32_t j0 = x0 + 4 * static_cast<int32_t>(q);
    uint32_t px[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};   // 0x00RRGGBB

    if (rx == 0 && ry == 0) {
        const uint32_t k00 = static_cast<uint32_t>(it->kh[0]) * static_cast<uint32_t>(it->kv[0]);   // <= 2^24
        const bool lvec = ((reinterpret_cast<uintptr_t>(it->src) | static_cast<uintptr_t>(pitch)) & 3u) == 0;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int32_t i = y0 + static_cast<int32_t>(r) + 16 * half;
            if (i >= h || j0 >= w) continue;
            const gcbyte* row = src + static_cast<int64_t>(i) * pitch;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t v4 = load_quad(row + c * splane, static_cast<uint32_t>(j0), static_cast<uint32_t>(w), lvec);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t x = (v4 >> (8 * k)) & 0xffu;
                    px[half][k] = (px[half][k] << 8) | conv_finish(fa, fb, x, k00 * x);
                }
            }
            gbyte* d = dst + static_cast<int64_t>(i) * dst_pitch + static_cast<int64_t>(j0) * kElem;
            store_quad<kFormat>(px[half], d, dplane, svec, static_cast<uint32_t>(j0), static_cast<uint32_t>(w), nk);
        }
        return;
    }

    const int32_t cols4 = (kConvTileW + 2 * rx + 3) >> 2;   // dwords of a loaded row
    const int32_t rows = kConvTileH + 2 * ry;               // loaded rows, and rows of row sums
    const int32_t nd = (2 * rx + 4) >> 2;                   // dwords of taps: ceil((2 rx + 1) / 4)
    const uint8_t* src1 = reinterpret_cast<const uint8_t*>(src4);

    for (int c = 0; c < 3; ++c) {
        // ---- load: LDS byte (yy, xx) = X(x0 - rx + xx, y0 - ry + yy) of plane c
        const gcbyte* sp = src + c * splane;
        for (int32_t e = static_cast<int32_t>(threadIdx.x); e < rows * cols4; e += kConvThreads) {
            const int32_t yy = e / cols4, xd = e - yy * cols4;
            const gcbyte* row = sp + static_cast<int64_t>(conv_src_index(y0 - ry + yy, h, border)) * pitch;
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                v |= static_cast<uint32_t>(row[conv_src_index(x0 - rx + 4 * xd + b, w, border)]) << (8 * b);
            src4[yy * (kConvSrcPitch / 4) + xd] = v;
        }
        __syncthreads();

        // ---- rows: sums[yy][4 qq + k] = sum over p of kh[p] * byte (yy, 4 qq + k + p)
        for (int32_t e = static_cast<int32_t>(threadIdx.x); e < rows * 16; e += kConvThreads) {
            const int32_t yy = e >> 4, qq = e & 15;
            const uint32_t* rowd = src4 + yy * (kConvSrcPitch / 4) + qq;
            uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            uint32_t cur = rowd[0];
            for (int32_t d = 0; d < nd; ++d) {
                const uint32_t nxt = rowd[d + 1];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t tap = it->kh[4 * d + b];   // uniform: a scalar load; 0 beyond 2 rx
                    // bytes 4 d + b .. + 3 of the row from 4 qq
                    const uint32_t v = b ? __builtin_amdgcn_alignbyte(nxt, cur, b) : cur;
                    s0 += tap * (v & 0xffu);
                    s1 += tap * ((v >> 8) & 0xffu);
                    s2 += tap * ((v >> 16) & 0xffu);
                    s3 += tap * (v >> 24);
                }
                cur = nxt;
            }
            *reinterpret_cast<uint4*>(sums + yy * kConvTileW + 4 * qq) = make_uint4(s0, s1, s2, s3);
        }
        __syncthreads();

        // ---- cols and the finish: this thread's two quads
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int32_t rr = static_cast<int32_t>(r) + 16 * half;
            const uint32_t* col = sums + rr * kConvTileW + 4 * q;
            uint32_t S[4] = {0, 0, 0, 0};
            for (int32_t p = 0; p <= 2 * ry; ++p) {
                const uint32_t tap = it->kv[p];
                const uint4 s = *reinterpret_cast<const uint4*>(col + p * kConvTileW);
                S[0] += tap * s.x;
                S[1] += tap * s.y;
                S[2] += tap * s.z;
                S[3] += tap * s.w;
            }
            const int32_t i = y0 + rr;
            const bool band_y = i < ry || i >= h - ry;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t x = src1[(rr + ry) * kConvSrcPitch + 4 * q + k + rx];
                const int32_t j = j0 + k;
                const uint32_t u = conv_finish(fa, fb, x, S[k]);
                px[half][k] = (px[half][k] << 8) | ((keep && (band_y || j < rx || j >= w - rx)) ? x : u);
            }
        }
        __syncthreads();   // the next plane's load and row pass overwrite what this one read
    }

#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int32_t i = y0 + static_cast<int32_t>(r) + 16 * half;
        if (i >= h || j0 >= w) continue;
        gbyte* d = dst + static_cast<int64_t>(i) * dst_pitch + static_cast<int64_t>(j0) * kElem;
        store_quad<kFormat>(px[half], d, dplane, svec, static_cast<uint32_t>(j0), static_cast<uint32_t>(w), nk);
    }
}

}  // namespace hjd
