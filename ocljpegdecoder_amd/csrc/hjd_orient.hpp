// hjd_orient.hpp -- the orientation kernel for gfx950 (include/hjd.h
// hjd_orient_*): n planar uint8 RGB images, each of its own
// size, permuted by their EXIF orientation (1..8) and written as planar uint8
// or normalised half / float planes.  A pure permutation of bytes.
//
// Work decomposition: a tile is 128 x 128 bytes of one stored plane, one
// 256-thread group per tile; an image has 3 * ceil(w / 128) * ceil(h / 128) of
// them and its record carries the prefix tile_begin, so a group finds its
// image by bisection over the records (group-uniform: scalar loads) and its
// plane and tile from the remainder.  One launch serves all images.
//
// The tile is 32 dword columns wide, one per lane of a 32-lane half-wave, so
// every global access of a half-wave is one whole 128-byte line of a row.  A
// thread reads four 4 x 4 byte blocks (pass p: rows 4 rq .. 4 rq + 3 of dword
// column cd, rq = tid / 32 + 8 p).  Orientations 5..8 transpose: each block is
// transposed in registers (8 v_perm_b32), its four dwords go to the LDS image
// of the transposed tile (128 rows x 32 dwords, 16 KiB) and come back along
// that tile's rows, so the global writes run along output rows as the reads
// ran along stored rows.  The LDS image has no padding: dword (row, col) lies
// at row * 32 + (col ^ (row >> 2)), so its bank (a / 4) % 32 is col ^ (row >> 2).
// A ds_write_b32 half-wave holds 32 rows 4 apart (row >> 2 = cd, all distinct)
// of one column, a ds_read_b32 half-wave the 32 columns of one row: 32
// distinct banks both ways, conflict degree 1.
// Orientations 1..4 skip the exchange.  A horizontal flip is a byte swap of
// the dword (v_perm_b32) stored at the mirrored dword position; a vertical
// flip is the row index.
//
// Whole dwords move where the image's base and pitch are multiples of 4 (the
// output's: of 4 elements) and no dword straddles the image's edge; any other
// tile takes guarded byte loads / element stores.  The two sides decide
// independently, per tile, group-uniformly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjd_store.hpp"

namespace hjd {

constexpr int kOrientThreads = 256;
constexpr int kOrientTile = 128;       // bytes per tile edge: one cache line

// Bytes 3, 2, 1, 0 of w.
__device__ __forceinline__ uint32_t orient_bswap(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x00010203u); }

// Byte k of q as the output element of channel constants (a, b).
__device__ __forceinline__ float orient_norm(uint32_t q, int k, float a, float b)
{
    return __builtin_fmaf(static_cast<float>((q >> (8 * k)) & 0xffu), a, b);
}

// Four output elements (the bytes of q, lowest first) of channel constants
// (a, b) at d: one dword / dwordx2 / dwordx4, non-temporal.
template <int kFormat>
__device__ __forceinline__ void orient_store_vec(uint32_t q, __attribute__((address_space(1))) uint8_t* d, float a,
                                                 float b)
{
    if constexpr (kFormat == 0) {
        typedef __attribute__((address_space(1))) uint32_t gword;
        __builtin_nontemporal_store(q, (gword*)d);
    } else {
        store_vec4<kFormat>(d, orient_norm(q, 0, a, b), orient_norm(q, 1, a, b), orient_norm(q, 2, a, b),
                            orient_norm(q, 3, a, b));
    }
}

// One output element (byte u8) at element index x of the row at d.
template <int kFormat>
__device__ __forceinline__ void orient_store_one(uint32_t u8, __attribute__((address_space(1))) uint8_t* d, uint32_t x,
                                                 float a, float b)
{
    if constexpr (kFormat == 0) d[x] = static_cast<uint8_t>(u8);
    else store_one<kFormat>(d, x, orient_norm(u8, 0, a, b));
}

template <int kFormat>
__global__ __launch_bounds__(kOrientThreads) void orient_kernel(const OrientDev* __restrict__ items, int n, NormDev nk)
{
    constexpr int kElem = out_elem_bytes(kFormat);
    constexpr uint32_t T = kOrientTile;
    constexpr uint32_t kCols = T / 4;                       // dword columns of a tile: 32, one per lane of a half-wave
    constexpr uint32_t kRowsPerPass = kOrientThreads / kCols;   // 8 row quads (loads) / 8 rows (stores) per pass
    constexpr uint32_t kPasses = T / 4 / kRowsPerPass;      // 4
    typedef __attribute__((address_space(1))) uint8_t gbyte;
    typedef __attribute__((address_space(1))) const uint8_t gcbyte;
    typedef __attribute__((address_space(1))) const uint32_t gcword;
    __shared__ uint32_t lds[T * kCols];

    // the image of this group: the last record whose tile_begin <= blockIdx.x
    // (items[0].tile_begin == 0 and the grid is the tile total)
    uint32_t lo = 0, hi = static_cast<uint32_t>(n);
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (items[mid].tile_begin <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const OrientDev it = items[lo];   // group-uniform: scalar loads
    const uint32_t w = static_cast<uint32_t>(it.w), h = static_cast<uint32_t>(it.h);
    const uint32_t tiles_x = (w + T - 1) / T, tiles_y = (h + T - 1) / T;
    uint32_t t = blockIdx.x - it.tile_begin;
    const uint32_t c = t / (tiles_x * tiles_y);   // the plane: 0 R, 1 G, 2 B
    t -= c * tiles_x * tiles_y;
    const uint32_t tyi = t / tiles_x, x0 = T * (t - tyi * tiles_x), y0 = T * tyi;
    const uint32_t o = static_cast<uint32_t>(it.orientation);
    const bool tr = o >= 5, fh = (0xCCu >> o) & 1u /* 2 3 6 7 */, fv = (0x198u >> o) & 1u /* 3 4 7 8 */;

    const uint32_t cd = threadIdx.x % kCols, rq0 = threadIdx.x / kCols;

    // ---- read: pass p, rows y0 + 4 (rq0 + 8 p) + i, bytes x0 + 4 cd .. + 3 (0 outside the image)
    const gcbyte* sp = (const gcbyte*)it.src + static_cast<int64_t>(c) * it.pitch * it.h;
    const bool load_vec = ((reinterpret_cast<uintptr_t>(it.src) | static_cast<uintptr_t>(it.pitch)) & 3u) == 0 &&
                          ((w & 3u) == 0 || x0 + T <= w);
    const uint32_t x = x0 + 4 * cd;
    uint32_t r[kPasses][4];
#pragma unroll
    for (uint32_t p = 0; p < kPasses; ++p) {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t y = y0 + 4 * (rq0 + kRowsPerPass * p) + i;
            const gcbyte* row = sp + static_cast<int64_t>(y) * it.pitch;
            uint32_t v = 0;
            if (y < h) {
                if (load_vec) {
                    if (x + 4 <= w) v = *(gcword*)(row + x);
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (x + b < w) v |= static_cast<uint32_t>(row[x + b]) << (8 * b);
                }
            }
            r[p][i] = v;
        }
    }

    // ---- the tile as the output sees it before the flips: U = S or its transpose
    if (tr) {
#pragma unroll
        for (uint32_t p = 0; p < kPasses; ++p) {
            // 4 x 4 bytes transposed: tv[k] = (r0[k], r1[k], r2[k], r3[k]), which is
            // dword (row 4 cd + k, col rq) of the transposed tile
            const uint32_t rq = rq0 + kRowsPerPass * p;
            const uint32_t lo01 = __builtin_amdgcn_perm(r[p][1], r[p][0], 0x05010400u);
            const uint32_t hi01 = __builtin_amdgcn_perm(r[p][1], r[p][0], 0x07030602u);
            const uint32_t lo23 = __builtin_amdgcn_perm(r[p][3], r[p][2], 0x05010400u);
            const uint32_t hi23 = __builtin_amdgcn_perm(r[p][3], r[p][2], 0x07030602u);
            const uint32_t tv[4] = {__builtin_amdgcn_perm(lo23, lo01, 0x05040100u),
                                    __builtin_amdgcn_perm(lo23, lo01, 0x07060302u),
                                    __builtin_amdgcn_perm(hi23, hi01, 0x05040100u),
                                    __builtin_amdgcn_perm(hi23, hi01, 0x07060302u)};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) lds[(4 * cd + k) * kCols + (rq ^ cd)] = tv[k];   // col ^ (row >> 2)
        }
        __syncthreads();
    }

    // ---- write: U's row uy, bytes ux .. ux + 3, flipped into the output
    const uint32_t uw = tr ? h : w, uh = tr ? w : h;
    const uint32_t ux0 = tr ? y0 : x0, uy0 = tr ? x0 : y0;
    const float na = c == 0 ? nk.a[0] : c == 1 ? nk.a[1] : nk.a[2];
    const float nb = c == 0 ? nk.b[0] : c == 1 ? nk.b[1] : nk.b[2];
    gbyte* dp = (gbyte*)it.dst + static_cast<int64_t>(c) * it.dst_pitch * static_cast<int64_t>(uh);
    const bool store_vec = store_vec_ok<kFormat>(it.dst, it.dst_pitch) && ((uw & 3u) == 0 || (!fh && ux0 + T <= uw));
    const uint32_t ux = ux0 + 4 * cd;
#pragma unroll
    for (uint32_t m = 0; m < 4 * kPasses; ++m) {
        // transposed: row rq0 + 8 m of the LDS image; else this thread's own row i of pass p
        const uint32_t row = tr ? rq0 + kRowsPerPass * m : 4 * (rq0 + kRowsPerPass * (m >> 2)) + (m & 3u);
        const uint32_t uy = uy0 + row;
        if (uy >= uh) continue;
        const uint32_t q = tr ? lds[row * kCols + (cd ^ (row >> 2))] : r[m >> 2][m & 3u];
        gbyte* drow = dp + static_cast<int64_t>(fv ? uh - 1 - uy : uy) * it.dst_pitch;
        if (store_vec) {
            if (ux + 4 <= uw)
                orient_store_vec<kFormat>(fh ? orient_bswap(q) : q,
                                          drow + static_cast<int64_t>(fh ? uw - 4 - ux : ux) * kElem, na, nb);
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b)
                if (ux + b < uw)
                    orient_store_one<kFormat>((q >> (8 * b)) & 0xffu, drow, fh ? uw - 1 - (ux + b) : ux + b, na, nb);
        }
    }
}

}  // namespace hjd
