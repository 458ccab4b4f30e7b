// hjd_store.hpp -- the output side the stage kernels share (hjd_resize.hpp,
// hjd_resize_aa.hpp, hjd_orient.hpp, hjd_warp.hpp): the format constant of their
// kFormat template argument, what follows from it, and the stores of the
// normalised half / float planes.  All stores are to global (not flat)
// addresses: the records' pointers are device memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjd_norm.hpp"

namespace hjd {

constexpr int kOutF16 = 1;   // a stage kernel's kFormat: 0 bytes, else one of these
constexpr int kOutF32 = 2;

// Bytes of one output element.
constexpr int out_elem_bytes(int format) { return format == kOutF32 ? 4 : format == kOutF16 ? 2 : 1; }

// Four adjacent elements of a row can go out as one dword / dwordx2 / dwordx4
// wherever the row starts on a multiple of 4 elements: the image's base and
// pitch are multiples of 4 elements (group-uniform).  (The pitch is widened by
// the caller: widened in here, orient_kernel's schedule came out different.)
template <int kFormat>
__device__ __forceinline__ bool store_vec_ok(const void* dst, int64_t pitch)
{
    return ((reinterpret_cast<uintptr_t>(dst) | static_cast<uintptr_t>(pitch)) & (4 * out_elem_bytes(kFormat) - 1)) == 0;
}

// Four elements of a float format at d: one dwordx2 / dwordx4, non-temporal.
template <int kFormat>
__device__ __forceinline__ void store_vec4(__attribute__((address_space(1))) uint8_t* d, float f0, float f1, float f2,
                                           float f3)
{
    static_assert(kFormat == kOutF16 || kFormat == kOutF32, "the float formats");
    if constexpr (kFormat == kOutF16) {
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        typedef __attribute__((address_space(1))) u32x2 gvec2;
        const u32x2 v = {pack_half2(f0, f1), pack_half2(f2, f3)};
        __builtin_nontemporal_store(v, (gvec2*)d);
    } else {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(1))) f32x4 gvec4;
        const f32x4 v = {f0, f1, f2, f3};
        __builtin_nontemporal_store(v, (gvec4*)d);
    }
}

// One element of a float format: element x of the row at d.
template <int kFormat>
__device__ __forceinline__ void store_one(__attribute__((address_space(1))) uint8_t* d, uint32_t x, float f)
{
    static_assert(kFormat == kOutF16 || kFormat == kOutF32, "the float formats");
    if constexpr (kFormat == kOutF16) {
        typedef __attribute__((address_space(1))) uint16_t ghalf;
        ((ghalf*)d)[x] = static_cast<uint16_t>(half_bits(f));
    } else {
        typedef __attribute__((address_space(1))) float gfloat;
        ((gfloat*)d)[x] = f;
    }
}

// Store one quad: px[k] = 0x00RRGGBB of output columns j0 .. j0 + 3 of one row,
// d the address of plane R's element j0.  vec: one dword / dwordx2 / dwordx4
// per plane; else element stores of the columns below wo.  Non-temporal.
template <int kFormat>
__device__ __forceinline__ void store_quad(const uint32_t (&px)[4], __attribute__((address_space(1))) uint8_t* d,
                                           int64_t dplane, bool vec, uint32_t j0, uint32_t wo, const NormDev& nk)
{
    if constexpr (kFormat == 0) {
        if (vec) {
            typedef __attribute__((address_space(1))) uint32_t gword;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int sh = 16 - 8 * c;
                const uint32_t v = ((px[0] >> sh) & 0xffu) | (((px[1] >> sh) & 0xffu) << 8) |
                                   (((px[2] >> sh) & 0xffu) << 16) | (((px[3] >> sh) & 0xffu) << 24);
                __builtin_nontemporal_store(v, (gword*)(d + c * dplane));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < wo) {
                    d[k] = static_cast<uint8_t>(px[k] >> 16);
                    d[dplane + k] = static_cast<uint8_t>(px[k] >> 8);
                    d[2 * dplane + k] = static_cast<uint8_t>(px[k]);
                }
        }
    } else {
        float f[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f[0][k] = norm_px<0>(px[k], nk);
            f[1][k] = norm_px<1>(px[k], nk);
            f[2][k] = norm_px<2>(px[k], nk);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            __attribute__((address_space(1))) uint8_t* dc = d + c * dplane;
            if (vec) {
                store_vec4<kFormat>(dc, f[c][0], f[c][1], f[c][2], f[c][3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j0 + k < wo) store_one<kFormat>(dc, k, f[c][k]);
            }
        }
    }
}

}  // namespace hjd
