// hjd_norm.hpp -- the arithmetic of the normalised float output formats
// (HJD_OUT_RGB_PLANAR_F16 / _F32), shared by the fused pixel
// kernels (hjd_kernels.hpp) and the stage kernels (hjd_store.hpp): one
// definition of out = fma((float)u8, a[c], b[c]) and of its rounding to half.
// The constants' record, NormDev, is in hjd_records.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hjd_records.h"

namespace hjd {

// Channel c (0 R, 1 G, 2 B) of BGRX word p as the normalised fp32 value: the
// byte is converted in place (v_cvt_f32_ubyte2/1/0), then one fused
// multiply-add, correctly rounded (never a multiply followed by an add).
template <int kC>
__device__ __forceinline__ float norm_px(uint32_t p, const NormDev& nk)
{
    return __builtin_fmaf(static_cast<float>((p >> (16 - 8 * kC)) & 0xffu), nk.a[kC], nk.b[kC]);
}
// fp32 -> IEEE half in the low 16 bits, rounded to nearest-even under the
// kernels' default mode (overflow to inf, subnormals kept).  The instruction
// is spelled out so that the fp32 value -- the definition's first rounding --
// exists: left to the compiler, the convert folds into v_fma_mixlo_f16 or
// pairs up as gfx950's v_cvt_pk_f16_f32, and the latter's results differed
// from fp32-then-half rounding on MI355X where the fp32 value is a half tie
// (tests/test_gpu_norm_outputs.py test_half_is_rounded_twice).
__device__ __forceinline__ uint32_t half_bits(float f)
{
    uint32_t w;
    asm("v_cvt_f16_f32_e32 %0, %1" : "=v"(w) : "v"(f));
    return w;
}
// Two fp32 values as two halves in one dword (low half first): the second
// convert writes the high half in place (SDWA), so no pack instruction.
__device__ __forceinline__ uint32_t pack_half2(float lo, float hi)
{
    uint32_t w = half_bits(lo);
    asm("v_cvt_f16_f32_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(w) : "v"(hi));
    return w;
}

}  // namespace hjd
