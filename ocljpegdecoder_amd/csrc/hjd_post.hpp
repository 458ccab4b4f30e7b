// hjd_post.hpp -- what the stage objects of include/hjd.h (hjd_resize_*,
// hjd_orient_*, hjd_warp_*; hjd_resize.hip, hjd_orient.hip, hjd_warp.hip) have in
// common on the host: the record table in device memory, the refusals every
// item check opens with, the groups of a launch and the dispatch from an
// out_format to a kernel's kFormat.  Host code, inline: no unit owns it.
#pragma once
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <type_traits>

#include "hjd.h"
#include "hjd_internal.h"
#include "hjd_store.hpp"

#define HJD_HIP(expr)                                                                                            \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return hjd_internal::set_error(HJD_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace hjd_internal {

inline bool dim_ok(int d) { return d >= 1 && d <= kResizeMaxDim; }

// Groups of `threads` threads per image: one unit (a quad, or a thread's place
// in a wave's tile) per thread up to kMaxGroups groups, beyond that the threads loop.
constexpr int kMaxGroups = 256;
inline int groups_per_image(int64_t units, int threads)
{
    const int64_t g = (units + threads - 1) / threads;
    return static_cast<int>(g < kMaxGroups ? g : kMaxGroups);
}

// f(std::integral_constant<int, kFormat>) for the kFormat of a planar out_format
// (hjd_store.hpp), and what it returns; any other format is refused here (no fallback).
template <class F>
int with_out_format(const char* stage, int out_format, F&& f)
{
    switch (out_format) {
    case HJD_OUT_RGB_PLANAR: return f(std::integral_constant<int, 0>{});
    case HJD_OUT_RGB_PLANAR_F16: return f(std::integral_constant<int, hjd::kOutF16>{});
    case HJD_OUT_RGB_PLANAR_F32: return f(std::integral_constant<int, hjd::kOutF32>{});
    default: return set_error(HJD_E_INVALID, "%s: output format %d has no kernel", stage, out_format);
    }
}

// What every kind's item check opens with (`kind`: the noun of its messages).
template <class Rec>
int item_common_check(const char* kind, const Rec& it, int index, int out_format)
{
    if (!it.src || !it.dst) return set_error(HJD_E_INVALID, "%s item %d: src or dst is NULL", kind, index);
    if (reinterpret_cast<uintptr_t>(it.dst) & out_format_align_mask(out_format))
        return set_error(HJD_E_INVALID, "%s item %d: dst must be a multiple of the element size (%d bytes)", kind, index,
                         out_format_row_bytes(out_format));
    if (!dim_ok(it.w) || !dim_ok(it.h))
        return set_error(HJD_E_INVALID, "%s item %d: source size %d x %d is outside 1..%d", kind, index, it.w, it.h,
                         kResizeMaxDim);
    if (it.pitch < it.w)
        return set_error(HJD_E_INVALID, "%s item %d: src_pitch %d is below src_w %d", kind, index, it.pitch, it.w);
    return HJD_OK;
}

// The part of a stage object every kind has: n records in device memory, the
// format its launches write and their normalisation constants.  The public
// objects derive from it and add their own fields.
template <class Rec>
struct StageTable {
    int device = 0;
    int n = 0, out_format = 0;
    Rec* d_items = nullptr;
    NormRecord norm = norm_identity();

    StageTable(hjd_ctx* ctx, int n_, int out_format_) : device(hjd_ctx_device(ctx)), n(n_), out_format(out_format_) {}
    StageTable(const StageTable&) = delete;
    ~StageTable() { release(d_items); }

    // Free device memory of this object (waits for the launches that read it).
    void release(void* p)
    {
        if (!p) return;
        (void)hipSetDevice(device);
        (void)hipFree(p);
    }

    // The end of a create: `count` records to the device, behind whatever the
    // kind did before (e, and `also`, its part of the message).  HJD_OK, or
    // the refusal: the caller then deletes the object.
    int upload(const char* kind, const void* recs, size_t count, hipError_t e = hipSuccess, const std::string& also = "")
    {
        const size_t bytes = sizeof(Rec) * count;
        if (e == hipSuccess) e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_items), bytes);
        if (e != hipSuccess) d_items = nullptr;
        if (e == hipSuccess) e = hipMemcpy(d_items, recs, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) return HJD_OK;
        (void)hipGetLastError();
        return set_error(e == hipErrorOutOfMemory ? HJD_E_NOMEM : HJD_E_HIP, "%s table upload (%zu bytes)%s: %s", kind,
                         bytes, also.c_str(), hipGetErrorString(e));
    }
};

// hjd_<kind>_set_normalize of the object t (or null).
template <class Rec>
int table_set_normalize(const char* kind, StageTable<Rec>* t, const float a[3], const float b[3])
{
    const int rc = norm_check(a, b);
    if (rc) return rc;
    if (!t) return set_error(HJD_E_INVALID, "%s is NULL", kind);
    if (!out_format_float_bytes(t->out_format))
        return set_error(HJD_E_INVALID, "hjd_%s_set_normalize: output format %d is not HJD_OUT_RGB_PLANAR_F16 / _F32", kind,
                         t->out_format);
    for (int c = 0; c < 3; ++c) {   // a launch argument: an enqueued launch keeps its own
        t->norm.a[c] = a[c];
        t->norm.b[c] = b[c];
    }
    return HJD_OK;
}

}  // namespace hjd_internal
