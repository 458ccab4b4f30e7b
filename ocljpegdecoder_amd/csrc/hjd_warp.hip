// hjd_warp.hip -- the warp object of include/hjd.h (hjd_warp_*), the host-only
// geometry that goes with it (hjd_warp_roi, hjd_warp_orient) and the launch of
// hjd::warp_kernel, which the GPU decoder's warped decode (hjd_gdec_post.hip)
// shares.  DESIGN.md s3.12.
#include "hjd_warp.hpp"

#include <algorithm>
#include <cstring>

#include "hjd_post.hpp"

using hjd_internal::set_error;

static_assert(sizeof(hjd_warp_item) == sizeof(hjd::WarpDev) && offsetof(hjd_warp_item, dst) == 8 &&
                  offsetof(hjd_warp_item, src_w) == 16 && offsetof(hjd_warp_item, flags) == 28 &&
                  offsetof(hjd_warp_item, m) == 32 && offsetof(hjd_warp_item, fill) == 56 &&
                  offsetof(hjd_warp_item, reserved) == 60,
              "hjd_warp_item is the kernel's record");
static_assert(HJD_WARP_REPLICATE == hjd::kWarpReplicate, "flags bit 0");

struct hjd_warp : hjd_internal::StageTable<hjd::WarpDev> {
    using StageTable::StageTable;
    int out_w = 0, out_h = 0, out_pitch = 0;
};

namespace {

// The units of an image dealt to its groups' threads: its quads, or (tiled) a
// thread's place in each wave's tile.
int64_t warp_units(int out_w, int out_h, bool tiled)
{
    const int64_t qw = (out_w + 3) / 4;
    return tiled ? ((qw + hjd::kWarpTileQuads - 1) / hjd::kWarpTileQuads) *
                       ((out_h + hjd::kWarpTileRows - 1) / hjd::kWarpTileRows) * 64
                 : qw * out_h;
}

inline int64_t floor_q16(int64_t v) { return v >> 16; }   // (arithmetic shift: floor)

inline int clamp_int(int64_t v, int lo, int hi) { return static_cast<int>(v < lo ? lo : v > hi ? hi : v); }

}  // namespace

int hjd_internal::warp_item_check(const WarpRecord& it, int index, int out_format)
{
    const int rc = item_common_check("warp", it, index, out_format);
    if (rc) return rc;
    if (it.flags & ~hjd::kWarpReplicate)
        return set_error(HJD_E_INVALID, "warp item %d: unknown flag bits 0x%x (bit 0: HJD_WARP_REPLICATE)", index,
                         static_cast<unsigned>(it.flags & ~hjd::kWarpReplicate));
    if (it.fill > 0xFFFFFFu)
        return set_error(HJD_E_INVALID, "warp item %d: fill 0x%x is above 0xFFFFFF (0x00RRGGBB)", index, it.fill);
    if (it.reserved) return set_error(HJD_E_INVALID, "warp item %d: reserved must be 0", index);
    return HJD_OK;
}

int hjd_internal::warp_roi(int width, int height, const int32_t m[6], int out_w, int out_h, ::hjd_rect* out)
{
    if (width < 1 || height < 1) return set_error(HJD_E_INVALID, "warp roi: frame size %d x %d", width, height);
    if (!dim_ok(out_w) || !dim_ok(out_h))
        return set_error(HJD_E_INVALID, "warp roi: output size %d x %d is outside 1..%d", out_w, out_h, kResizeMaxDim);
    // X and Y are affine in (j, i): their extrema lie at the four output corners
    int64_t lo[2], hi[2];
    for (int a = 0; a < 2; ++a) {
        const int64_t mj = m[3 * a], mi = m[3 * a + 1], t = m[3 * a + 2];
        const int64_t dj = mj * (out_w - 1), di = mi * (out_h - 1);
        lo[a] = t + std::min<int64_t>(dj, 0) + std::min<int64_t>(di, 0);
        hi[a] = t + std::max<int64_t>(dj, 0) + std::max<int64_t>(di, 0);
    }
    // every tap's column lies in floor(Xmin) .. floor(Xmax) + 1; clamped into the frame
    const int x_lo = clamp_int(floor_q16(lo[0]), 0, width - 1), x_hi = clamp_int(floor_q16(hi[0]) + 1, 0, width - 1);
    const int y_lo = clamp_int(floor_q16(lo[1]), 0, height - 1), y_hi = clamp_int(floor_q16(hi[1]) + 1, 0, height - 1);
    *out = {x_lo, y_lo, x_hi - x_lo + 1, y_hi - y_lo + 1};
    return HJD_OK;
}

int hjd_internal::warp_orient(const int32_t m[6], int stored_w, int stored_h, int orientation, int32_t out[6])
{
    if (stored_w < 1 || stored_h < 1)
        return set_error(HJD_E_INVALID, "warp orient: stored size %d x %d", stored_w, stored_h);
    if (!orientation_ok(orientation))
        return set_error(HJD_E_INVALID, "warp orient: orientation %d is outside 1..8", orientation);
    // The table of include/hjd.h as a map of positions: D[i][j] = S[row][col]
    // says where on S the displayed position (x = j, y = i) lies, (xs, ys) =
    //     1 (x, y)  2 (w-1-x, y)  3 (w-1-x, h-1-y)  4 (x, h-1-y)
    //     5 (y, x)  6 (y, h-1-x)  7 (w-1-y, h-1-x)  8 (w-1-y, x)
    const bool tr = orientation_transposes(orientation);
    const bool neg_xs = (0x18Cu >> orientation) & 1u;   // xs = w - 1 - (.) : 2 3 7 8
    const bool neg_ys = (0x0D8u >> orientation) & 1u;   // ys = h - 1 - (.) : 3 4 6 7
    const int32_t* row_xs = tr ? m + 3 : m;             // the displayed coordinate xs is made of
    const int32_t* row_ys = tr ? m : m + 3;
    int64_t r[6];
    for (int k = 0; k < 3; ++k) {
        r[k] = neg_xs ? -static_cast<int64_t>(row_xs[k]) : row_xs[k];
        r[3 + k] = neg_ys ? -static_cast<int64_t>(row_ys[k]) : row_ys[k];
    }
    if (neg_xs) r[2] += static_cast<int64_t>(stored_w - 1) << 16;
    if (neg_ys) r[5] += static_cast<int64_t>(stored_h - 1) << 16;
    for (int k = 0; k < 6; ++k)
        if (r[k] < INT32_MIN || r[k] > INT32_MAX)
            return set_error(HJD_E_INVALID, "warp orient: composed entry m[%d] = %lld leaves int32", k,
                             static_cast<long long>(r[k]));
    for (int k = 0; k < 6; ++k) out[k] = static_cast<int32_t>(r[k]);
    return HJD_OK;
}

int hjd_internal::launch_warp(int device, const WarpRecord* d_items, int n, int out_w, int out_h, int out_pitch,
                              int out_format, const NormRecord& norm, void* stream, int tiled)
{
    return with_out_format("warp", out_format, [&](auto format) -> int {
        constexpr int kFormat = decltype(format)::value;
        HJD_HIP(hipSetDevice(device));
        const bool form = tiled < 0 ? hjd::kWarpTiled : tiled != 0;
        const int groups = groups_per_image(warp_units(out_w, out_h, form), hjd::kWarpThreads);
        const dim3 grid(static_cast<uint32_t>(n) * static_cast<uint32_t>(groups)), block(hjd::kWarpThreads);
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (form == hjd::kWarpTiled)
            hipLaunchKernelGGL(hjd::warp_kernel<kFormat>, grid, block, 0, s, d_items, groups, out_w, out_h, out_pitch, norm);
        else
            hipLaunchKernelGGL(hjd::warp_other_form_kernel<kFormat>, grid, block, 0, s, d_items, groups, out_w, out_h,
                               out_pitch, norm);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    });
}

extern "C" {

int hjd_warp_roi(int width, int height, const int32_t m[6], int out_w, int out_h, hjd_rect* out)
{
    if (!m || !out) return set_error(HJD_E_INVALID, "warp roi: m or out is NULL");
    return hjd_internal::warp_roi(width, height, m, out_w, out_h, out);
}

int hjd_warp_orient(const int32_t m[6], int stored_w, int stored_h, int orientation, int32_t out[6])
{
    if (!m || !out) return set_error(HJD_E_INVALID, "warp orient: m or out is NULL");
    return hjd_internal::warp_orient(m, stored_w, stored_h, orientation, out);
}

int hjd_warp_check(const hjd_warp_item* items, int n, int out_w, int out_h, int out_pitch, int out_format)
{
    if (!items) return set_error(HJD_E_INVALID, "warp: items is NULL");
    int rc = hjd_internal::resize_out_check(n, out_w, out_h, out_pitch, out_format);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        hjd_internal::WarpRecord r;
        memcpy(&r, &items[i], sizeof(r));
        rc = hjd_internal::warp_item_check(r, i, out_format);
        if (rc) return rc;
    }
    return HJD_OK;
}

int hjd_warp_create(hjd_ctx* ctx, const hjd_warp_item* items, int n, int out_w, int out_h, int out_pitch, int out_format,
                    hjd_warp** out)
{
    if (!ctx || !out) return set_error(HJD_E_INVALID, "warp: ctx or out is NULL");
    *out = nullptr;
    int rc = hjd_warp_check(items, n, out_w, out_h, out_pitch, out_format);
    if (rc) return rc;
    hjd_warp* w = new (std::nothrow) hjd_warp(ctx, n, out_format);
    if (!w) return set_error(HJD_E_NOMEM, "warp allocation");
    w->out_w = out_w;
    w->out_h = out_h;
    w->out_pitch = out_pitch;
    rc = w->upload("warp", items, static_cast<size_t>(n));   // (hjd_warp_item is the kernel's record)
    if (rc) {
        delete w;
        return rc;
    }
    *out = w;
    return HJD_OK;
}

int hjd_warp_set_normalize(hjd_warp* w, const float a[3], const float b[3])
{
    return hjd_internal::table_set_normalize("warp", w, a, b);
}

int hjd_warp_launch(hjd_warp* w, void* stream)
{
    if (!w) return set_error(HJD_E_INVALID, "warp is NULL");
    return hjd_internal::launch_warp(w->device, w->d_items, w->n, w->out_w, w->out_h, w->out_pitch, w->out_format,
                                     w->norm, stream);
}

int hjd_debug_warp_launch_form(hjd_warp* w, int tiled, void* stream)
{
    if (!w) return set_error(HJD_E_INVALID, "warp is NULL");
    if (tiled != 0 && tiled != 1)
        return set_error(HJD_E_INVALID, "hjd_debug_warp_launch_form: form %d is neither 0 (row-major) nor 1 (tiled)", tiled);
    return hjd_internal::launch_warp(w->device, w->d_items, w->n, w->out_w, w->out_h, w->out_pitch, w->out_format,
                                     w->norm, stream, tiled);
}

int hjd_warp_destroy(hjd_warp* w)
{
    delete w;   // (its destructor frees the table)
    return HJD_OK;
}

}  // extern "C"
