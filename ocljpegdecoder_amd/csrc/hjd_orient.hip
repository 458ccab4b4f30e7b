// hjd_orient.hip -- the orientation object of include/hjd.h (hjd_orient_*), the
// display-to-stored rectangle mapping (hjd_orient_roi) and the launch of
// hjd::orient_kernel, which the GPU decoder's oriented decodes (hjd_gdec_post.hip)
// share.  DESIGN.md s3.11.
#include "hjd_orient.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

#include "hjd_post.hpp"

using hjd_internal::set_error;

static_assert(sizeof(hjd_orient_item) == sizeof(hjd::OrientDev) && offsetof(hjd_orient_item, dst) == 8 &&
                  offsetof(hjd_orient_item, src_w) == 16 && offsetof(hjd_orient_item, orientation) == 28 &&
                  offsetof(hjd_orient_item, dst_pitch) == 32 && offsetof(hjd_orient_item, reserved) == 36,
              "hjd_orient_item is the kernel's record");
static_assert(hjd::kOrientTile == 128, "orient_tiles counts 128 x 128 tiles");

struct hjd_orient : hjd_internal::StageTable<hjd::OrientDev> {
    using StageTable::StageTable;
    int64_t tiles = 0;
};

namespace {

// An address range of one item: its source (dst false) or its output.
struct Span {
    uintptr_t begin, end;
    bool dst;
    int item;
};

}  // namespace

int hjd_internal::orient_out_check(int n, int out_format)
{
    if (n < 1 || n > kResizeMaxItems)
        return set_error(HJD_E_INVALID, "orient: n = %d is outside 1..%d", n, kResizeMaxItems);
    if (!out_format_planar(out_format))
        return set_error(HJD_E_INVALID,
                         "orient: output format %d is not HJD_OUT_RGB_PLANAR, HJD_OUT_RGB_PLANAR_F16 or _F32", out_format);
    return HJD_OK;
}

int hjd_internal::orient_item_check(const OrientRecord& it, int index, int out_format)
{
    const int rc = item_common_check("orient", it, index, out_format);
    if (rc) return rc;
    if (!orientation_ok(it.orientation))
        return set_error(HJD_E_INVALID, "orient item %d: orientation %d is outside 1..8", index, it.orientation);
    const int out_w = orientation_transposes(it.orientation) ? it.h : it.w, elem = out_format_row_bytes(out_format);
    if (it.dst_pitch < elem * out_w || (it.dst_pitch & out_format_pitch_mask(out_format)))
        return set_error(HJD_E_INVALID,
                         "orient item %d: dst_pitch %d must be >= %d (%d bytes x the oriented width %d) and a multiple of %d",
                         index, it.dst_pitch, elem * out_w, elem, out_w, elem);
    return HJD_OK;
}

int hjd_internal::orient_roi(int width, int height, int orientation, const ::hjd_rect& d, ::hjd_rect* stored)
{
    if (width < 1 || height < 1)
        return set_error(HJD_E_INVALID, "orient roi: stored size %d x %d", width, height);
    if (!orientation_ok(orientation))
        return set_error(HJD_E_INVALID, "orient roi: orientation %d is outside 1..8", orientation);
    const bool tr = orientation_transposes(orientation);
    const int dw = tr ? height : width, dh = tr ? width : height;
    if (d.x < 0 || d.y < 0 || d.w < 1 || d.h < 1 || d.w > dw - d.x || d.h > dh - d.y)
        return set_error(HJD_E_INVALID, "orient roi: roi (%d, %d, %d x %d) is outside the %d x %d oriented image", d.x, d.y,
                         d.w, d.h, dw, dh);
    const int W = width, H = height;
    switch (orientation) {   // from the table of include/hjd.h
    case 1: *stored = {d.x, d.y, d.w, d.h}; break;
    case 2: *stored = {W - d.x - d.w, d.y, d.w, d.h}; break;
    case 3: *stored = {W - d.x - d.w, H - d.y - d.h, d.w, d.h}; break;
    case 4: *stored = {d.x, H - d.y - d.h, d.w, d.h}; break;
    case 5: *stored = {d.y, d.x, d.h, d.w}; break;
    case 6: *stored = {d.y, H - d.x - d.w, d.h, d.w}; break;
    case 7: *stored = {W - d.y - d.h, H - d.x - d.w, d.h, d.w}; break;
    default: *stored = {W - d.y - d.h, d.x, d.h, d.w}; break;
    }
    return HJD_OK;
}

int hjd_internal::launch_orient(int device, const OrientRecord* d_items, int n, int64_t tiles, int out_format,
                                const NormRecord& norm, void* stream)
{
    if (tiles < 1 || tiles > kOrientMaxTiles)
        return set_error(HJD_E_INVALID, "orient: %lld tiles in one launch (at most %lld)", static_cast<long long>(tiles),
                         static_cast<long long>(kOrientMaxTiles));
    return with_out_format("orient", out_format, [&](auto format) -> int {
        HJD_HIP(hipSetDevice(device));
        const dim3 grid(static_cast<uint32_t>(tiles)), block(hjd::kOrientThreads);
        hipLaunchKernelGGL(hjd::orient_kernel<decltype(format)::value>, grid, block, 0, static_cast<hipStream_t>(stream),
                           d_items, n, norm);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    });
}

extern "C" {

int hjd_orient_roi(int width, int height, int orientation, const hjd_rect* display, hjd_rect* stored)
{
    if (!display || !stored) return set_error(HJD_E_INVALID, "orient roi: display or stored is NULL");
    return hjd_internal::orient_roi(width, height, orientation, *display, stored);
}

int hjd_orient_check(const hjd_orient_item* items, int n, int out_format)
{
    if (!items) return set_error(HJD_E_INVALID, "orient: items is NULL");
    int rc = hjd_internal::orient_out_check(n, out_format);
    if (rc) return rc;
    const int elem = hjd_internal::out_format_row_bytes(out_format);
    int64_t tiles = 0;
    std::vector<Span> spans;
    spans.reserve(2 * static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        hjd_internal::OrientRecord r;
        memcpy(&r, &items[i], sizeof(r));
        rc = hjd_internal::orient_item_check(r, i, out_format);
        if (rc) return rc;
        if (items[i].reserved)
            return set_error(HJD_E_INVALID, "orient item %d: reserved must be 0", i);
        tiles += hjd_internal::orient_tiles(r.w, r.h);
        const bool tr = hjd_internal::orientation_transposes(r.orientation);
        const uintptr_t ow = static_cast<uintptr_t>(tr ? r.h : r.w), oh = static_cast<uintptr_t>(tr ? r.w : r.h);
        const uintptr_t s = reinterpret_cast<uintptr_t>(r.src), d = reinterpret_cast<uintptr_t>(r.dst);
        // (the last row of the last plane ends with its last pixel, not its pitch)
        spans.push_back({s, s + (3 * static_cast<uintptr_t>(r.h) - 1) * static_cast<uintptr_t>(r.pitch) +
                                static_cast<uintptr_t>(r.w), false, i});
        spans.push_back({d, d + (3 * oh - 1) * static_cast<uintptr_t>(r.dst_pitch) + ow * static_cast<uintptr_t>(elem),
                         true, i});
    }
    if (tiles > hjd_internal::kOrientMaxTiles)
        return set_error(HJD_E_INVALID, "orient: the items have %lld tiles of 128 x 128 in all (at most %lld per launch)",
                         static_cast<long long>(tiles), static_cast<long long>(hjd_internal::kOrientMaxTiles));
    // an output may overlap nothing, a source only other sources: one sweep in address order
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
    uintptr_t end_any = 0, end_dst = 0;
    int by_any = -1, by_dst = -1;
    for (const Span& sp : spans) {
        if (sp.dst ? sp.begin < end_any : sp.begin < end_dst)
            return set_error(HJD_E_INVALID, "orient item %d: its %s overlaps item %d's %s", sp.item,
                             sp.dst ? "output" : "source", sp.dst ? by_any : by_dst,
                             sp.dst ? "source or output" : "output");
        if (sp.end > end_any) {
            end_any = sp.end;
            by_any = sp.item;
        }
        if (sp.dst && sp.end > end_dst) {
            end_dst = sp.end;
            by_dst = sp.item;
        }
    }
    return HJD_OK;
}

int hjd_orient_create(hjd_ctx* ctx, const hjd_orient_item* items, int n, int out_format, hjd_orient** out)
{
    if (!ctx || !out) return set_error(HJD_E_INVALID, "orient: ctx or out is NULL");
    *out = nullptr;
    int rc = hjd_orient_check(items, n, out_format);
    if (rc) return rc;
    hjd_orient* r = new (std::nothrow) hjd_orient(ctx, n, out_format);
    if (!r) return set_error(HJD_E_NOMEM, "orient allocation");
    std::vector<hjd::OrientDev> table(static_cast<size_t>(n));
    memcpy(table.data(), items, sizeof(hjd::OrientDev) * static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        table[i].tile_begin = static_cast<uint32_t>(r->tiles);
        r->tiles += hjd_internal::orient_tiles(table[i].w, table[i].h);
    }
    rc = r->upload("orient", table.data(), table.size());
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return HJD_OK;
}

int hjd_orient_set_normalize(hjd_orient* r, const float a[3], const float b[3])
{
    return hjd_internal::table_set_normalize("orient", r, a, b);
}

int hjd_orient_launch(hjd_orient* r, void* stream)
{
    if (!r) return set_error(HJD_E_INVALID, "orient is NULL");
    return hjd_internal::launch_orient(r->device, r->d_items, r->n, r->tiles, r->out_format, r->norm, stream);
}

int hjd_orient_destroy(hjd_orient* r)
{
    delete r;   // (its destructor frees the table)
    return HJD_OK;
}

}  // extern "C"
