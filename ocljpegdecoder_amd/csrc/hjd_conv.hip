// hjd_conv.hip -- the filter object of include/hjd.h (hjd_conv_*), its host
// reference (hjd_conv_apply_host) and the launch of hjd::conv_kernel.
// DESIGN.md s3.15.
#include "hjd_conv.hpp"

#include <cstring>
#include <vector>

#include "hjd_post.hpp"

using hjd_internal::set_error;

static_assert(sizeof(hjd_conv_item) == sizeof(hjd::ConvDev) && offsetof(hjd_conv_item, dst) == 8 &&
                  offsetof(hjd_conv_item, w) == 16 && offsetof(hjd_conv_item, dst_pitch) == 28 &&
                  offsetof(hjd_conv_item, filter) == offsetof(hjd::ConvDev, rx) && sizeof(hjd_conv_filter) == 120 &&
                  offsetof(hjd_conv_item, filter) + offsetof(hjd_conv_filter, border) == offsetof(hjd::ConvDev, border) &&
                  offsetof(hjd_conv_item, filter) + offsetof(hjd_conv_filter, a) == offsetof(hjd::ConvDev, a) &&
                  offsetof(hjd_conv_item, filter) + offsetof(hjd_conv_filter, reserved) ==
                      offsetof(hjd::ConvDev, tile_begin) &&
                  offsetof(hjd_conv_item, filter) + offsetof(hjd_conv_filter, kh) == offsetof(hjd::ConvDev, kh) &&
                  offsetof(hjd_conv_item, filter) + offsetof(hjd_conv_filter, kv) == offsetof(hjd::ConvDev, kv),
              "hjd_conv_item is the kernel's record");
static_assert(HJD_CONV_KEEP == 0 && HJD_CONV_REFLECT == 1 && HJD_CONV_REPLICATE == 2, "conv_src_index's borders");
static_assert(HJD_CONV_MAX_RADIUS == hjd::kConvMaxRadius && 2 * HJD_CONV_MAX_RADIUS + 1 < 24, "the taps of a row");
static_assert(hjd::kConvTileW == 64 && hjd::kConvTileH == 32, "conv_tiles counts 64 x 32 tiles");

struct hjd_conv : hjd_internal::StageTable<hjd::ConvDev> {
    using StageTable::StageTable;
    int64_t tiles = 0;
};

int hjd_internal::conv_out_check(int n, int out_format)
{
    if (n < 1 || n > kResizeMaxItems) return set_error(HJD_E_INVALID, "conv: n = %d is outside 1..%d", n, kResizeMaxItems);
    if (!out_format_planar(out_format))
        return set_error(HJD_E_INVALID, "conv: output format %d is not HJD_OUT_RGB_PLANAR, HJD_OUT_RGB_PLANAR_F16 or _F32",
                         out_format);
    return HJD_OK;
}

int hjd_internal::conv_filter_check(const ConvRecord& it, int index)
{
    if (it.rx < 0 || it.rx > HJD_CONV_MAX_RADIUS || it.ry < 0 || it.ry > HJD_CONV_MAX_RADIUS)
        return set_error(HJD_E_INVALID, "conv item %d: radius (%d, %d) is outside 0..%d", index, it.rx, it.ry,
                         HJD_CONV_MAX_RADIUS);
    if (it.border < HJD_CONV_KEEP || it.border > HJD_CONV_REPLICATE)
        return set_error(HJD_E_INVALID, "conv item %d: border %d is outside 0..2 (HJD_CONV_KEEP, _REFLECT, _REPLICATE)",
                         index, it.border);
    if (it.border == HJD_CONV_REFLECT && (it.rx >= it.w || it.ry >= it.h))
        return set_error(HJD_E_INVALID, "conv item %d: HJD_CONV_REFLECT needs radius (%d, %d) below the size %d x %d", index,
                         it.rx, it.ry, it.w, it.h);
    const struct {
        const char* name;
        const uint16_t* k;
        int r;
    } axes[2] = {{"kh", it.kh, it.rx}, {"kv", it.kv, it.ry}};
    for (const auto& ax : axes) {
        uint32_t sum = 0;
        for (int p = 0; p < 24; ++p) {
            if (p > 2 * ax.r && ax.k[p])
                return set_error(HJD_E_INVALID,
                                 "conv item %d: %s[%d] = %d lies beyond the %d taps of radius %d and must be 0", index, ax.name, p, ax.k[p], 2 * ax.r + 1, ax.r);
            sum += ax.k[p];
        }
        if (sum < 1 || sum > 4096)
            return set_error(HJD_E_INVALID, "conv item %d: the taps of %s sum to %u, outside 1..4096", index, ax.name, sum);
    }
    if (it.a < -HJD_CONV_MAX_GAIN || it.a > HJD_CONV_MAX_GAIN || it.b < -HJD_CONV_MAX_GAIN || it.b > HJD_CONV_MAX_GAIN)
        return set_error(HJD_E_INVALID, "conv item %d: gain a = %d or b = %d is outside +-%d (Q12)", index, it.a, it.b,
                         HJD_CONV_MAX_GAIN);
    return HJD_OK;
}

int hjd_internal::conv_item_check(const ConvRecord& it, int index, int out_format)
{
    int rc = item_common_check("conv", it, index, out_format);
    if (rc) return rc;
    const int elem = out_format_row_bytes(out_format);
    if (it.dst_pitch < elem * it.w || (it.dst_pitch & out_format_pitch_mask(out_format)))
        return set_error(HJD_E_INVALID,
                         "conv item %d: dst_pitch %d must be >= %d (%d bytes x the width %d) and a multiple of %d", index, it.dst_pitch, elem * it.w, elem, it.w, elem);
    if (it.dst == it.src) return set_error(HJD_E_INVALID, "conv item %d: dst == src (a filter cannot run in place)", index);
    return conv_filter_check(it, index);
}

int hjd_internal::launch_conv(int device, const ConvRecord* d_items, int n, int64_t tiles, int out_format,
                              const NormRecord& norm, void* stream)
{
    if (tiles < 1 || tiles > kConvMaxTiles)
        return set_error(HJD_E_INVALID, "conv: %lld tiles in one launch (at most %lld)", static_cast<long long>(tiles),
                         static_cast<long long>(kConvMaxTiles));
    return with_out_format("conv", out_format, [&](auto format) -> int {
        HJD_HIP(hipSetDevice(device));
        const dim3 grid(static_cast<uint32_t>(tiles)), block(hjd::kConvThreads);
        hipLaunchKernelGGL(hjd::conv_kernel<decltype(format)::value>, grid, block, 0, static_cast<hipStream_t>(stream),
                           d_items, n, norm);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    });
}

extern "C" {

int hjd_conv_check(const hjd_conv_item* items, int n, int out_format)
{
    if (!items) return set_error(HJD_E_INVALID, "conv: items is NULL");
    int rc = hjd_internal::conv_out_check(n, out_format);
    if (rc) return rc;
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        hjd_internal::ConvRecord r;
        memcpy(&r, &items[i], sizeof(r));
        rc = hjd_internal::conv_item_check(r, i, out_format);
        if (rc) return rc;
        if (items[i].filter.reserved) return set_error(HJD_E_INVALID, "conv item %d: reserved must be 0", i);
        tiles += hjd_internal::conv_tiles(r.w, r.h);
    }
    if (tiles > hjd_internal::kConvMaxTiles)
        return set_error(HJD_E_INVALID, "conv: the items have %lld tiles of 64 x 32 in all (at most %lld per launch)",
                         static_cast<long long>(tiles), static_cast<long long>(hjd_internal::kConvMaxTiles));
    return HJD_OK;
}

int hjd_conv_create(hjd_ctx* ctx, const hjd_conv_item* items, int n, int out_format, hjd_conv** out)
{
    if (!ctx || !out) return set_error(HJD_E_INVALID, "conv: ctx or out is NULL");
    *out = nullptr;
    int rc = hjd_conv_check(items, n, out_format);
    if (rc) return rc;
    hjd_conv* r = new (std::nothrow) hjd_conv(ctx, n, out_format);
    if (!r) return set_error(HJD_E_NOMEM, "conv allocation");
    std::vector<hjd::ConvDev> table(static_cast<size_t>(n));
    memcpy(table.data(), items, sizeof(hjd::ConvDev) * static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        table[i].tile_begin = static_cast<uint32_t>(r->tiles);
        r->tiles += hjd_internal::conv_tiles(table[i].w, table[i].h);
    }
    rc = r->upload("conv", table.data(), table.size());
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return HJD_OK;
}

int hjd_conv_set_normalize(hjd_conv* r, const float a[3], const float b[3])
{
    return hjd_internal::table_set_normalize("conv", r, a, b);
}

int hjd_conv_launch(hjd_conv* r, void* stream)
{
    if (!r) return set_error(HJD_E_INVALID, "conv is NULL");
    return hjd_internal::launch_conv(r->device, r->d_items, r->n, r->tiles, r->out_format, r->norm, stream);
}

int hjd_conv_destroy(hjd_conv* r)
{
    delete r;   // (its destructor frees the table)
    return HJD_OK;
}

int hjd_conv_apply_host(const uint8_t* src, int w, int h, int src_pitch, const hjd_conv_filter* f, uint8_t* dst,
                        int dst_pitch)
{
    if (!src || !dst || !f) return set_error(HJD_E_INVALID, "conv host: src, dst or the filter is NULL");
    if (!hjd_internal::dim_ok(w) || !hjd_internal::dim_ok(h) || src_pitch < w || dst_pitch < w)
        return set_error(HJD_E_INVALID, "conv host: size %d x %d (1..%d) with pitches %d and %d", w, h,
                         hjd_internal::kResizeMaxDim, src_pitch, dst_pitch);
    if (dst == src) return set_error(HJD_E_INVALID, "conv host: dst == src (a filter cannot run in place)");
    hjd_internal::ConvRecord it;
    memset(&it, 0, sizeof(it));
    it.w = w;
    it.h = h;
    memcpy(&it.rx, f, sizeof(*f));
    int rc = hjd_internal::conv_filter_check(it, 0);
    if (rc) return rc;
    if (f->reserved) return set_error(HJD_E_INVALID, "conv host: reserved must be 0");
    const int rx = it.rx, ry = it.ry;
    // the row sums of every source row (up to 1 GiB: no exception may leave an extern "C" function)
    const size_t nrows = static_cast<size_t>(w) * static_cast<size_t>(h);
    uint32_t* rows = new (std::nothrow) uint32_t[nrows];
    if (!rows) return set_error(HJD_E_NOMEM, "conv host: %zu bytes of row sums", nrows * sizeof(uint32_t));
    for (int c = 0; c < 3; ++c) {
        const uint8_t* sp = src + static_cast<size_t>(c) * static_cast<size_t>(src_pitch) * static_cast<size_t>(h);
        uint8_t* dp = dst + static_cast<size_t>(c) * static_cast<size_t>(dst_pitch) * static_cast<size_t>(h);
        for (int i = 0; i < h; ++i) {
            const uint8_t* row = sp + static_cast<size_t>(i) * static_cast<size_t>(src_pitch);
            for (int j = 0; j < w; ++j) {
                uint32_t s = 0;
                for (int p = -rx; p <= rx; ++p)
                    s += static_cast<uint32_t>(it.kh[p + rx]) * row[hjd::conv_src_index(j + p, w, it.border)];
                rows[static_cast<size_t>(i) * static_cast<size_t>(w) + static_cast<size_t>(j)] = s;
            }
        }
        for (int i = 0; i < h; ++i) {
            const uint8_t* row = sp + static_cast<size_t>(i) * static_cast<size_t>(src_pitch);
            uint8_t* out = dp + static_cast<size_t>(i) * static_cast<size_t>(dst_pitch);
            const bool band_y = i < ry || i >= h - ry;
            for (int j = 0; j < w; ++j) {
                if (it.border == HJD_CONV_KEEP && (band_y || j < rx || j >= w - rx)) {
                    out[j] = row[j];
                    continue;
                }
                uint32_t S = 0;
                for (int q = -ry; q <= ry; ++q)
                    S += static_cast<uint32_t>(it.kv[q + ry]) *
                         rows[static_cast<size_t>(hjd::conv_src_index(i + q, h, it.border)) * static_cast<size_t>(w) +
                              static_cast<size_t>(j)];
                out[j] = static_cast<uint8_t>(hjd::conv_finish(it.a, it.b, row[j], S));
            }
        }
    }
    delete[] rows;
    return HJD_OK;
}

}  // extern "C"
