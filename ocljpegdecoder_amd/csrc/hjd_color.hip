// hjd_color.hip -- the colour object of include/hjd.h (hjd_color_*) and the
// launches of hjd::color_sum_kernel and hjd::color_kernel, which the GPU
// decoder's colour calls (hjd_gdec_post.hip) share.  DESIGN.md s3.13.
#include "hjd_color.hpp"

#include <cstring>
#include <vector>

#include "hjd_post.hpp"

using hjd_internal::set_error;

static_assert(sizeof(hjd_color_item) == sizeof(hjd::ColorDev) && offsetof(hjd_color_item, dst) == 8 &&
                  offsetof(hjd_color_item, w) == 16 && offsetof(hjd_color_item, dst_pitch) == 28 &&
                  offsetof(hjd_color_item, m) == 32 && offsetof(hjd_color_item, p) == 68 &&
                  offsetof(hjd_color_item, t) == 104 && offsetof(hjd_color_item, reserved) == 116,
              "hjd_color_item is the kernel's record");
static_assert(hjd::kColorMaxGroups == hjd_internal::kMaxGroups &&
                  hjd_internal::color_sums_bytes(1) == hjd::kColorMaxGroups * 3 * sizeof(uint32_t),
              "the table of sums has a row per group");
static_assert(HJD_COLOR_MAX_COEF == 32767 && HJD_COLOR_MAX_OFFSET == (1 << 23), "the bounds of the 24-bit multiplies");

struct hjd_color : hjd_internal::StageTable<hjd::ColorDev> {
    using StageTable::StageTable;
    ~hjd_color() { release(d_sums); }
    int groups = 1;                // per image: the largest image's
    bool sums = false;             // some record reads its image's sums
    uint32_t* d_sums = nullptr;    // then: [n][kMaxGroups][3], which every launch of this object shares
};

int hjd_internal::color_out_check(int n, int out_format)
{
    if (n < 1 || n > kResizeMaxItems)
        return set_error(HJD_E_INVALID, "color: n = %d is outside 1..%d", n, kResizeMaxItems);
    if (!out_format_planar(out_format))
        return set_error(HJD_E_INVALID,
                         "color: output format %d is not HJD_OUT_RGB_PLANAR, HJD_OUT_RGB_PLANAR_F16 or _F32", out_format);
    return HJD_OK;
}

int hjd_internal::color_coef_check(const int32_t m[9], const int32_t p[9], const int32_t t[3], int index,
                                   bool* uses_sums)
{
    bool any = false;
    for (int k = 0; k < 18; ++k) {
        const int32_t v = k < 9 ? m[k] : p[k - 9];
        if (v < -HJD_COLOR_MAX_COEF || v > HJD_COLOR_MAX_COEF)
            return set_error(HJD_E_INVALID, "color item %d: %s[%d] = %d is outside -%d..%d (Q12)", index, k < 9 ? "m" : "p",
                             k % 9, v, HJD_COLOR_MAX_COEF, HJD_COLOR_MAX_COEF);
        any = any || (k >= 9 && v != 0);
    }
    for (int k = 0; k < 3; ++k)
        if (t[k] < -HJD_COLOR_MAX_OFFSET || t[k] > HJD_COLOR_MAX_OFFSET)
            return set_error(HJD_E_INVALID, "color item %d: t[%d] = %d is outside -2^23..2^23 (Q12 grey levels)", index, k,
                             t[k]);
    if (uses_sums) *uses_sums = any;
    return HJD_OK;
}

int hjd_internal::color_item_check(const ColorRecord& it, int index, int out_format)
{
    int rc = item_common_check("color", it, index, out_format);
    if (rc) return rc;
    const int elem = out_format_row_bytes(out_format);
    if (it.dst_pitch < elem * it.w || (it.dst_pitch & out_format_pitch_mask(out_format)))
        return set_error(HJD_E_INVALID, "color item %d: dst_pitch %d must be >= %d (%d bytes x the width %d) and a multiple of %d",
                         index, it.dst_pitch, elem * it.w, elem, it.w, elem);
    return color_coef_check(it.m, it.p, it.t, index, nullptr);
}

int hjd_internal::color_groups(int w, int h)
{
    return groups_per_image(static_cast<int64_t>((w + 3) / 4) * h, hjd::kColorThreads);
}

int hjd_internal::launch_color(int device, const ColorRecord* d_items, int n, int groups, uint32_t* d_sums, int out_format,
                               const NormRecord& norm, void* stream)
{
    if (groups < 1 || groups > kMaxGroups)
        return set_error(HJD_E_INVALID, "color: %d groups per image (1..%d)", groups, kMaxGroups);
    return with_out_format("color", out_format, [&](auto format) -> int {
        HJD_HIP(hipSetDevice(device));
        const dim3 grid(static_cast<uint32_t>(n) * static_cast<uint32_t>(groups)), block(hjd::kColorThreads);
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (d_sums) {
            hipLaunchKernelGGL(hjd::color_sum_kernel, grid, block, 0, s, d_items, groups, d_sums);
            HJD_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(hjd::color_kernel<decltype(format)::value>, grid, block, 0, s, d_items, groups,
                           static_cast<const uint32_t*>(d_sums), norm);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    });
}

extern "C" {

int hjd_color_check(const hjd_color_item* items, int n, int out_format)
{
    if (!items) return set_error(HJD_E_INVALID, "color: items is NULL");
    int rc = hjd_internal::color_out_check(n, out_format);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        hjd_internal::ColorRecord r;
        memcpy(&r, &items[i], sizeof(r));
        rc = hjd_internal::color_item_check(r, i, out_format);
        if (rc) return rc;
        if (items[i].reserved) return set_error(HJD_E_INVALID, "color item %d: reserved must be 0", i);
    }
    return HJD_OK;
}

int hjd_color_create(hjd_ctx* ctx, const hjd_color_item* items, int n, int out_format, hjd_color** out)
{
    if (!ctx || !out) return set_error(HJD_E_INVALID, "color: ctx or out is NULL");
    *out = nullptr;
    int rc = hjd_color_check(items, n, out_format);
    if (rc) return rc;
    hjd_color* r = new (std::nothrow) hjd_color(ctx, n, out_format);
    if (!r) return set_error(HJD_E_NOMEM, "color allocation");
    std::vector<hjd::ColorDev> table(static_cast<size_t>(n));
    memcpy(table.data(), items, sizeof(hjd::ColorDev) * static_cast<size_t>(n));
    for (hjd::ColorDev& rec : table) {
        bool uses = false;
        (void)hjd_internal::color_coef_check(rec.m, rec.p, rec.t, 0, &uses);
        rec.use_sums = uses ? 1 : 0;
        r->sums = r->sums || uses;
        const int g = hjd_internal::color_groups(rec.w, rec.h);
        r->groups = g > r->groups ? g : r->groups;
    }
    const size_t sums_bytes = r->sums ? hjd_internal::color_sums_bytes(n) : 0;
    hipError_t e = hipSetDevice(r->device);
    if (r->sums) {
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->d_sums), sums_bytes);
        if (e != hipSuccess) r->d_sums = nullptr;
    }
    rc = r->upload("color", table.data(), table.size(), e, " and sums (" + std::to_string(sums_bytes) + " bytes)");
    if (rc) {
        delete r;   // (frees whichever of the two it holds)
        return rc;
    }
    *out = r;
    return HJD_OK;
}

int hjd_color_set_normalize(hjd_color* r, const float a[3], const float b[3])
{
    return hjd_internal::table_set_normalize("color", r, a, b);
}

int hjd_color_launch(hjd_color* r, void* stream)
{
    if (!r) return set_error(HJD_E_INVALID, "color is NULL");
    return hjd_internal::launch_color(r->device, r->d_items, r->n, r->groups, r->d_sums, r->out_format, r->norm, stream);
}

int hjd_color_destroy(hjd_color* r)
{
    delete r;   // (its destructors free the table and the sums)
    return HJD_OK;
}

}  // extern "C"
