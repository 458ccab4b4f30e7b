// hjd_tone.hip -- the tone object of include/hjd.h (hjd_tone_*) and the
// launches of hjd::tone_hist_kernel, hjd::tone_lut_kernel and hjd::tone_kernel,
// which the GPU decoder's tone calls (hjd_gdec_post.hip) share.  DESIGN.md s3.14.
#include "hjd_tone.hpp"

#include <cstring>
#include <vector>

#include "hjd_post.hpp"

using hjd_internal::set_error;

static_assert(sizeof(hjd_tone_item) == sizeof(hjd::ToneDev) && offsetof(hjd_tone_item, dst) == 8 &&
                  offsetof(hjd_tone_item, w) == 16 && offsetof(hjd_tone_item, dst_pitch) == 28 &&
                  offsetof(hjd_tone_item, curve) == offsetof(hjd::ToneDev, mode) &&
                  offsetof(hjd_tone_item, curve) + offsetof(hjd_tone_curve, lut) == offsetof(hjd::ToneDev, lut) &&
                  sizeof(hjd_tone_curve) == 776,
              "hjd_tone_item is the kernel's record");
static_assert(hjd_internal::tone_hist_bytes(1) == hjd::kToneHistGroups * 768 * sizeof(uint32_t) &&
                  hjd_internal::tone_luts_bytes(1) == 768,
              "the table of partial histograms has a row per group, the table of curves one per image");
static_assert(HJD_TONE_TABLE == 0 && HJD_TONE_AUTOCONTRAST == 1 && HJD_TONE_EQUALIZE == 2, "tone_data_curve's modes");

struct hjd_tone : hjd_internal::StageTable<hjd::ToneDev> {
    using StageTable::StageTable;
    ~hjd_tone()
    {
        release(d_hist);
        release(d_luts);
    }
    int groups = 1;                // per image: the largest image's
    uint32_t* d_hist = nullptr;    // some record's mode is not 0: [n][kToneHistGroups][3][256], and
    uint8_t* d_luts = nullptr;     // [n][3][256], which every launch of this object shares
};

int hjd_internal::tone_out_check(int n, int out_format)
{
    if (n < 1 || n > kResizeMaxItems) return set_error(HJD_E_INVALID, "tone: n = %d is outside 1..%d", n, kResizeMaxItems);
    if (!out_format_planar(out_format))
        return set_error(HJD_E_INVALID, "tone: output format %d is not HJD_OUT_RGB_PLANAR, HJD_OUT_RGB_PLANAR_F16 or _F32",
                         out_format);
    return HJD_OK;
}

int hjd_internal::tone_curve_check(int32_t mode, int32_t reserved, int index)
{
    if (mode < HJD_TONE_TABLE || mode > HJD_TONE_EQUALIZE)
        return set_error(HJD_E_INVALID, "tone item %d: mode %d is outside 0..2 (HJD_TONE_TABLE, _AUTOCONTRAST, _EQUALIZE)",
                         index, mode);
    if (reserved) return set_error(HJD_E_INVALID, "tone item %d: reserved must be 0", index);
    return HJD_OK;
}

int hjd_internal::tone_item_check(const ToneRecord& it, int index, int out_format)
{
    int rc = item_common_check("tone", it, index, out_format);
    if (rc) return rc;
    const int elem = out_format_row_bytes(out_format);
    if (it.dst_pitch < elem * it.w || (it.dst_pitch & out_format_pitch_mask(out_format)))
        return set_error(HJD_E_INVALID, "tone item %d: dst_pitch %d must be >= %d (%d bytes x the width %d) and a multiple of %d",
                         index, it.dst_pitch, elem * it.w, elem, it.w, elem);
    return tone_curve_check(it.mode, it.reserved, index);
}

int hjd_internal::launch_tone(int device, const ToneRecord* d_items, int n, int groups, uint32_t* d_hist, uint8_t* d_luts,
                              int out_format, const NormRecord& norm, void* stream)
{
    if (groups < 1 || groups > kMaxGroups)
        return set_error(HJD_E_INVALID, "tone: %d groups per image (1..%d)", groups, kMaxGroups);
    if ((d_hist == nullptr) != (d_luts == nullptr))
        return set_error(HJD_E_INVALID, "tone: the tables of histograms and of curves go together");
    return with_out_format("tone", out_format, [&](auto format) -> int {
        HJD_HIP(hipSetDevice(device));
        const dim3 block(hjd::kToneThreads);
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (d_hist) {
            const int hgroups = groups < hjd::kToneHistGroups ? groups : hjd::kToneHistGroups;
            hipLaunchKernelGGL(hjd::tone_hist_kernel, dim3(static_cast<uint32_t>(n) * static_cast<uint32_t>(hgroups)), block,
                               0, s, d_items, hgroups, d_hist);
            HJD_HIP(hipGetLastError());
            hipLaunchKernelGGL(hjd::tone_lut_kernel, dim3(static_cast<uint32_t>(n)), dim3(hjd::kToneLutThreads), 0, s,
                               d_items, hgroups, static_cast<const uint32_t*>(d_hist), d_luts);
            HJD_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(hjd::tone_kernel<decltype(format)::value>,
                           dim3(static_cast<uint32_t>(n) * static_cast<uint32_t>(groups)), block, 0, s, d_items, groups,
                           static_cast<const uint8_t*>(d_luts), norm);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    });
}

extern "C" {

int hjd_tone_check(const hjd_tone_item* items, int n, int out_format)
{
    if (!items) return set_error(HJD_E_INVALID, "tone: items is NULL");
    int rc = hjd_internal::tone_out_check(n, out_format);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        // (the record without its table: the checks do not read it)
        hjd_internal::ToneRecord r;
        memcpy(&r, &items[i], offsetof(hjd::ToneDev, lut));
        rc = hjd_internal::tone_item_check(r, i, out_format);
        if (rc) return rc;
    }
    return HJD_OK;
}

int hjd_tone_create(hjd_ctx* ctx, const hjd_tone_item* items, int n, int out_format, hjd_tone** out)
{
    if (!ctx || !out) return set_error(HJD_E_INVALID, "tone: ctx or out is NULL");
    *out = nullptr;
    int rc = hjd_tone_check(items, n, out_format);
    if (rc) return rc;
    hjd_tone* r = new (std::nothrow) hjd_tone(ctx, n, out_format);
    if (!r) return set_error(HJD_E_NOMEM, "tone allocation");
    bool data = false;   // some record's mode is not 0
    for (int i = 0; i < n; ++i) {
        data = data || items[i].curve.mode != HJD_TONE_TABLE;
        const int g = hjd_internal::color_groups(items[i].w, items[i].h);
        r->groups = g > r->groups ? g : r->groups;
    }
    const size_t hist_bytes = data ? hjd_internal::tone_hist_bytes(n) : 0, luts_bytes = data ? hjd_internal::tone_luts_bytes(n) : 0;
    hipError_t e = hipSetDevice(r->device);
    if (data) {
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->d_hist), hist_bytes);
        if (e != hipSuccess) r->d_hist = nullptr;
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->d_luts), luts_bytes);
        if (e != hipSuccess) r->d_luts = nullptr;
    }
    // (hjd_tone_item is the record: uploaded as it stands)
    rc = r->upload("tone", items, static_cast<size_t>(n), e,
                   " and histograms and curves (" + std::to_string(hist_bytes + luts_bytes) + " bytes)");
    if (rc) {
        delete r;   // (frees whichever of the three it holds)
        return rc;
    }
    *out = r;
    return HJD_OK;
}

int hjd_tone_set_normalize(hjd_tone* r, const float a[3], const float b[3])
{
    return hjd_internal::table_set_normalize("tone", r, a, b);
}

int hjd_tone_launch(hjd_tone* r, void* stream)
{
    if (!r) return set_error(HJD_E_INVALID, "tone is NULL");
    return hjd_internal::launch_tone(r->device, r->d_items, r->n, r->groups, r->d_hist, r->d_luts, r->out_format, r->norm,
                                     stream);
}

int hjd_tone_destroy(hjd_tone* r)
{
    delete r;   // (its destructors free the table, the histograms and the curves)
    return HJD_OK;
}

int hjd_tone_curve_from_histogram(int mode, const uint32_t hist[3][256], const uint8_t lut_in[3][256], uint8_t lut_out[3][256])
{
    if (!hist || !lut_out) return set_error(HJD_E_INVALID, "tone curve: hist or lut_out is NULL");
    if (mode < HJD_TONE_TABLE || mode > HJD_TONE_EQUALIZE) return set_error(HJD_E_INVALID, "tone curve: mode %d is outside 0..2", mode);
    uint8_t composed[3][256];   // (lut_out may be lut_in)
    for (int c = 0; c < 3; ++c) {
        uint64_t n = 0;
        uint32_t lo = 256, hi = 0;
        for (uint32_t v = 0; v < 256; ++v) {
            n += hist[c][v];
            if (hist[c][v]) {
                lo = lo == 256 ? v : lo;
                hi = v;
            }
        }
        if (n > (1u << 28))
            return set_error(HJD_E_INVALID, "tone curve: channel %d counts %llu pixels (at most 2^28)", c,
                             static_cast<unsigned long long>(n));
        const uint32_t last = hist[c][hi];
        uint32_t below = 0;
        for (uint32_t v = 0; v < 256; ++v) {
            const uint32_t d = hjd::tone_data_curve(mode, v, below, lo, hi, last, static_cast<uint32_t>(n));
            composed[c][v] = lut_in ? lut_in[c][d] : static_cast<uint8_t>(d);
            below += hist[c][v];
        }
    }
    memcpy(lut_out, composed, sizeof(composed));
    return HJD_OK;
}

}  // extern "C"
