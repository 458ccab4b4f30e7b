// hjd_resize.hip -- the resize object of include/hjd.h (hjd_resize_*) and the
// launches of hjd::resize_kernel (bilinear) and of hjd::resize_aa_h_kernel /
// resize_aa_v_kernel (the antialiased filter), which the GPU decoder's resized
// decode (hjd_gdec_post.hip) shares.  DESIGN.md s3.9, s3.10.
#include "hjd_resize.hpp"
#include "hjd_resize_aa.hpp"

#include <cstring>
#include <vector>

#include "hjd_post.hpp"

using hjd_internal::set_error;

static_assert(sizeof(hjd_resize_item) == sizeof(hjd::ResizeDev) && offsetof(hjd_resize_item, dst) == 8 &&
                  offsetof(hjd_resize_item, src_w) == 16 && offsetof(hjd_resize_item, flags) == 28,
              "hjd_resize_item is the kernel's record");

// d_items, filter 1: n horizontal records, then n vertical ones
struct hjd_resize : hjd_internal::StageTable<hjd::ResizeDev> {
    using StageTable::StageTable;
    ~hjd_resize() { release(d_mid); }
    int out_w = 0, out_h = 0, out_pitch = 0;
    int filter = HJD_RESIZE_BILINEAR;
    int max_src_h = 0;                    // filter 1: sizes the horizontal launch
    uint8_t* d_mid = nullptr;             // filter 1: the intermediate every launch of this object shares
};

// Groups per image of a launch over rows of out_w / 4 quads, one quad per thread.
static int resize_groups(int out_w, int rows)
{
    return hjd_internal::groups_per_image(static_cast<int64_t>((out_w + 3) / 4) * rows, hjd::kResizeThreads);
}

int hjd_internal::resize_out_check(int n, int out_w, int out_h, int out_pitch, int out_format)
{
    if (n < 1 || n > kResizeMaxItems)
        return set_error(HJD_E_INVALID, "resize: n = %d is outside 1..%d", n, kResizeMaxItems);
    if (!out_format_planar(out_format))
        return set_error(HJD_E_INVALID,
                         "resize: output format %d is not HJD_OUT_RGB_PLANAR, HJD_OUT_RGB_PLANAR_F16 or _F32", out_format);
    if (!dim_ok(out_w) || !dim_ok(out_h))
        return set_error(HJD_E_INVALID, "resize: output size %d x %d is outside 1..%d", out_w, out_h, kResizeMaxDim);
    const int elem = out_format_row_bytes(out_format);
    if (out_pitch < elem * out_w || (out_pitch & out_format_pitch_mask(out_format)))
        return set_error(HJD_E_INVALID, "resize: out_pitch %d must be >= %d (%d bytes x out_w) and a multiple of %d",
                         out_pitch, elem * out_w, elem, elem);
    return HJD_OK;
}

int hjd_internal::resize_item_check(const ResizeRecord& it, int index, int out_format)
{
    const int rc = item_common_check("resize", it, index, out_format);
    if (rc) return rc;
    if (it.flags & ~hjd::kResizeFlipH)
        return set_error(HJD_E_INVALID, "resize item %d: unknown flag bits 0x%x (bit 0: horizontal flip)", index,
                         static_cast<unsigned>(it.flags & ~hjd::kResizeFlipH));
    return HJD_OK;
}

int hjd_internal::resize_filter_check(int filter)
{
    if (filter != HJD_RESIZE_BILINEAR && filter != HJD_RESIZE_TRIANGLE_AA)
        return set_error(HJD_E_INVALID, "resize: filter %d is neither HJD_RESIZE_BILINEAR (0) nor HJD_RESIZE_TRIANGLE_AA (1)",
                         filter);
    return HJD_OK;
}

int hjd_internal::resize_aa_ratio_check(int src_w, int src_h, int out_w, int out_h, int index)
{
    constexpr int64_t kRatio = int64_t{1} << 21;   // 255.5 * T < 2^31 (include/hjd.h)
    if (static_cast<int64_t>(src_w) * src_w > kRatio * out_w)
        return set_error(HJD_E_INVALID,
                         "resize item %d: src_w %d -> out_w %d: the antialiased filter takes src_w^2 <= 2^21 * out_w", index,
                         src_w, out_w);
    if (static_cast<int64_t>(src_h) * src_h > kRatio * out_h)
        return set_error(HJD_E_INVALID,
                         "resize item %d: src_h %d -> out_h %d: the antialiased filter takes src_h^2 <= 2^21 * out_h", index,
                         src_h, out_h);
    return HJD_OK;
}

int hjd_internal::launch_resize(int device, const ResizeRecord* d_items, int n, int out_w, int out_h, int out_pitch,
                                int out_format, const NormRecord& norm, void* stream)
{
    return with_out_format("resize", out_format, [&](auto format) -> int {
        HJD_HIP(hipSetDevice(device));
        const int groups = resize_groups(out_w, out_h);
        const dim3 grid(static_cast<uint32_t>(n) * static_cast<uint32_t>(groups)), block(hjd::kResizeThreads);
        hipLaunchKernelGGL(hjd::resize_kernel<decltype(format)::value>, grid, block, 0, static_cast<hipStream_t>(stream),
                           d_items, groups, out_w, out_h, out_pitch, norm);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    });
}

int hjd_internal::launch_resize_aa(int device, const ResizeRecord* d_h, const ResizeRecord* d_v, int n, int max_src_h,
                                   int out_w, int out_h, int out_pitch, int out_format, const NormRecord& norm,
                                   void* stream, int passes)
{
    return with_out_format("resize", out_format, [&](auto format) -> int {
        HJD_HIP(hipSetDevice(device));
        // horizontal: an image's quads are its src_h rows of out_w / 4; every image gets the largest one's groups
        const int hgroups = resize_groups(out_w, max_src_h), vgroups = resize_groups(out_w, out_h);
        const dim3 hgrid(static_cast<uint32_t>(n) * static_cast<uint32_t>(hgroups)),
            vgrid(static_cast<uint32_t>(n) * static_cast<uint32_t>(vgroups)), block(hjd::kResizeThreads);
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (passes & 1) {
            hipLaunchKernelGGL(hjd::resize_aa_h_kernel, hgrid, block, 0, s, d_h, hgroups, out_w);
            HJD_HIP(hipGetLastError());
        }
        if (!(passes & 2)) return HJD_OK;
        hipLaunchKernelGGL(hjd::resize_aa_v_kernel<decltype(format)::value>, vgrid, block, 0, s, d_v, vgroups, out_w, out_h,
                           out_pitch, norm);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    });
}

extern "C" {

int hjd_resize_check_filter(const hjd_resize_item* items, int n, int out_w, int out_h, int out_pitch, int out_format,
                            int filter)
{
    if (!items) return set_error(HJD_E_INVALID, "resize: items is NULL");
    int rc = hjd_internal::resize_filter_check(filter);
    if (rc) return rc;
    rc = hjd_internal::resize_out_check(n, out_w, out_h, out_pitch, out_format);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        hjd_internal::ResizeRecord r;
        memcpy(&r, &items[i], sizeof(r));
        rc = hjd_internal::resize_item_check(r, i, out_format);
        if (rc) return rc;
        if (filter == HJD_RESIZE_TRIANGLE_AA) {
            rc = hjd_internal::resize_aa_ratio_check(r.w, r.h, out_w, out_h, i);
            if (rc) return rc;
        }
    }
    return HJD_OK;
}

int hjd_resize_check(const hjd_resize_item* items, int n, int out_w, int out_h, int out_pitch, int out_format)
{
    return hjd_resize_check_filter(items, n, out_w, out_h, out_pitch, out_format, HJD_RESIZE_BILINEAR);
}

int hjd_resize_create_filter(hjd_ctx* ctx, const hjd_resize_item* items, int n, int out_w, int out_h, int out_pitch,
                             int out_format, int filter, hjd_resize** out)
{
    if (!ctx || !out) return set_error(HJD_E_INVALID, "resize: ctx or out is NULL");
    *out = nullptr;
    int rc = hjd_resize_check_filter(items, n, out_w, out_h, out_pitch, out_format, filter);
    if (rc) return rc;
    hjd_resize* r = new (std::nothrow) hjd_resize(ctx, n, out_format);
    if (!r) return set_error(HJD_E_NOMEM, "resize allocation");
    r->out_w = out_w;
    r->out_h = out_h;
    r->out_pitch = out_pitch;
    r->filter = filter;
    const bool aa = filter == HJD_RESIZE_TRIANGLE_AA;
    // the table: the items as they are; for the antialiased filter the
    // horizontal records (dst: the item's intermediate), then the vertical ones
    std::vector<hjd::ResizeDev> table(static_cast<size_t>(n) * (aa ? 2 : 1));
    memcpy(table.data(), items, sizeof(hjd::ResizeDev) * static_cast<size_t>(n));
    size_t mid_bytes = 0;
    hipError_t e = hipSetDevice(r->device);
    if (aa) {
        for (int i = 0; i < n; ++i) {
            mid_bytes += hjd_internal::resize_aa_item_bytes(out_w, table[i].h);
            r->max_src_h = table[i].h > r->max_src_h ? table[i].h : r->max_src_h;
        }
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->d_mid), mid_bytes);
        if (e != hipSuccess) r->d_mid = nullptr;
        size_t off = 0;
        for (int i = 0; i < n && e == hipSuccess; ++i) {
            hjd::ResizeDev& hrec = table[i];
            hjd::ResizeDev& vrec = table[static_cast<size_t>(n) + i];
            vrec.src = r->d_mid + off;
            vrec.dst = hrec.dst;
            vrec.w = out_w;
            vrec.h = hrec.h;
            vrec.pitch = hjd_internal::resize_aa_pitch(out_w);
            vrec.flags = 0;   // (the flip is the horizontal pass's)
            hrec.dst = r->d_mid + off;
            off += hjd_internal::resize_aa_item_bytes(out_w, hrec.h);
        }
    }
    rc = r->upload("resize", table.data(), table.size(), e, " and intermediate (" + std::to_string(mid_bytes) + " bytes)");
    if (rc) {
        delete r;   // (frees whichever of the two it holds)
        return rc;
    }
    *out = r;
    return HJD_OK;
}

int hjd_resize_create(hjd_ctx* ctx, const hjd_resize_item* items, int n, int out_w, int out_h, int out_pitch,
                      int out_format, hjd_resize** out)
{
    return hjd_resize_create_filter(ctx, items, n, out_w, out_h, out_pitch, out_format, HJD_RESIZE_BILINEAR, out);
}

int hjd_resize_set_normalize(hjd_resize* r, const float a[3], const float b[3])
{
    return hjd_internal::table_set_normalize("resize", r, a, b);
}

static int launch_aa_object(hjd_resize* r, void* stream, int passes)
{
    return hjd_internal::launch_resize_aa(r->device, r->d_items, r->d_items + r->n, r->n, r->max_src_h, r->out_w, r->out_h,
                                          r->out_pitch, r->out_format, r->norm, stream, passes);
}

int hjd_debug_resize_launch_pass(hjd_resize* r, int pass, void* stream)
{
    if (!r) return set_error(HJD_E_INVALID, "resize is NULL");
    if (r->filter != HJD_RESIZE_TRIANGLE_AA || (pass != 0 && pass != 1))
        return set_error(HJD_E_INVALID, "hjd_debug_resize_launch_pass: pass %d of a filter-%d object", pass, r->filter);
    return launch_aa_object(r, stream, 1 << pass);
}

int hjd_resize_launch(hjd_resize* r, void* stream)
{
    if (!r) return set_error(HJD_E_INVALID, "resize is NULL");
    if (r->filter == HJD_RESIZE_TRIANGLE_AA) return launch_aa_object(r, stream, 3);
    return hjd_internal::launch_resize(r->device, r->d_items, r->n, r->out_w, r->out_h, r->out_pitch, r->out_format,
                                       r->norm, stream);
}

int hjd_resize_destroy(hjd_resize* r)
{
    delete r;   // (its destructors free the table and the intermediate)
    return HJD_OK;
}

}  // extern "C"
