// hjd_gdec_post.hip -- the decoder calls with stages behind the pixel kernels
// (include/hjd_host.h hjd_gdec_decode_oriented, _resized*, _warped*; DESIGN.md
// s10).  Each entry point admits its frames (admit_frame), lays out the
// scratch (Region) and states its stages as one PostPlan, which gdec_issue
// writes and launches through post_write_records and post_launch.  Everything
// that can refuse a call is checked before anything is staged, allocated or enqueued.
#include "hjd_gdec.hpp"

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>

#include "hjd_host.h"

using hjd_internal::ColorRecord;
using hjd_internal::ConvRecord;
using hjd_internal::OrientRecord;
using hjd_internal::ResizeRecord;
using hjd_internal::set_error;
using hjd_internal::ToneRecord;
using hjd_internal::WarpRecord;
using namespace hjd::ent;

namespace {

// One region of a call's scratch, an image per frame: laid out while the
// frames are admitted, placed once the scratch is large enough.
struct Region {
    std::vector<void*> ptrs;   // null until grow_scratch places the region
    std::vector<size_t> offs;   // from the region's start
    std::vector<int32_t> pitches;
    std::vector<hjd_rect> dims;
    size_t need = 0;
    explicit Region(size_t n) : ptrs(n), offs(n), pitches(n), dims(n) {}
    // Image i, planar w x rows: 16-byte aligned, its pitch rounded up to 4
    // (whole strips of the pixel kernel keep their vector stores).
    void add(int i, int w, int rows)
    {
        pitches[i] = (w + 3) & ~3;
        dims[i].w = w;
        dims[i].h = rows;
        offs[i] = need;
        need = hjd_internal::align_up(need + 3 * static_cast<size_t>(pitches[i]) * static_cast<size_t>(rows), 16);
    }
    // All of the region's images as one planar batch of w x rows: the pitch rounded up to 4, image i
    // at i * 3 * pitch * rows (what batch_record computes from the first), the whole 16-byte aligned.
    void add_batch(int w, int rows)
    {
        const size_t image = 3 * static_cast<size_t>((w + 3) & ~3) * static_cast<size_t>(rows);
        for (size_t i = 0; i < ptrs.size(); ++i) {
            pitches[i] = (w + 3) & ~3;
            dims[i] = hjd_rect{0, 0, w, rows};
            offs[i] = need + image * i;
        }
        need = hjd_internal::align_up(need + image * ptrs.size(), 16);
    }
    // One array of `bytes` bytes (a region of one "image" nobody reads as one).
    void add_bytes(size_t bytes)
    {
        offs[0] = need;
        need = hjd_internal::align_up(need + bytes, 16);
    }
    PostImages images() const { return PostImages{ptrs.data(), pitches.data(), dims.data()}; }
};

// Grow the decoder's scratch to hold the regions, one behind the other, and
// place them (grow-only; the previous call may still use the old buffer, so
// growing waits for it).
int grow_scratch(hjd_gdec* g, std::initializer_list<Region*> regions, const char* what)
{
    size_t need = 0;
    for (const Region* r : regions) need += r->need;
    if (need > g->crops_bytes) {
        HJD_HIP(hipSetDevice(g->device));
        if (g->pending) HJD_HIP(hipEventSynchronize(g->done));
        g->release(g->d_crops);
        g->d_crops = nullptr;
        g->crops_bytes = 0;
        if (g->alloc(g->d_crops, need)) {
            (void)hipGetLastError();
            return set_error(HJD_E_NOMEM, "the %s of this call need %zu bytes of device memory", what, need);
        }
        g->crops_bytes = need;
    }
    uint8_t* base = g->d_crops;
    for (Region* r : regions) {
        for (size_t i = 0; i < r->ptrs.size(); ++i) r->ptrs[i] = base + r->offs[i];
        base += r->need;
    }
    return HJD_OK;
}

// The plan's next stage, its records at the next 16-byte aligned offset behind plan.recs_bytes.
PostStage& add_stage(PostPlan& plan, PostKind kind, const PostImages& in, int out_format, size_t recs_bytes)
{
    PostStage& s = plan.stage[plan.nstages++];
    s = PostStage{};
    s.kind = kind;
    s.in = in;
    s.out_format = out_format;
    s.recs_off = hjd_internal::align_up(plan.recs_bytes, 16);
    s.recs_bytes = recs_bytes;
    plan.recs_bytes = s.recs_off + recs_bytes;
    return s;
}

// Stage and issue the call: the pixel kernels write `crops`, the plan's stages follow.
int run_post(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, void* stream, const Region& crops,
             bool rects, const PostPlan& plan)
{
    GdecCall c(datas, sizes, n, stream);
    c.d_outs = crops.ptrs.data();
    c.pitches = crops.pitches.data();
    c.rois = rects ? crops.dims.data() : nullptr;
    c.post = &plan;
    return gdec_run(g, c);
}

// The orient kernel's records: image i from s.in to s.out, its tiles behind image i - 1's (the
// running count is each record's tile_begin; the launch takes s.tiles).
int write_orient_records(const PostStage& s, int n, OrientRecord* recs)
{
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        const OrientRecord rec{s.in.ptrs[i],    s.out.ptrs[i],     s.in.dims[i].w,   s.in.dims[i].h,
                               s.in.pitches[i], s.orientations[i], s.out.pitches[i], static_cast<uint32_t>(tiles)};
        const int rc = hjd_internal::orient_item_check(rec, i, s.out_format);
        if (rc) return rc;
        tiles += hjd_internal::orient_tiles(rec.w, rec.h);
        recs[i] = rec;
    }
    return HJD_OK;
}

// What a resize or warp record begins with: image i from s.in to its place in the batch.
template <class Rec>
Rec batch_record(const PostStage& s, int i)
{
    Rec rec;
    rec.src = s.in.ptrs[i];
    rec.dst = static_cast<uint8_t*>(s.batch.ptr) +
              3 * static_cast<size_t>(s.batch.pitch) * static_cast<size_t>(s.batch.h) * static_cast<size_t>(i);
    rec.w = s.in.dims[i].w;
    rec.h = s.in.dims[i].h;
    rec.pitch = s.in.pitches[i];
    rec.flags = s.flags ? s.flags[i] : 0;
    return rec;
}

// The resize kernel's records -- with the antialiased filter n more, the vertical
// launch's, image i then going by way of its intermediate s.mids[i].
int write_resize_records(const PostStage& s, int n, ResizeRecord* recs)
{
    for (int i = 0; i < n; ++i) {
        const ResizeRecord rec = batch_record<ResizeRecord>(s, i);
        const int rc = hjd_internal::resize_item_check(rec, i, s.out_format);
        if (rc) return rc;
        recs[i] = rec;
        if (s.kind == PostKind::resize_aa) {
            // (the flip is the horizontal pass's)
            recs[n + i] = ResizeRecord{s.mids[i], rec.dst, s.batch.w, rec.h, hjd_internal::resize_aa_pitch(s.batch.w), 0};
            recs[i].dst = s.mids[i];
        }
    }
    return HJD_OK;
}

// The warp kernel's records: image i through s.mats[i].
int write_warp_records(const PostStage& s, int n, WarpRecord* recs)
{
    for (int i = 0; i < n; ++i) {
        WarpRecord rec = batch_record<WarpRecord>(s, i);
        memcpy(rec.m, s.mats[i], sizeof(rec.m));
        rec.fill = s.fills ? s.fills[i] : 0;
        rec.reserved = 0;
        const int rc = hjd_internal::warp_item_check(rec, i, s.out_format);
        if (rc) return rc;
        recs[i] = rec;
    }
    return HJD_OK;
}

// The colour kernels' records: image i of the batch s.in (the resize's or warp's planar bytes in
// the scratch) through s.colors[i] to its place in the caller's batch.
int write_color_records(const PostStage& s, int n, ColorRecord* recs)
{
    for (int i = 0; i < n; ++i) {
        ColorRecord rec;
        rec.src = s.in.ptrs[i];
        rec.dst = static_cast<uint8_t*>(s.batch.ptr) +
                  3 * static_cast<size_t>(s.batch.pitch) * static_cast<size_t>(s.batch.h) * static_cast<size_t>(i);
        rec.w = s.batch.w;
        rec.h = s.batch.h;
        rec.pitch = s.in.pitches[i];
        rec.dst_pitch = s.batch.pitch;
        const int32_t* c = s.colors[i];   // m[9], p[9], t[3]
        memcpy(rec.m, c, sizeof(rec.m));
        memcpy(rec.p, c + 9, sizeof(rec.p));
        memcpy(rec.t, c + 18, sizeof(rec.t));
        bool uses = false;
        int rc = hjd_internal::color_coef_check(c, c + 9, c + 18, i, &uses);
        rec.use_sums = uses ? 1 : 0;
        if (!rc) rc = hjd_internal::color_item_check(rec, i, s.out_format);
        if (rc) return rc;
        recs[i] = rec;
    }
    return HJD_OK;
}

// The filter kernel's records: image i of the batch s.in (planar bytes in the scratch: the resize's,
// the warp's, or the colour stage's in their place) through s.convs[i] to its place in s.batch (the
// caller's, or with a tone stage behind a second batch in the scratch), its tiles behind image i - 1's.
int write_conv_records(const PostStage& s, int n, ConvRecord* recs)
{
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        ConvRecord rec;
        rec.src = s.in.ptrs[i];
        rec.dst = static_cast<uint8_t*>(s.batch.ptr) +
                  3 * static_cast<size_t>(s.batch.pitch) * static_cast<size_t>(s.batch.h) * static_cast<size_t>(i);
        rec.w = s.batch.w;
        rec.h = s.batch.h;
        rec.pitch = s.in.pitches[i];
        rec.dst_pitch = s.batch.pitch;
        static_assert(sizeof(hjd_conv_filter) == sizeof(ConvRecord) - offsetof(ConvRecord, rx),
                      "the filter is the record's tail");
        memcpy(&rec.rx, &s.convs[i], sizeof(hjd_conv_filter));
        rec.tile_begin = static_cast<uint32_t>(tiles);   // (the filter's reserved word, 0: convs_check)
        const int rc = hjd_internal::conv_item_check(rec, i, s.out_format);
        if (rc) return rc;
        tiles += hjd_internal::conv_tiles(rec.w, rec.h);
        recs[i] = rec;
    }
    return HJD_OK;
}

// The tone kernels' records: image i of the batch s.in (planar bytes in the scratch: the resize's,
// the warp's, the colour stage's in their place, or the filter stage's) through s.tones[i] to its place in the
// caller's batch.
int write_tone_records(const PostStage& s, int n, ToneRecord* recs)
{
    for (int i = 0; i < n; ++i) {
        ToneRecord& rec = recs[i];   // (written in place: a record is 808 bytes)
        rec.src = s.in.ptrs[i];
        rec.dst = static_cast<uint8_t*>(s.batch.ptr) +
                  3 * static_cast<size_t>(s.batch.pitch) * static_cast<size_t>(s.batch.h) * static_cast<size_t>(i);
        rec.w = s.batch.w;
        rec.h = s.batch.h;
        rec.pitch = s.in.pitches[i];
        rec.dst_pitch = s.batch.pitch;
        rec.mode = s.tones[i].mode;
        rec.reserved = s.tones[i].reserved;
        memcpy(rec.lut, s.tones[i].lut, sizeof(rec.lut));
        const int rc = hjd_internal::tone_item_check(rec, i, s.out_format);
        if (rc) return rc;
    }
    return HJD_OK;
}

}  // namespace

int hjd::ent::post_write_records(hjd_gdec* g, const PostPlan& plan, int n)
{
    for (int k = 0; k < plan.nstages; ++k) {
        const PostStage& s = plan.stage[k];
        void* recs = g->st.h_stage + g->st.H.recs + s.recs_off;
        int rc = HJD_OK;
        switch (s.kind) {
        case PostKind::orient: rc = write_orient_records(s, n, static_cast<OrientRecord*>(recs)); break;
        case PostKind::resize:
        case PostKind::resize_aa: rc = write_resize_records(s, n, static_cast<ResizeRecord*>(recs)); break;
        case PostKind::warp: rc = write_warp_records(s, n, static_cast<WarpRecord*>(recs)); break;
        case PostKind::color: rc = write_color_records(s, n, static_cast<ColorRecord*>(recs)); break;
        case PostKind::conv: rc = write_conv_records(s, n, static_cast<ConvRecord*>(recs)); break;
        case PostKind::tone: rc = write_tone_records(s, n, static_cast<ToneRecord*>(recs)); break;
        }
        if (rc) return rc;
    }
    return HJD_OK;
}

int hjd::ent::post_launch(hjd_gdec* g, const PostPlan& plan, int n, hipStream_t stream)
{
    for (int k = 0; k < plan.nstages; ++k) {
        const PostStage& s = plan.stage[k];
        const void* recs = g->d_blob + g->st.H.recs + s.recs_off;
        const ResizeRecord* rr = static_cast<const ResizeRecord*>(recs);
        int rc = HJD_OK;
        switch (s.kind) {
        case PostKind::orient:
            rc = hjd_internal::launch_orient(g->device, static_cast<const OrientRecord*>(recs), n, s.tiles,
                                             s.out_format, g->norm, stream);
            break;
        case PostKind::resize:
            rc = hjd_internal::launch_resize(g->device, rr, n, s.batch.w, s.batch.h, s.batch.pitch, s.out_format, g->norm,
                                             stream);
            break;
        case PostKind::resize_aa:
            rc = hjd_internal::launch_resize_aa(g->device, rr, rr + n, n, s.max_h, s.batch.w, s.batch.h, s.batch.pitch,
                                                s.out_format, g->norm, stream);
            break;
        case PostKind::warp:
            rc = hjd_internal::launch_warp(g->device, static_cast<const WarpRecord*>(recs), n, s.batch.w,
                                           s.batch.h, s.batch.pitch, s.out_format, g->norm, stream);
            break;
        case PostKind::color:
            rc = hjd_internal::launch_color(g->device, static_cast<const ColorRecord*>(recs), n,
                                            hjd_internal::color_groups(s.batch.w, s.batch.h), s.sums, s.out_format,
                                            g->norm, stream);
            break;
        case PostKind::conv:
            rc = hjd_internal::launch_conv(g->device, static_cast<const ConvRecord*>(recs), n,
                                           n * hjd_internal::conv_tiles(s.batch.w, s.batch.h), s.out_format, g->norm,
                                           stream);
            break;
        case PostKind::tone:
            rc = hjd_internal::launch_tone(g->device, static_cast<const ToneRecord*>(recs), n,
                                           hjd_internal::color_groups(s.batch.w, s.batch.h), s.hist, s.luts, s.out_format,
                                           g->norm, stream);
            break;
        }
        if (rc) return rc;
    }
    return HJD_OK;
}

namespace {

// HJD_OK if every orientation lies in 1..8; *any says whether one is not 1.
int orientations_check(const int32_t* orientations, int n, bool* any)
{
    *any = false;
    for (int i = 0; i < n; ++i) {
        if (!hjd_internal::orientation_ok(orientations[i]))
            return set_error(HJD_E_INVALID, "frame %d: orientation %d is outside 1..8", i, orientations[i]);
        *any = *any || orientations[i] != 1;
    }
    return HJD_OK;
}

// CropMapFn of an oriented call with rois (ctx: its orientations): the display
// rectangle mapped to the stored one.
int orient_map(const void* ctx, int i, int sw, int sh, const hjd_rect* roi, hjd_rect* crop)
{
    return hjd_internal::orient_roi(sw, sh, static_cast<const int32_t*>(ctx)[i], *roi, crop);
}

// CropMapFn of a warped call: the matrix on the stored image (mats[i]: m[i]
// with the orientation composed) and the rectangle it reads.
struct WarpMap {
    const int32_t (*m)[6];
    const int32_t* orientations;   // or null
    int out_w, out_h;
    int32_t (*mats)[6];
};
int warp_map(const void* ctx, int i, int sw, int sh, const hjd_rect*, hjd_rect* crop)
{
    const WarpMap& m = *static_cast<const WarpMap*>(ctx);
    const int rc = hjd_internal::warp_orient(m.m[i], sw, sh, m.orientations ? m.orientations[i] : 1, m.mats[i]);
    return rc ? rc : hjd_internal::warp_roi(sw, sh, m.mats[i], m.out_w, m.out_h, crop);
}

constexpr char kCapOriented[] = "frame %d: the crop is %d x %d, the orientation and the resize take up to %d";
constexpr char kCapResized[] = "frame %d: the crop is %d x %d, the resize takes up to %d";
constexpr char kCapWarped[] = "frame %d: the warp reads a %d x %d crop, it takes up to %d";

int tiles_check(int64_t tiles)
{
    if (tiles > hjd_internal::kOrientMaxTiles)
        return set_error(HJD_E_INVALID, "the crops have %lld tiles of 128 x 128 in all (at most %lld per call)",
                         static_cast<long long>(tiles), static_cast<long long>(hjd_internal::kOrientMaxTiles));
    return HJD_OK;
}

// The colour records of a call: HJD_OK if every one is legal (else the refusal names the frame).
// *any: one is not the identity (else the call is the one without colours); *sums: one reads its
// image's sums.  n has passed the call's own check.
int colors_check(const int32_t (*colors)[21], int n, bool* any, bool* sums)
{
    static const int32_t kIdentity[21] = {4096, 0, 0, 0, 4096, 0, 0, 0, 4096};
    *any = *sums = false;
    for (int i = 0; i < n; ++i) {
        bool uses = false;
        const int rc = hjd_internal::color_coef_check(colors[i], colors[i] + 9, colors[i] + 18, i, &uses);
        if (rc) return set_error(rc, "frame %d: %s", i, std::string(hjd_last_error()).c_str());
        *sums = *sums || uses;
        *any = *any || memcmp(colors[i], kIdentity, sizeof(kIdentity)) != 0;
    }
    return HJD_OK;
}

// The tone curves of a call: HJD_OK if every one is legal (else the refusal names the frame).
// *any: one is not mode 0 with the identity table (else the call is the one without tones);
// *data: one's mode is not 0, so the call takes histograms.  n has passed the call's own check.
int tones_check(const hjd_tone_curve* tones, int n, bool* any, bool* data)
{
    *any = *data = false;
    for (int i = 0; i < n; ++i) {
        const int rc = hjd_internal::tone_curve_check(tones[i].mode, tones[i].reserved, i);
        if (rc) return set_error(rc, "frame %d: %s", i, std::string(hjd_last_error()).c_str());
        *data = *data || tones[i].mode != HJD_TONE_TABLE;
        bool identity = tones[i].mode == HJD_TONE_TABLE;
        for (int k = 0; identity && k < 768; ++k) identity = tones[i].lut[k >> 8][k & 255] == (k & 255);
        *any = *any || !identity;
    }
    return HJD_OK;
}

// The filters of a call, for its batch of out_w x out_h images: HJD_OK if every one is legal (else the
// refusal names the frame) and their tiles fit a launch.  *any: one is not the identity record (else
// the call is the one without filters).  n has passed the call's own check.
int convs_check(const hjd_conv_filter* convs, int n, int out_w, int out_h, bool* any)
{
    *any = false;
    for (int i = 0; i < n; ++i) {
        ConvRecord rec;
        memset(&rec, 0, sizeof(rec));
        rec.w = out_w;
        rec.h = out_h;
        memcpy(&rec.rx, &convs[i], sizeof(hjd_conv_filter));
        int rc = hjd_internal::conv_filter_check(rec, i);
        if (!rc && convs[i].reserved) rc = set_error(HJD_E_INVALID, "conv item %d: reserved must be 0", i);
        if (rc) return set_error(rc, "frame %d: %s", i, std::string(hjd_last_error()).c_str());
        *any = *any || !hjd_internal::conv_is_identity(rec);
    }
    const int64_t tiles = n * hjd_internal::conv_tiles(out_w, out_h);
    if (*any && tiles > hjd_internal::kConvMaxTiles)
        return set_error(HJD_E_INVALID, "the batch has %lld tiles of 64 x 32 in all (at most %lld per call)",
                         static_cast<long long>(tiles), static_cast<long long>(hjd_internal::kConvMaxTiles));
    return HJD_OK;
}

// The scratch of a call's colour, filter and tone stages: `mid`, the batch the resize or warp writes in
// their place (planar bytes; a colour stage with another behind it runs on it in place); `mid2`, a
// second batch of that layout, which the filter stage writes where a tone stage follows (a filter
// cannot run in place); `sums`, the colour stage's table of partial sums where a record reads them;
// `hist` and `luts`, the tone stage's partial histograms and composed curves where a mode is not 0.
struct ColorScratch {
    Region mid, mid2, sums, hist, luts;
    ColorScratch(bool colors, bool color_sums, bool convs, bool tones, bool tone_data, int n, int out_w, int out_h)
        : mid(colors || convs || tones ? static_cast<size_t>(n) : 0), mid2(convs && tones ? static_cast<size_t>(n) : 0),
          sums(colors && color_sums ? 1 : 0), hist(tones && tone_data ? 1 : 0), luts(tones && tone_data ? 1 : 0)
    {
        if (colors || convs || tones) mid.add_batch(out_w, out_h);
        if (convs && tones) mid2.add_batch(out_w, out_h);
        if (colors && color_sums) sums.add_bytes(hjd_internal::color_sums_bytes(n));
        if (tones && tone_data) {
            hist.add_bytes(hjd_internal::tone_hist_bytes(n));
            luts.add_bytes(hjd_internal::tone_luts_bytes(n));
        }
    }
};

// Put the colour stage behind `last`, the plan's resize or warp stage, which wrote the caller's batch
// in the decoder's format: it now writes planar bytes into c.mid, and the colour stage that batch.
void add_color_stage(PostPlan& plan, PostStage& last, const ColorScratch& c, const int32_t (*colors)[21], int out_format,
                     int n)
{
    const auto batch = last.batch;
    last.out_format = HJD_OUT_RGB_PLANAR;
    last.batch = {c.mid.ptrs[0], batch.w, batch.h, c.mid.pitches[0]};
    PostStage& s = add_stage(plan, PostKind::color, c.mid.images(), out_format, sizeof(ColorRecord) * static_cast<size_t>(n));
    s.batch = batch;
    s.colors = colors;
    s.sums = c.sums.ptrs.empty() ? nullptr : static_cast<uint32_t*>(c.sums.ptrs[0]);
}

// Put the filter stage behind `last`, the plan's resize, warp or colour stage, which wrote the caller's
// batch in the decoder's format: it now writes planar bytes into c.mid (a colour stage, which reads
// c.mid, then runs in place), and the filter stage that batch.
void add_conv_stage(PostPlan& plan, PostStage& last, const ColorScratch& c, const hjd_conv_filter* convs, int out_format,
                    int n)
{
    const auto batch = last.batch;
    last.out_format = HJD_OUT_RGB_PLANAR;
    last.batch = {c.mid.ptrs[0], batch.w, batch.h, c.mid.pitches[0]};
    PostStage& s = add_stage(plan, PostKind::conv, c.mid.images(), out_format, sizeof(ConvRecord) * static_cast<size_t>(n));
    s.batch = batch;
    s.convs = convs;
}

// Put the tone stage behind `last`, the plan's resize, warp, colour or filter stage, which wrote the
// caller's batch in the decoder's format: it now writes planar bytes into `via` -- c.mid (a colour
// stage, which reads c.mid, then runs in place), or behind a filter stage, which reads c.mid, c.mid2
// -- and the tone stage that batch.
void add_tone_stage(PostPlan& plan, PostStage& last, const ColorScratch& c, const hjd_tone_curve* tones, int out_format,
                    int n)
{
    const Region& via = last.kind == PostKind::conv ? c.mid2 : c.mid;
    const auto batch = last.batch;
    last.out_format = HJD_OUT_RGB_PLANAR;
    last.batch = {via.ptrs[0], batch.w, batch.h, via.pitches[0]};
    PostStage& s = add_stage(plan, PostKind::tone, via.images(), out_format, sizeof(ToneRecord) * static_cast<size_t>(n));
    s.batch = batch;
    s.tones = tones;
    s.hist = c.hist.ptrs.empty() ? nullptr : static_cast<uint32_t*>(c.hist.ptrs[0]);
    s.luts = c.luts.ptrs.empty() ? nullptr : static_cast<uint8_t*>(c.luts.ptrs[0]);
}

// hjd_gdec_decode_resized_filter (orientations null), hjd_gdec_decode_resized_oriented,
// hjd_gdec_decode_resized_color (colors not null), hjd_gdec_decode_resized_tone (tones not null) and
// hjd_gdec_decode_resized_aug (any of colors, convs and tones): decode to the scratch, with
// orientations orient to a second scratch region, then the resize launches, then with colours the
// colour launches, then with filters the filter launch, then with tones the tone launches.
int decode_resized(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                   const int32_t* orientations, const int32_t* flags, const int32_t (*colors)[21],
                   const hjd_conv_filter* convs, const hjd_tone_curve* tones, void* d_out, int out_w, int out_h,
                   int32_t out_pitch, int filter, void* stream)
{
    if (!g || !datas || !sizes) return set_error(HJD_E_INVALID, "NULL argument");
    if (!d_out) return set_error(HJD_E_INVALID, "d_out is NULL");
    int rc = hjd_internal::resize_filter_check(filter);
    if (rc) return rc;
    const bool aa = filter == HJD_RESIZE_TRIANGLE_AA;
    rc = hjd_internal::resize_out_check(n, out_w, out_h, out_pitch, g->out_format);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & hjd_internal::out_format_align_mask(g->out_format))
        return set_error(HJD_E_INVALID, "d_out must be a multiple of the element size (%d bytes)",
                         hjd_internal::out_format_row_bytes(g->out_format));
    if (n > g->st.caps.max_frames)
        return set_error(HJD_E_INVALID, "batch of %d frames (capacity %d)", n, g->st.caps.max_frames);
    if (orientations) {
        bool any = false;
        rc = orientations_check(orientations, n, &any);
        if (rc) return rc;
        if (!any) orientations = nullptr;   // nothing to orient: the plain resized call
    }
    bool color_sums = false;
    if (colors) {
        bool any = false;
        rc = colors_check(colors, n, &any, &color_sums);
        if (rc) return rc;
        if (!any) colors = nullptr;   // every record the identity: the call without colours
    }
    if (convs) {
        bool any = false;
        rc = convs_check(convs, n, out_w, out_h, &any);
        if (rc) return rc;
        if (!any) convs = nullptr;   // every record the identity: the call without filters
    }
    bool tone_data = false;
    if (tones) {
        bool any = false;
        rc = tones_check(tones, n, &any, &tone_data);
        if (rc) return rc;
        if (!any) tones = nullptr;   // every curve the identity: the call without tones
    }
    // (the scratch: the crops, an oriented call's oriented crops, the antialiased filter's intermediates)
    const size_t un = static_cast<size_t>(n);
    Region crops(un), oriented(orientations ? un : 0), mids(aa ? un : 0);
    ColorScratch cs(colors != nullptr, color_sums, convs != nullptr, tones != nullptr, tone_data, n, out_w, out_h);
    const Admit admit{g->scale, false, orientations ? kCapOriented : kCapResized,
                      orientations && rois ? orient_map : nullptr, orientations};
    int64_t tiles = 0;
    int max_h = 1;
    for (int i = 0; i < n; ++i) {
        hjd_rect& crop = crops.dims[i];   // the stored crop
        rc = admit_frame(admit, datas[i], sizes[i], i, rois ? &rois[i] : nullptr, &crop);
        if (rc) return rc;
        if (flags && (flags[i] & ~1))
            return set_error(HJD_E_INVALID, "frame %d: unknown flag bits 0x%x (bit 0: horizontal flip)", i,
                             static_cast<unsigned>(flags[i] & ~1));
        // what the resize reads: the crop, or its oriented image
        const bool tr = orientations && hjd_internal::orientation_transposes(orientations[i]);
        const int rw = tr ? crop.h : crop.w, rh = tr ? crop.w : crop.h;
        if (aa) {
            rc = hjd_internal::resize_aa_ratio_check(rw, rh, out_w, out_h, i);
            if (rc) return set_error(rc, "frame %d: %s", i, std::string(hjd_last_error()).c_str());
            mids.add(i, out_w, rh);
            max_h = std::max(max_h, rh);
        }
        crops.add(i, crop.w, crop.h);
        if (orientations) {
            oriented.add(i, rw, rh);
            tiles += hjd_internal::orient_tiles(crop.w, crop.h);
        }
    }
    rc = tiles_check(tiles);
    if (rc) return rc;
    rc = grow_scratch(g, {&crops, &oriented, &mids, &cs.mid, &cs.mid2, &cs.sums, &cs.hist, &cs.luts},
                      aa ? "crops and the resize's intermediate" : "crops");
    if (rc) return rc;
    PostPlan plan{0, {}, pixel_tables_bytes(n, rois != nullptr, false)};   // the pixel kernels' tables: planar bytes
    PostImages in = crops.images();
    if (orientations) {
        PostStage& o = add_stage(plan, PostKind::orient, in, HJD_OUT_RGB_PLANAR, sizeof(OrientRecord) * un);
        o.out = in = oriented.images();
        o.orientations = orientations;
        o.tiles = tiles;
    }
    PostStage& r = add_stage(plan, aa ? PostKind::resize_aa : PostKind::resize, in, g->out_format,
                             sizeof(ResizeRecord) * un * (aa ? 2 : 1));
    r.batch = {d_out, out_w, out_h, out_pitch};
    r.flags = flags;
    r.mids = mids.ptrs.data();
    r.max_h = max_h;
    if (colors) add_color_stage(plan, r, cs, colors, g->out_format, n);
    if (convs) add_conv_stage(plan, plan.stage[plan.nstages - 1], cs, convs, g->out_format, n);
    if (tones) add_tone_stage(plan, plan.stage[plan.nstages - 1], cs, tones, g->out_format, n);
    return run_post(g, datas, sizes, n, stream, crops, rois != nullptr, plan);
}

// hjd_gdec_decode_warped (colors, convs and tones null), hjd_gdec_decode_warped_color, _tone and
// _aug: decode the rectangle each warp reads to the scratch, then the warp launch, then with colours
// the colour launches, then with filters the filter launch, then with tones the tone launches.
int decode_warped(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const int32_t (*m)[6],
                  const int32_t* orientations, const int32_t* flags, const uint32_t* fills, const int32_t (*colors)[21],
                  const hjd_conv_filter* convs, const hjd_tone_curve* tones, void* d_out, int out_w, int out_h,
                  int32_t out_pitch, void* stream)
{
    if (!g || !datas || !sizes) return set_error(HJD_E_INVALID, "NULL argument");
    if (!m) return set_error(HJD_E_INVALID, "m is NULL");
    if (!d_out) return set_error(HJD_E_INVALID, "d_out is NULL");
    int rc = hjd_internal::resize_out_check(n, out_w, out_h, out_pitch, g->out_format);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_out) & hjd_internal::out_format_align_mask(g->out_format))
        return set_error(HJD_E_INVALID, "d_out must be a multiple of the element size (%d bytes)",
                         hjd_internal::out_format_row_bytes(g->out_format));
    if (n > g->st.caps.max_frames)
        return set_error(HJD_E_INVALID, "batch of %d frames (capacity %d)", n, g->st.caps.max_frames);
    bool color_sums = false;
    if (colors) {
        bool any = false;
        rc = colors_check(colors, n, &any, &color_sums);
        if (rc) return rc;
        if (!any) colors = nullptr;   // every record the identity: the call without colours
    }
    if (convs) {
        bool any = false;
        rc = convs_check(convs, n, out_w, out_h, &any);
        if (rc) return rc;
        if (!any) convs = nullptr;   // every record the identity: the call without filters
    }
    bool tone_data = false;
    if (tones) {
        bool any = false;
        rc = tones_check(tones, n, &any, &tone_data);
        if (rc) return rc;
        if (!any) tones = nullptr;   // every curve the identity: the call without tones
    }
    // per frame: the matrix on the stored image, the rectangle it reads (the
    // crop, in the scratch), the matrix on that crop
    const size_t un = static_cast<size_t>(n);
    Region crops(un);
    ColorScratch cs(colors != nullptr, color_sums, convs != nullptr, tones != nullptr, tone_data, n, out_w, out_h);
    std::vector<int32_t> mats(6 * un);
    const WarpMap wmap{m, orientations, out_w, out_h, reinterpret_cast<int32_t(*)[6]>(mats.data())};
    const Admit admit{g->scale, false, kCapWarped, warp_map, &wmap};
    for (int i = 0; i < n; ++i) {
        hjd_rect& r = crops.dims[i];
        rc = admit_frame(admit, datas[i], sizes[i], i, nullptr, &r);
        if (rc) return rc;
        int32_t* mc = wmap.mats[i];
        const int64_t tx = static_cast<int64_t>(mc[2]) - (static_cast<int64_t>(r.x) << 16);
        const int64_t ty = static_cast<int64_t>(mc[5]) - (static_cast<int64_t>(r.y) << 16);
        if (tx < INT32_MIN || tx > INT32_MAX || ty < INT32_MIN || ty > INT32_MAX)
            return set_error(HJD_E_INVALID, "frame %d: the translation shifted to the crop at (%d, %d) leaves int32", i, r.x,
                             r.y);
        mc[2] = static_cast<int32_t>(tx);
        mc[5] = static_cast<int32_t>(ty);
        if (flags && (flags[i] & ~HJD_WARP_REPLICATE))
            return set_error(HJD_E_INVALID, "frame %d: unknown flag bits 0x%x (bit 0: HJD_WARP_REPLICATE)", i,
                             static_cast<unsigned>(flags[i] & ~HJD_WARP_REPLICATE));
        if (fills && fills[i] > 0xFFFFFFu)
            return set_error(HJD_E_INVALID, "frame %d: fill 0x%x is above 0xFFFFFF (0x00RRGGBB)", i, fills[i]);
        crops.add(i, r.w, r.h);
    }
    rc = grow_scratch(g, {&crops, &cs.mid, &cs.mid2, &cs.sums, &cs.hist, &cs.luts}, "crops");
    if (rc) return rc;
    PostPlan plan{0, {}, pixel_tables_bytes(n, true, false)};   // the pixel kernels' tables: planar bytes
    PostStage& w = add_stage(plan, PostKind::warp, crops.images(), g->out_format, sizeof(WarpRecord) * un);
    w.batch = {d_out, out_w, out_h, out_pitch};
    w.flags = flags;
    w.mats = wmap.mats;
    w.fills = fills;
    if (colors) add_color_stage(plan, w, cs, colors, g->out_format, n);
    if (convs) add_conv_stage(plan, plan.stage[plan.nstages - 1], cs, convs, g->out_format, n);
    if (tones) add_tone_stage(plan, plan.stage[plan.nstages - 1], cs, tones, g->out_format, n);
    return run_post(g, datas, sizes, n, stream, crops, true, plan);
}

}  // namespace

extern "C" {

int hjd_gdec_decode_oriented(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                             const int32_t* orientations, void* const* d_outs, const int32_t* pitches, void* stream)
{
    if (!g || !datas || !sizes) return set_error(HJD_E_INVALID, "NULL argument");
    if (!d_outs) return set_error(HJD_E_INVALID, "d_outs is NULL");
    if (!orientations) return set_error(HJD_E_INVALID, "orientations is NULL");
    if (!pitches) return set_error(HJD_E_INVALID, "pitches is NULL");
    int rc = hjd_internal::orient_out_check(n, g->out_format);
    if (rc) return rc;
    bool any = false;
    rc = orientations_check(orientations, n, &any);
    if (rc) return rc;
    if (!any)   // nothing to orient: today's call, no scratch and no extra launch
        return rois ? hjd_gdec_decode_roi(g, datas, sizes, n, rois, d_outs, pitches, stream)
                    : hjd_gdec_decode(g, datas, sizes, n, d_outs, pitches, stream);
    if (n > g->st.caps.max_frames)
        return set_error(HJD_E_INVALID, "batch of %d frames (capacity %d)", n, g->st.caps.max_frames);
    Region crops(static_cast<size_t>(n));   // the stored crops
    const Admit admit{g->scale, false, kCapOriented, rois ? orient_map : nullptr, orientations};
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        hjd_rect& crop = crops.dims[i];
        rc = admit_frame(admit, datas[i], sizes[i], i, rois ? &rois[i] : nullptr, &crop);
        if (rc) return rc;
        crops.add(i, crop.w, crop.h);
        // the record's checks on the caller's side of it, before anything is allocated: its source
        // comes with the scratch, below, so the destination stands in for it (any non-null address)
        const OrientRecord rec{d_outs[i], d_outs[i], crop.w, crop.h, crops.pitches[i], orientations[i], pitches[i], 0};
        rc = hjd_internal::orient_item_check(rec, i, g->out_format);
        if (rc) return set_error(rc, "frame %d: %s", i, std::string(hjd_last_error()).c_str());
        tiles += hjd_internal::orient_tiles(crop.w, crop.h);
    }
    rc = tiles_check(tiles);
    if (rc) return rc;
    rc = grow_scratch(g, {&crops}, "stored crops");
    if (rc) return rc;
    PostPlan plan{0, {}, pixel_tables_bytes(n, rois != nullptr, false)};   // the pixel kernels' tables: planar bytes
    PostStage& o = add_stage(plan, PostKind::orient, crops.images(), g->out_format,
                             sizeof(OrientRecord) * static_cast<size_t>(n));
    o.out = PostImages{d_outs, pitches, nullptr};
    o.orientations = orientations;
    o.tiles = tiles;
    return run_post(g, datas, sizes, n, stream, crops, rois != nullptr, plan);
}

int hjd_gdec_decode_resized(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                            const int32_t* flags, void* d_out, int out_w, int out_h, int32_t out_pitch, void* stream)
{
    return decode_resized(g, datas, sizes, n, rois, nullptr, flags, nullptr, nullptr, nullptr, d_out, out_w, out_h,
                          out_pitch, HJD_RESIZE_BILINEAR, stream);
}

int hjd_gdec_decode_resized_filter(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                   const hjd_rect* rois, const int32_t* flags, void* d_out, int out_w, int out_h,
                                   int32_t out_pitch, int filter, void* stream)
{
    return decode_resized(g, datas, sizes, n, rois, nullptr, flags, nullptr, nullptr, nullptr, d_out, out_w, out_h,
                          out_pitch, filter, stream);
}

int hjd_gdec_decode_resized_oriented(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                     const hjd_rect* rois, const int32_t* orientations, const int32_t* flags, void* d_out,
                                     int out_w, int out_h, int32_t out_pitch, int filter, void* stream)
{
    if (!orientations) return set_error(HJD_E_INVALID, "orientations is NULL");
    return decode_resized(g, datas, sizes, n, rois, orientations, flags, nullptr, nullptr, nullptr, d_out, out_w, out_h,
                          out_pitch, filter, stream);
}

int hjd_gdec_decode_resized_color(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                  const hjd_rect* rois, const int32_t* orientations, const int32_t* flags,
                                  const int32_t (*colors)[21], void* d_out, int out_w, int out_h, int32_t out_pitch,
                                  int filter, void* stream)
{
    if (!colors) return set_error(HJD_E_INVALID, "colors is NULL");
    return decode_resized(g, datas, sizes, n, rois, orientations, flags, colors, nullptr, nullptr, d_out, out_w, out_h,
                          out_pitch, filter, stream);
}

int hjd_gdec_decode_resized_tone(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                                 const int32_t* orientations, const int32_t* flags, const int32_t (*colors)[21],
                                 const hjd_tone_curve* tones, void* d_out, int out_w, int out_h, int32_t out_pitch,
                                 int filter, void* stream)
{
    if (!tones) return set_error(HJD_E_INVALID, "tones is NULL");
    return decode_resized(g, datas, sizes, n, rois, orientations, flags, colors, nullptr, tones, d_out, out_w, out_h,
                          out_pitch, filter, stream);
}

int hjd_gdec_decode_warped(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const int32_t (*m)[6],
                           const int32_t* orientations, const int32_t* flags, const uint32_t* fills, void* d_out,
                           int out_w, int out_h, int32_t out_pitch, void* stream)
{
    return decode_warped(g, datas, sizes, n, m, orientations, flags, fills, nullptr, nullptr, nullptr, d_out, out_w, out_h,
                         out_pitch, stream);
}

int hjd_gdec_decode_warped_color(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n,
                                 const int32_t (*m)[6], const int32_t* orientations, const int32_t* flags,
                                 const uint32_t* fills, const int32_t (*colors)[21], void* d_out, int out_w, int out_h,
                                 int32_t out_pitch, void* stream)
{
    if (!colors) return set_error(HJD_E_INVALID, "colors is NULL");
    return decode_warped(g, datas, sizes, n, m, orientations, flags, fills, colors, nullptr, nullptr, d_out, out_w, out_h,
                         out_pitch, stream);
}

int hjd_gdec_decode_warped_tone(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const int32_t (*m)[6],
                                const int32_t* orientations, const int32_t* flags, const uint32_t* fills,
                                const int32_t (*colors)[21], const hjd_tone_curve* tones, void* d_out, int out_w, int out_h,
                                int32_t out_pitch, void* stream)
{
    if (!tones) return set_error(HJD_E_INVALID, "tones is NULL");
    return decode_warped(g, datas, sizes, n, m, orientations, flags, fills, colors, nullptr, tones, d_out, out_w, out_h,
                         out_pitch, stream);
}

int hjd_gdec_decode_resized_aug(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                                const int32_t* orientations, const int32_t* flags, const int32_t (*colors)[21],
                                const hjd_conv_filter* convs, const hjd_tone_curve* tones, void* d_out, int out_w, int out_h,
                                int32_t out_pitch, int filter, void* stream)
{
    return decode_resized(g, datas, sizes, n, rois, orientations, flags, colors, convs, tones, d_out, out_w, out_h,
                          out_pitch, filter, stream);
}

int hjd_gdec_decode_warped_aug(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const int32_t (*m)[6],
                               const int32_t* orientations, const int32_t* flags, const uint32_t* fills,
                               const int32_t (*colors)[21], const hjd_conv_filter* convs, const hjd_tone_curve* tones,
                               void* d_out, int out_w, int out_h, int32_t out_pitch, void* stream)
{
    return decode_warped(g, datas, sizes, n, m, orientations, flags, fills, colors, convs, tones, d_out, out_w, out_h,
                         out_pitch, stream);
}

}  // extern "C"
