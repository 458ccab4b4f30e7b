// hjd_gdec.hip -- the GPU entropy decoder object (include/hjd_host.h hjd_gdec_*;
// DESIGN.md s10): its device buffers, the policy that picks a batch's sync and
// subsequence length, and the issue of a staged batch -- uploads, the entropy
// kernels (launched in hjd_entropy.hip), then the fused pixel kernel.  The
// calls with stages behind the pixel kernels are hjd_gdec_post.hip's.
#include "hjd_gdec.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <utility>

#include "hjd_host.h"

using hjd_internal::FrameRecord;
using hjd_internal::set_error;
using hjd_internal::tuning;
using namespace hjd::ent;

// ---------------------------------------------------------------------------
// Policy: a batch's sync, its subsequence length S and its lead-in
// ---------------------------------------------------------------------------

// Lead-in of the speculative sync's spec runs (HJD_SPEC_LEAD overrides; tuning).
// A chain breaks where none of a subsequence's spec runs has met the true
// decode by its checkpoint; a longer lead-in makes that rarer and costs every
// spec run its length.  Measured FHD single images (ms at W = 512 / 1536,
// profiles/r06zx_spec_lead.json): bench q90 4:2:0 0.40 / 0.46 (no break),
// another q90 4:2:0 at the same 164 bits per block 0.61 / 0.46 (2 breaks),
// q90 4:4:4 0.96 / 0.47 (9 breaks), q93 4:2:0 1.10 / 0.75 (19 / 3 breaks;
// none at 2048, host emulation).  Bits per block do not tell these apart, so
// the decoder goes by its own history: a batch whose chain needed a repair
// moves the next batches one step up the ladder, and kLeadBatches clean
// batches move them one step down (a camera's frames look alike).  A repair
// right after a step down doubles the clean run the next step down waits for
// (up to kLeadBatchesMax), so a stream that needs the long lead-in pays a
// repaired frame ever more rarely.
constexpr uint32_t kLeadLadder[] = {512, 1536, 2560};
constexpr uint32_t kLeadSteps = sizeof(kLeadLadder) / sizeof(kLeadLadder[0]), kLeadBatches = 32,
                   kLeadBatchesMax = 4096;
uint32_t hjd::ent::spec_lead_bits(uint32_t step)
{
    const auto& e = tuning().spec_lead;
    return e.is_set() ? static_cast<uint32_t>(e.get()) : kLeadLadder[step < kLeadSteps ? step : kLeadSteps - 1];
}

// Dense scans sync slowly: at S = 512 a q95 FHD frame breaks the
// speculative chain ~200 times and a q100 one ~3,600 times, each break a
// serial single-thread repair (8 ms and worse per image).  Above
// kDenseBitsPerBlock a latency decoder takes the round-based sync instead,
// at longer subsequences the denser the scan (kDenseTiers: q95 FHD 4:2:0
// 1.4 ms at S = 1024; q98 2.4 at 2048 against 6.0 at 1024; q100 7.6 at 8192
// against 14 at 2048; tools/fhd_env_sweep.py).  Never shorter than the
// decoder's S (its capacity is sized for that).
constexpr uint64_t kDenseBitsPerBlock = 200;   // (a q90 FHD 4:2:0 frame: 164; q95: 232; q100: 436)
// the round-based S of a dense scan: the first tier whose bits per block bound
// it (best S measured per FHD frame: q95 232 / 243 -> 1024, q97 286 / 301 and
// q98 322 -> 2048, q99 388 and q100 436 -> 8192; profiles/r06zz_dense_sub_bits.json)
constexpr struct { uint64_t bits_per_block; uint32_t sub_bits; } kDenseTiers[] = {
    {260, 1024}, {360, 2048}, {0, 8192}};   // (the last: everything denser)

// Subsequence length when the caller passes 0.  Longer subsequences mean fewer
// guessed starts to repair but fewer workgroups.  Measured on 4K q90 4:2:0
// batches (profiles/r01_entropy_subbits.json, sync + write kernels):
// - 64 frames: S = 4096 is 5-8 % faster than 2048;
// - 32 frames: S = 4096 is 6 % slower;
// - 8 frames: S = 4096 is 34 % slower.
// Hence 4096 for decoders sized for >= 48 frames per call (the stream's
// 48-frame batches: profiles/r01_stream_batch_ab.json).  A decoder for one or
// two images is latency-bound by the serial chain of a subsequence: one FHD
// q90 JPEG, end to end, took 1.16 ms at S = 1024 against 1.35 ms at 2048
// (512: 1.04 ms, but its 4096-bit warm-up overlap fails to link often enough
// at 256 to fall back; profiles/r02_fhd_jpeg_subbits.json), so 1024 there.
// With the sync kernel's step tables: 1.05 ms at 1024, 0.96 at 512, 1.21 at 2048.
// HJD_SUB_BITS overrides it (tuning hook, tools/gpu_subbits_sweep.sh).
static int default_sub_bits(int max_frames)
{
    const auto& e = tuning().sub_bits;
    if (e.is_set() && e.get()) return static_cast<int>(e.get());
    return max_frames >= 48 ? 2 * kDefaultSubBits : max_frames <= 2 ? kDefaultSubBits / 2 : kDefaultSubBits;
}

// The stream's decoders: batches of several slots overlap on the GPU, so the
// parallelism a single batch lacks at long subsequences comes from the other
// slots, and fewer guessed starts to repair wins.  Measured end to end on the
// config-5 stream (profiles/r02_stream_subbits.json): S = 8192 at 32-48
// frames per batch x 8 slots gives 97-101 Gpx/s against 91-94 at S = 4096;
// 16384 and 64-96-frame batches are slower.
// Speculative sync (ent_spec/cand/sync_spec kernels) for latency decoders:
// one or two frames per call, where the round-based sync's serial rounds are
// the critical path and most of the GPU is idle.  HJD_SYNC_SPEC=0/1 overrides.
static bool spec_sync_default(int max_frames)
{
    const auto& e = tuning().sync_spec;
    if (e.is_set()) return e.get() != 0;
    return max_frames <= 2;
}

int hjd::ent::stream_sub_bits(int max_frames)
{
    const auto& e = tuning().sub_bits;
    if (e.is_set()) return static_cast<int>(e.get());
    return max_frames >= 24 ? 4 * kDefaultSubBits : default_sub_bits(max_frames);
}

// The sync of the batch staged in g (g->batch_spec) and its S, which it returns
// (g->batch_sub_bits: 0 unless a dense tier's): kDenseBitsPerBlock, kDenseTiers.
static uint32_t choose_sync(hjd_gdec* g)
{
    g->batch_spec = g->spec;
    g->batch_sub_bits = 0;
    const uint32_t S = static_cast<uint32_t>(g->st.caps.sub_bits);
    if (!g->spec) return S;
    uint64_t bits = 0, blocks = 0;
    for (const Prepared& p : g->st.frames) {
        bits += p.data_bits;
        blocks += static_cast<uint64_t>(p.nblocks);
        for (const Prepared& q : p.more) {
            bits += q.data_bits;
            blocks += static_cast<uint64_t>(q.nblocks);
        }
    }
    if (bits <= kDenseBitsPerBlock * blocks) return S;
    g->batch_spec = false;
    const auto& e = tuning().dense_sub_bits;   // tuning: the dense scans' S
    constexpr size_t nt = sizeof(kDenseTiers) / sizeof(kDenseTiers[0]);
    size_t t = 0;
    while (t + 1 < nt && bits > kDenseTiers[t].bits_per_block * blocks) ++t;
    const uint32_t want = e.is_set() ? static_cast<uint32_t>(e.get()) : kDenseTiers[t].sub_bits;
    return g->batch_sub_bits = std::max(want, S);
}

// ---------------------------------------------------------------------------
// Batch object
// ---------------------------------------------------------------------------
namespace {

// HJD_DESTUFF: "host" (always destuff on the host), "device" (always on the
// GPU; unpinned bytes are memcpy'd raw into staging), default "auto": on the
// GPU when the caller's bytes are pinned host memory (hipHostMalloc'd or
// hipHostRegister'ed, e.g. hjd_host_register), so the host CPU never touches
// the scan, on the host otherwise.
int destuff_policy() { return static_cast<int>(tuning().destuff.get()); }

bool pinned_host(const void* p, size_t n)
{
    if (!p || !n) return false;
    for (const void* q : {p, static_cast<const void*>(static_cast<const uint8_t*>(p) + n - 1)}) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, q) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}

}  // namespace

int hjd::ent::plan_raw(const Staging& st, const uint8_t* data, size_t size, RawCursor& cur, int& mode,
                       uint64_t& raw_off, bool& fits, size_t data_room, uint64_t reserve, bool host_fallback)
{
    mode = kDestuffHost;
    raw_off = 0;
    fits = true;
    const int pol = destuff_policy();
    if (pol == hjd_internal::kPolicyHost || !data) return HJD_OK;
    const bool pinned = pinned_host(data, size);
    if (pol == hjd_internal::kPolicyDevice) mode = pinned ? kDestuffFromCaller : kDestuffFromStaging;
    else if (pinned) mode = kDestuffFromCaller;
    if (mode == kDestuffHost) return HJD_OK;
    hjd_internal::ScanHeader h;
    const int rc = hjd_internal::parse_scan_header(data, size, &h);
    if (rc) return rc;
    if (h.scan_offset >= size) return set_error(HJD_E_INVALID, "empty scan");
    if (h.extra_scans > 0) {   // several scans: destuffed (and their ends found) on the host
        mode = kDestuffHost;
        return HJD_OK;
    }
    const size_t raw = size - h.scan_offset;
    // the device path needs the raw scan (stuffing, markers and the bytes
    // after EOI included) in both the raw and the data area; the host path
    // only the destuffed bytes in the data area
    fits = align_up(raw + kDataPad, 16) + reserve <= data_room &&
           cur.place(data + h.scan_offset, raw, size, mode == kDestuffFromCaller, st.data_cap(), raw_off, reserve);
    if (!fits && host_fallback && pol == hjd_internal::kPolicyAuto) {   // auto: destuff this one on the host instead
        mode = kDestuffHost;
        raw_off = 0;
        fits = true;
    }
    return HJD_OK;
}

namespace {

int gdec_alloc(hjd_gdec* g)
{
    const Caps& caps = g->st.caps;
    const size_t total = g->st.bytes();
    const size_t subs = static_cast<size_t>(caps.max_subs), wgs = static_cast<size_t>(caps.max_wgs);
    const size_t ef = kMaxScans * static_cast<size_t>(caps.max_frames);   // entropy frames
    HJD_HIP(hipSetDevice(g->device));
    // (a failed alloc has set the error text)
    bool bad = g->alloc(g->st.h_stage, total, true) || g->alloc(g->h_status, 4 * ef, true) ||
               g->alloc(g->d_blob, total) || g->alloc(g->d_entries, 8 * subs) ||
               g->alloc(g->d_stats, sizeof(SubStats) * subs) || g->alloc(g->d_mids, 8 * subs) ||
               g->alloc(g->d_stats1, sizeof(SubStats) * subs) || g->alloc(g->d_wentries, 8 * kWarm * wgs) ||
               g->alloc(g->d_linked, 4 * wgs) || g->alloc(g->d_agg, sizeof(SubStats) * wgs) ||
               g->alloc(g->d_coefs, 128 * static_cast<size_t>(caps.max_blocks)) ||
               g->alloc(g->d_raw, g->st.data_cap()) || g->alloc(g->d_tiles, 12 * static_cast<size_t>(caps.max_tiles)) ||
               g->alloc(g->d_steps, (kMaxTables * ef) << kStepBits);
    // chunk functions: [entropy frame][chunks of the largest frame]
    g->chain_fn_rows = g->spec ? static_cast<int64_t>(ef * (subs / kChainChunk + 1)) : 0;
    const size_t fn_bytes = 4 * kLbWords * static_cast<size_t>(g->chain_fn_rows);
    if (g->spec)
        bad = bad || g->alloc(g->d_spec, sizeof(SpecRec) * kMaxBpm * subs) ||
              g->alloc(g->d_cand, sizeof(CandRec) * kCandRow * subs) || g->alloc(g->d_cmap, kSlotRow * subs) ||
              g->alloc(g->d_cslot, subs + 16) || g->alloc(g->d_chainfn, fn_bytes) ||
              g->alloc(g->d_chain_broken, 4 * ef) || g->alloc(g->d_agg2, sizeof(SubStats) * wgs);
    if (bad) return HJD_E_HIP;
    if (g->spec) {
        HJD_HIP(hipMemset(g->d_chain_broken, 0, 4 * ef));
        HJD_HIP(hipMemset(g->d_chainfn, 0, fn_bytes));
    }
    HJD_HIP(hipEventCreateWithFlags(&g->staged, hipEventDisableTiming));
    HJD_HIP(hipEventCreateWithFlags(&g->done, hipEventDisableTiming));
    return HJD_OK;
}

// DestuffHook::fire of a latency decoder's lone image: pull the destuffed
// bytes that are final so far (16-B words) while the host destuffs the rest;
// gdec_issue pulls the remainder with the header.  One early pull per call
// (each costs a launch on the host, ~5 us: two measured no better).
void gdec_early_pull(DestuffHook* h, size_t done)
{
    GdecCall& c = *static_cast<GdecCall*>(h->ctx);
    hjd_gdec* g = c.early_g;
    h->next = SIZE_MAX;
    const size_t upto = done & ~static_cast<size_t>(15);
    if (upto <= c.prepulled) return;
    PullSegs segs{};
    segs.add(g->st.caps.data + c.prepulled, upto - c.prepulled);   // frame 0: data_off 0
    if (hipSetDevice(g->device) != hipSuccess) return;
    if (g->pending && hipStreamWaitEvent(c.stream, g->done, 0) != hipSuccess) return;
    if (launch_pull(g->st.h_stage, g->d_blob, segs, c.stream) == hipSuccess) c.prepulled = upto;
}

// Pixel-kernel launch groups of a batch, one per sampling class
// (hjd_internal::SamplingGeom::index): each class's frame table
// (hjd_internal::frame_table) at `table` bytes from H.recs.
constexpr int kClassSampling[hjd_internal::kSamplingClasses] = {HJD_YUV444, HJD_YUV420,      HJD_YUV422,
                                                                HJD_GRAY,   HJD_YUV411_H4V1, HJD_YUV440};
struct PixelClasses {
    int nrec[hjd_internal::kSamplingClasses] = {};
    int64_t tasks[hjd_internal::kSamplingClasses] = {};
    uint8_t* out_base[hjd_internal::kSamplingClasses] = {};
    size_t table[hjd_internal::kSamplingClasses] = {};
    bool roi = false;
    int out_format = 0;   // what the pixel kernels write: the decoder's, or planar bytes for the stages
};

// Pixel-kernel launch class of a sampling (parse_scan_header admits only known ones).
inline int sampling_class(int sampling)
{
    hjd_internal::SamplingGeom g;
    return hjd_internal::sampling_geom(sampling, &g) ? g.index : 0;
}

// The pixel kernel's tables of the batch assembled in g->st: the frame
// records grouped by sampling class (one launch each) at H.recs, and the
// natural-order qtables at H.qt.
int write_pixel_records(hjd_gdec* g, const GdecCall& c, int out_format, bool fnorm, PixelClasses& px)
{
    Staging& st = g->st;
    const int n = static_cast<int>(st.frames.size());
    const hjd_rect* rois = c.rois;
    px.roi = rois != nullptr;
    const EntFrame* ef = reinterpret_cast<const EntFrame*>(st.h_stage + st.H.frames);
    int32_t* qtn = reinterpret_cast<int32_t*>(st.h_stage + st.H.qt);
    const int obytes = hjd_internal::out_format_row_bytes(out_format);
    const uintptr_t amask = hjd_internal::out_format_align_mask(out_format);
    const int pmask = hjd_internal::out_format_pitch_mask(out_format);
    for (int i = 0; i < n; ++i) {
        const Prepared& p = st.frames[i];
        const int out_w = rois ? rois[i].w : hjd_internal::scaled_dim(p.width, g->scale);
        if (!c.d_outs[i] || !c.pitches || c.pitches[i] < obytes * out_w ||
            (c.pitches[i] & pmask) ||
            (reinterpret_cast<uintptr_t>(c.d_outs[i]) & amask))
            return set_error(HJD_E_INVALID,
                             "frame %d: bad output buffer or pitch (BGRX: 16-byte aligned, >= 4*width; "
                             "BGR24: 4-byte aligned, >= 3*width; RGB24: >= 3*width; planar RGB: >= width; "
                             "float planar: element-aligned, >= 2*width (F16) or 4*width (F32); "
                             "width = the scaled width, or the ROI's)", i);
        if (c.pitches[i] > hjd_internal::kMaxOutPitch)
            return set_error(HJD_E_INVALID, "frame %d: out_pitch %d is above HJD_MAX_OUT_PITCH (%d)", i, c.pitches[i],
                             hjd_internal::kMaxOutPitch);
        ++px.nrec[sampling_class(p.sampling)];
    }
    for (int k = 1; k < hjd_internal::kSamplingClasses; ++k)
        px.table[k] = px.table[k - 1] + hjd_internal::frame_table(px.nrec[k - 1], px.roi, fnorm).bytes;
    int written[hjd_internal::kSamplingClasses] = {};
    for (int i = 0; i < n; ++i) {
        const Prepared& p = st.frames[i];
        const int sidx = sampling_class(p.sampling);
        if (!px.out_base[sidx]) px.out_base[sidx] = static_cast<uint8_t*>(c.d_outs[i]);
        const int qti[3] = {3 * i, 3 * i + 1, 3 * i + 2};
        FrameRecord rec;
        hjd_internal::RoiRecord side;
        const int64_t t = hjd_internal::make_frame_record(
            p.width, p.height, p.sampling, static_cast<int64_t>(ef[i].coef_off),
            static_cast<int64_t>(static_cast<uint8_t*>(c.d_outs[i]) - px.out_base[sidx]), c.pitches[i], qti, &rec,
            out_format, reinterpret_cast<uintptr_t>(px.out_base[sidx]), g->scale, rois ? &rois[i] : nullptr,
            rois ? &side : nullptr);
        if (t < 0) return static_cast<int>(t);
        rec.task_begin = px.tasks[sidx];
        px.tasks[sidx] += t;
        const hjd_internal::FrameTable tab = hjd_internal::frame_table(px.nrec[sidx], px.roi, fnorm);
        uint8_t* tablep = st.h_stage + st.H.recs + px.table[sidx];
        reinterpret_cast<FrameRecord*>(tablep)[written[sidx]] = rec;
        if (rois) reinterpret_cast<hjd_internal::RoiRecord*>(tablep + tab.side)[written[sidx]] = side;
        if (fnorm) memcpy(tablep + tab.norm, &g->norm, sizeof(g->norm));
        ++written[sidx];
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < 64; ++k) qtn[(3 * i + q) * 64 + hjd_internal::kZigzag[k]] = p.qt[q][k];
    }
    return HJD_OK;
}

// ---------------------------------------------------------------------------
// The steps of gdec_issue, in its order
// ---------------------------------------------------------------------------

// The batch header at subsequence length S (Staging::assemble) with the call's
// records in it: the pixel kernels' tables (px; px.out_format is what those
// kernels write) and the stages'.
int assemble_batch(hjd_gdec* g, const GdecCall& c, uint32_t S, int16_t* coefs, EntBatchDev& b, PixelClasses& px)
{
    const int n = static_cast<int>(g->st.frames.size());
    px.out_format = g->out_format;
    bool fnorm = c.d_outs && hjd_internal::out_format_float_bytes(px.out_format) != 0;
    size_t recs_bytes = c.d_outs ? pixel_tables_bytes(n, c.rois != nullptr, fnorm) : 0;
    if (c.post) {   // the pixel kernels write planar bytes (the crops); the last stage the decoder's format
        px.out_format = HJD_OUT_RGB_PLANAR;
        fnorm = false;
        recs_bytes = c.post->recs_bytes;
    }
    int rc = g->st.assemble(g->d_blob, coefs, c.block_offsets, S, recs_bytes,
                            c.d_outs ? 192 * 4 * static_cast<size_t>(n) : 0, b);
    if (rc || !c.d_outs) return rc;
    rc = write_pixel_records(g, c, px.out_format, fnorm, px);
    if (rc || !c.post) return rc;
    return post_write_records(g, *c.post, n);
}

// The decoder's work arrays in b, for the sync choose_sync picked.  The
// look-back chain kernel's launch takes the next 24-bit tag: true when the tag
// started over at 1 (issue_uploads then clears the words).
bool bind_work_arrays(hjd_gdec* g, EntBatchDev& b)
{
    b.entries = g->d_entries;
    b.stats = g->d_stats;
    b.mids = g->d_mids;
    b.stats1 = g->d_stats1;
    b.wentries = g->d_wentries;
    b.linked = g->d_linked;
    b.agg = g->d_agg;
    b.status = reinterpret_cast<uint32_t*>(g->d_blob + g->st.H.status);
    if (b.nwg) b.host_status = g->h_status;   // the write kernel delivers the status words
    b.raw = g->d_raw;
    b.tiles = g->d_tiles;
    b.steps_g = g->d_steps;
    g->batch_lookback = false;
    g->batch_chain_chunks = b.chain_chunks;
    g->batch_lead = 0;
    if (!g->batch_spec) return false;
    b.spec = g->d_spec;
    b.cand = g->d_cand;
    b.cmap = g->d_cmap;
    b.cslot = g->d_cslot;
    b.spec_lead = spec_lead_bits(g->lead_step);
    g->batch_lead = b.spec_lead;
    if (static_cast<int64_t>(b.chain_chunks) * b.nframes > g->chain_fn_rows) return false;
    b.chainfn = g->d_chainfn;
    b.chain_broken = g->d_chain_broken;
    b.agg2 = g->d_agg2;
    const bool wrapped = g->chain_epoch >= 0xFFFFFFu;
    g->chain_epoch = g->chain_epoch % 0xFFFFFFu + 1u;   // 1 .. 2^24 - 1
    b.chain_epoch = g->chain_epoch;
    g->batch_lookback = true;
    return wrapped;
}

// Everything the kernels wait for, on s: the previous call, the clearing of
// the look-back words at the tag's wrap, then the plan's uploads as it lists them.
int issue_uploads(hjd_gdec* g, const UploadPlan& plan, bool epoch_wrapped, hipStream_t s)
{
    // the device buffers are reused: order this call after the previous one
    // (which may have been issued on another stream)
    if (g->pending) HJD_HIP(hipStreamWaitEvent(s, g->done, 0));
    // The look-back words are told apart by their tag alone, and a frame's word
    // row moves with the batch's chain_chunks, so a word may outlive any number
    // of launches.  When the tag starts over at 1, the words of the launches one
    // cycle (2^24 - 1 launches) earlier would carry this launch's tag again:
    // clear them all, behind the previous call and before this call's kernels
    // (one memset per 16.7 M launches).
    if (epoch_wrapped)
        HJD_HIP(hipMemsetAsync(g->d_chainfn, 0, 4 * kLbWords * static_cast<size_t>(g->chain_fn_rows), s));
    if (plan.pull) HJD_HIP(launch_pull(g->st.h_stage, g->d_blob, plan.segs, s));   // (and no copies)
    for (const UploadCopy& u : plan.copies) {
        uint8_t* dst = (u.kind == kUploadHeader || u.kind == kUploadData ? g->d_blob : g->d_raw) + u.dst_off;
        if (u.kind != kUploadRawCaller) {
            HJD_HIP(hipMemcpyAsync(dst, g->st.h_stage + u.src, u.bytes, hipMemcpyHostToDevice, s));
            continue;
        }
        // (hipMemcpyBatchAsync would submit the caller's spans at once, but the HIP runtime
        // this library shares with PyTorch -- DESIGN.md s8 -- predates it)
        if (hipMemcpyAsync(dst, reinterpret_cast<const void*>(u.src), u.bytes, hipMemcpyHostToDevice, s) == hipSuccess)
            continue;
        // A merged span can cross from one pinned allocation into another (the
        // caller's buffers merely lie close together), which the DMA rejects
        // before queueing anything: copy those scans one by one.
        (void)hipGetLastError();
        if (u.last - u.first < 2)
            return set_error(HJD_E_HIP, "hipMemcpyAsync of a pinned scan (%zu bytes) failed", u.bytes);
        for (int f = u.first; f < u.last; ++f) {
            const Prepared& q = g->st.frames[f];
            HJD_HIP(hipMemcpyAsync(g->d_raw + q.raw_off, const_cast<uint8_t*>(q.raw_src), q.raw_len,
                                   hipMemcpyHostToDevice, s));
        }
    }
    g->last_h2d = plan.moved;
    g->last_host_scan_bytes = plan.host_bytes;
    // (pulled: the staging is free when `done` fires -- an event between the
    // pull and the first entropy kernel delayed that kernel by ~6 us, and a
    // latency decoder's next call waits for `done` anyway)
    if (!plan.pull) HJD_HIP(hipEventRecord(g->staged, s));
    g->staged_by_done = plan.pull;
    g->pending = true;
    return HJD_OK;
}

// A multi-scan file's non-interleaved scans leave its MCU-padding blocks
// uncoded: they must read as zeros (as the host decoder's).
int zero_multiscan_padding(const Staging& st, int16_t* coefs, hipStream_t s)
{
    size_t first = 0;
    for (const Prepared& p : st.frames) {
        if (!p.more.empty()) HJD_HIP(hipMemsetAsync(coefs + first * 64, 0, static_cast<size_t>(p.out_blocks) * 128, s));
        first += static_cast<size_t>(p.out_blocks);
    }
    return HJD_OK;
}

// One pixel-kernel launch per sampling class the batch has, then the call's stages.
int launch_pixels(hjd_gdec* g, const GdecCall& c, const PixelClasses& px, const int16_t* coefs, hipStream_t s)
{
    for (int sidx = 0; sidx < hjd_internal::kSamplingClasses; ++sidx) {
        if (!px.nrec[sidx]) continue;
        hjd_internal::DecodeLaunch l;   // int16 input, HJD_KERNEL_AUTO, the default grid
        l.sampling = kClassSampling[sidx];
        l.out_format = px.out_format;
        l.scale = g->scale;
        l.roi = px.roi;
        l.tasks = px.tasks[sidx];
        l.device = g->device;
        l.d_coefs = coefs;
        l.d_qt_nat = reinterpret_cast<const int32_t*>(g->d_blob + g->st.H.qt);
        l.d_frames = reinterpret_cast<const FrameRecord*>(g->d_blob + g->st.H.recs + px.table[sidx]);
        l.nframes = px.nrec[sidx];
        l.d_out = px.out_base[sidx];
        l.stream = s;
        const int rc = hjd_internal::launch_decode(l);
        if (rc) return rc;
    }
    // behind the pixel kernels; `done` covers them
    return c.post ? post_launch(g, *c.post, static_cast<int>(g->st.frames.size()), s) : HJD_OK;
}

// What goes back to the host: the pixels of host-output frames (the D2H sink)
// to the caller's memory, and the status words unless the write kernel delivers them.
int copy_back(hjd_gdec* g, const GdecCall& c, const EntBatchDev& b, hipStream_t s)
{
    for (size_t i = 0; c.host && c.d_outs && i < g->st.frames.size(); ++i) {
        const HostCopy& h = c.host[i];
        if (!h.host) continue;
        // planar: the planes are contiguous at pitch * height on both
        // sides, so one copy of 3 * height rows moves all three
        HJD_HIP(hipMemcpy2DAsync(h.host, static_cast<size_t>(h.host_pitch), c.d_outs[i],
                                 static_cast<size_t>(c.pitches[i]),
                                 static_cast<size_t>(h.width) * hjd_internal::out_format_row_bytes(g->out_format),
                                 static_cast<size_t>(hjd_internal::out_format_rows(g->out_format, h.height)),
                                 hipMemcpyDeviceToHost, s));
    }
    if (!b.host_status)
        HJD_HIP(hipMemcpyAsync(g->h_status, b.status, 4 * static_cast<size_t>(b.nframes), hipMemcpyDeviceToHost, s));
    return HJD_OK;
}

}  // namespace

int hjd::ent::gdec_issue(hjd_gdec* g, GdecCall& c)
{
    HJD_HIP(hipSetDevice(g->device));
    const hipStream_t s = c.stream;
    int16_t* coefs = c.coefs_out ? c.coefs_out : g->d_coefs;
    const uint32_t S = choose_sync(g);
    EntBatchDev b;
    PixelClasses px;
    int rc = assemble_batch(g, c, S, coefs, b, px);
    if (rc) return rc;
    const bool epoch_wrapped = bind_work_arrays(g, b);
    g->st.plan_uploads(g->spec, c.prepulled, g->uploads);
    rc = issue_uploads(g, g->uploads, epoch_wrapped, s);
    if (rc) return rc;
    rc = zero_multiscan_padding(g->st, coefs, s);
    if (rc) return rc;
    rc = launch_entropy(b, g->st.h_stage + g->st.H.tabs, g->steps_tabs, s);
    if (rc) return rc;
    if (c.d_outs) rc = launch_pixels(g, c, px, coefs, s);
    if (rc) return rc;
    rc = copy_back(g, c, b, s);
    if (rc) return rc;
    HJD_HIP(hipEventRecord(g->done, s));
    g->nframes_issued = static_cast<int>(g->st.frames.size());
    return HJD_OK;
}

namespace {

// PlanFn of a decoder's own staging: HJD_DESTUFF=auto may fall back to the host path.
int plan_staged(const Staging& st, const uint8_t* data, size_t size, RawCursor& cur, int& mode, uint64_t& raw_off,
                bool& fits, size_t data_room, uint64_t reserve)
{
    return plan_raw(st, data, size, cur, mode, raw_off, fits, data_room, reserve, true);
}

}  // namespace

int hjd::ent::gdec_run(hjd_gdec* g, GdecCall& c)
{
    if (!g || !c.datas || !c.sizes) return set_error(HJD_E_INVALID, "NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    if (g->pending) {   // the previous call still reads the staging
        HJD_HIP(hipSetDevice(g->device));
        HJD_HIP(hipEventSynchronize(g->staged_by_done ? g->done : g->staged));
    }
    const auto t1 = std::chrono::steady_clock::now();
    // a lone image may be pulled while it is destuffed
    DestuffHook hook{SIZE_MAX, gdec_early_pull, &c};
    c.early_g = g->spec && c.n == 1 ? g : nullptr;
    int rc = g->st.stage_frames(c.datas, c.sizes, c.n, plan_staged, c.early_g ? &hook : nullptr);
    c.early_g = nullptr;
    if (rc) {
        if (c.prepulled) (void)hipStreamSynchronize(c.stream);   // an early pull still reads the staging
        return rc;
    }
    const auto t2 = std::chrono::steady_clock::now();
    rc = gdec_issue(g, c);
    if (rc) return rc;
    const auto t3 = std::chrono::steady_clock::now();
    g->host_us[0] += std::chrono::duration<double, std::micro>(t1 - t0).count();
    g->host_us[1] += std::chrono::duration<double, std::micro>(t2 - t1).count();
    g->host_us[2] += std::chrono::duration<double, std::micro>(t3 - t2).count();
    ++g->host_calls;
    // The caller may reuse its bytes once this returns (include/hjd_host.h):
    // scans read by DMA straight from the caller's pinned memory must have
    // landed first.  Only the uploads are waited for, not the kernels.
    for (const Prepared& p : g->st.frames)
        if (p.destuff == kDestuffFromCaller) {
            HJD_HIP(hipEventSynchronize(g->staged));
            break;
        }
    return HJD_OK;
}

int hjd::ent::admit_frame(const Admit& a, const uint8_t* data, size_t size, int i, const hjd_rect* roi, hjd_rect* crop)
{
    hjd_internal::ScanHeader h;
    int rc = data ? hjd_internal::parse_scan_header(data, size, &h) : HJD_E_INVALID;
    if (rc && a.lenient) return HJD_OK;
    if (!data) return set_error(HJD_E_INVALID, "frame %d: NULL data", i);
    if (!rc) {
        *crop = hjd_rect{0, 0, hjd_internal::scaled_dim(h.width, a.scale), hjd_internal::scaled_dim(h.height, a.scale)};
        if (a.map) rc = a.map(a.ctx, i, crop->w, crop->h, roi, crop);
        else if (roi) *crop = *roi;
    }
    if (!rc && (a.map || roi)) {   // the rectangle, and the scale against the file's sampling
        hjd_internal::RoiGeom rg;
        rc = hjd_internal::roi_geom(h.width, h.height, h.sampling, a.scale, crop, &rg);
    } else if (!rc && a.scale != 1) {   // a whole frame: a file the scaled kernels do not serve
        hjd_internal::DecodeShape shape;
        shape.scale = a.scale;
        shape.sampling = h.sampling;
        rc = hjd_internal::shape_check(shape);
    }
    if (rc) return set_error(rc, "frame %d: %s", i, std::string(hjd_last_error()).c_str());
    if (a.cap_fmt && (crop->w > hjd_internal::kResizeMaxDim || crop->h > hjd_internal::kResizeMaxDim))
        return set_error(HJD_E_INVALID, a.cap_fmt, i, crop->w, crop->h, hjd_internal::kResizeMaxDim);
    return HJD_OK;
}

namespace {

// hjd_gdec_decode (rois null) and _roi.  An invalid rectangle, or a scale the
// file's sampling does not serve, is refused before anything is staged or
// enqueued (a file that is null or malformed fails in staging).
int decode_pixels(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                  void* const* d_outs, const int32_t* pitches, void* stream)
{
    if (g && datas && sizes && (rois || g->scale != 1)) {
        const Admit admit{g->scale, true, nullptr, nullptr, nullptr};
        hjd_rect crop;
        for (int i = 0; i < n; ++i) {
            const int rc = admit_frame(admit, datas[i], sizes[i], i, rois ? &rois[i] : nullptr, &crop);
            if (rc) return rc;
        }
    }
    GdecCall c(datas, sizes, n, stream);
    c.d_outs = d_outs;
    c.pitches = pitches;
    c.rois = rois;
    return gdec_run(g, c);
}

}  // namespace

extern "C" {

int hjd_gdec_create(hjd_ctx* ctx, int max_frames, int64_t max_scan_bytes, int64_t max_blocks, int sub_bits,
                    hjd_gdec** out)
{
    if (!ctx || !out || max_frames <= 0 || max_scan_bytes <= 0 || max_blocks <= 0)
        return set_error(HJD_E_INVALID, "invalid gdec arguments");
    const bool spec = spec_sync_default(max_frames);
    // the speculative sync's critical path is a few runs of S (+ the lead-in)
    // bits, no longer ~7 serial rounds: shorter subsequences pay there.  One
    // FHD q90 JPEG end to end (profiles/r03_fhd420_jpeg_spec_sweep.json):
    // 0.65 ms at S = 512 / lead-in 512, 0.71 at 1024, 0.69-0.76 at 768.
    if (sub_bits == 0)
        sub_bits = spec && !tuning().sub_bits.is_set() ? kDefaultSubBits / 4 : default_sub_bits(max_frames);
    if (sub_bits < 32 || sub_bits > (1 << 20)) return set_error(HJD_E_INVALID, "sub_bits out of range [32, 2^20]");
    *out = nullptr;
    hjd_gdec* g = new (std::nothrow) hjd_gdec;
    if (!g) return set_error(HJD_E_NOMEM, "gdec allocation");
    g->ctx = ctx;
    g->device = hjd_ctx_device(ctx);
    g->num_cu = hjd_internal::ctx_num_cu(ctx);
    g->st.caps = make_caps(max_frames, max_scan_bytes, max_blocks, sub_bits);
    g->spec = spec;
    g->lead_hold = kLeadBatches;
    const int rc = gdec_alloc(g);
    if (rc) {
        hjd_gdec_destroy(g);
        return rc;
    }
    *out = g;
    return HJD_OK;
}

int hjd_gdec_destroy(hjd_gdec* g)
{
    if (!g) return HJD_OK;
    if (g->host_calls && tuning().gdec_host_times.get())
        fprintf(stderr, "hjd_gdec host us/call over %lld calls: wait_staging %.1f stage %.1f issue %.1f\n",
                static_cast<long long>(g->host_calls), g->host_us[0] / g->host_calls, g->host_us[1] / g->host_calls,
                g->host_us[2] / g->host_calls);
    (void)hipSetDevice(g->device);
    if (g->done) (void)hipEventSynchronize(g->done);
    while (!g->owned.empty()) g->release(g->owned.front().first);   // in the order they were allocated
    if (g->staged) (void)hipEventDestroy(g->staged);
    if (g->done) (void)hipEventDestroy(g->done);
    delete g;
    return HJD_OK;
}

int hjd_gdec_decode(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, void* const* d_outs,
                    const int32_t* pitches, void* stream)
{
    if (!d_outs) return set_error(HJD_E_INVALID, "d_outs is NULL");
    return decode_pixels(g, datas, sizes, n, nullptr, d_outs, pitches, stream);
}

int hjd_gdec_decode_roi(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, const hjd_rect* rois,
                        void* const* d_outs, const int32_t* pitches, void* stream)
{
    if (!d_outs) return set_error(HJD_E_INVALID, "d_outs is NULL");
    if (!rois) return set_error(HJD_E_INVALID, "rois is NULL");
    return decode_pixels(g, datas, sizes, n, rois, d_outs, pitches, stream);
}

int hjd_gdec_decode_coefs(hjd_gdec* g, const uint8_t* const* datas, const size_t* sizes, int n, int16_t* d_coefs,
                          int64_t* block_offsets, void* stream)
{
    if (!d_coefs || (reinterpret_cast<uintptr_t>(d_coefs) & 15))
        return set_error(HJD_E_INVALID, "d_coefs must be a 16-byte aligned device pointer");
    GdecCall c(datas, sizes, n, stream);
    c.coefs_out = d_coefs;
    c.block_offsets = block_offsets;
    return gdec_run(g, c);
}

int hjd_gdec_last_bytes(hjd_gdec* g, int64_t* host_scan_bytes, int64_t* h2d_bytes)
{
    if (!g) return set_error(HJD_E_INVALID, "gdec is NULL");
    if (host_scan_bytes) *host_scan_bytes = g->last_host_scan_bytes;
    if (h2d_bytes) *h2d_bytes = g->last_h2d;
    return HJD_OK;
}

int hjd_gdec_set_output_format(hjd_gdec* g, int out_format)
{
    if (!g) return set_error(HJD_E_INVALID, "gdec is NULL");
    if (!hjd_internal::out_format_bytes(out_format)) return set_error(HJD_E_INVALID, "unknown output format %d", out_format);
    g->out_format = out_format;   // applies to the next decode; an issued one keeps its format
    return HJD_OK;
}

int hjd_gdec_set_normalize(hjd_gdec* g, const float a[3], const float b[3])
{
    const int rc = hjd_internal::norm_check(a, b);
    if (rc) return rc;
    if (!g) return set_error(HJD_E_INVALID, "gdec is NULL");
    for (int c = 0; c < 3; ++c) {   // staged with the next call's records; an issued one keeps its own
        g->norm.a[c] = a[c];
        g->norm.b[c] = b[c];
    }
    return HJD_OK;
}

int hjd_gdec_set_scale(hjd_gdec* g, int scale)
{
    if (!g) return set_error(HJD_E_INVALID, "gdec is NULL");
    hjd_internal::DecodeShape shape;
    shape.scale = scale;
    int rc = hjd_internal::shape_check(shape);
    if (rc) return rc;
    g->scale = scale;   // applies to the next decode; an issued one keeps its scale
    return HJD_OK;
}

int hjd_gdec_sync(hjd_gdec* g, int32_t* status)
{
    if (!g) return set_error(HJD_E_INVALID, "gdec is NULL");
    if (!g->pending) return HJD_OK;
    HJD_HIP(hipSetDevice(g->device));
    HJD_HIP(hipEventSynchronize(g->done));
    for (size_t e = 0; e < g->st.scan_file.size(); ++e)   // a JPEG's further scans
        g->h_status[g->st.scan_file[e]] |= g->h_status[g->nframes_issued + e];
    int bad = 0;
    bool repaired = false;
    for (int i = 0; i < g->nframes_issued; ++i) {
        const uint32_t s = g->h_status[i] & ~kStatusFallback;
        if (status) status[i] = static_cast<int32_t>(g->h_status[i]);
        if (s) ++bad;
        repaired = repaired || (g->h_status[i] & kStatusFallback);
    }
    if (g->batch_spec) {   // the lead-in of the next batches (spec_lead_bits)
        if (repaired) {
            if (g->lead_stepped_down) g->lead_hold = std::min(2 * g->lead_hold, kLeadBatchesMax);
            g->lead_step = std::min(g->lead_step + 1, kLeadSteps - 1);
            g->lead_left = g->lead_hold;
            g->lead_stepped_down = false;
        } else {
            g->lead_stepped_down = false;
            if (g->lead_step && --g->lead_left == 0) {
                g->lead_left = --g->lead_step ? g->lead_hold : 0;
                g->lead_stepped_down = true;
            }
        }
    }
    g->pending = false;
    if (bad) return set_error(HJD_E_INVALID, "%d of %d frames had corrupt entropy data", bad, g->nframes_issued);
    return HJD_OK;
}

int hjd_debug_gdec_state(hjd_gdec* g, hjd_gdec_debug_state* out)
{
    if (!g || !out) return set_error(HJD_E_INVALID, "gdec or out is NULL");
    out->chain_epoch = g->chain_epoch;
    out->batch_spec = g->batch_spec;
    out->batch_lookback = g->batch_lookback;
    out->batch_chain_chunks = g->batch_chain_chunks;
    out->batch_sub_bits = g->batch_sub_bits ? g->batch_sub_bits : static_cast<uint32_t>(g->st.caps.sub_bits);
    out->batch_lead_bits = g->batch_lead;
    out->lead_step = g->lead_step;
    out->lead_left = g->lead_left;
    out->lead_hold = g->lead_hold;
    out->lead_stepped_down = g->lead_stepped_down;
    return HJD_OK;
}

// Only the host's counter: the words in d_chainfn keep their tags, and the
// next launch advances the counter as ever (gdec_issue), so the wrap a test
// reaches this way is the one 2^24 - 1 launches reach.
int hjd_debug_gdec_set_chain_epoch(hjd_gdec* g, uint32_t value)
{
    if (!g) return set_error(HJD_E_INVALID, "gdec is NULL");
    if (value > 0xFFFFFFu) return set_error(HJD_E_INVALID, "the look-back tag has 24 bits");
    if (g->pending) return set_error(HJD_E_STATE, "a call is pending: hjd_gdec_sync first");
    g->chain_epoch = value;
    return HJD_OK;
}

int hjd_host_register(void* ptr, size_t size)
{
    if (!ptr || !size) return set_error(HJD_E_INVALID, "NULL or empty host range");
    HJD_HIP(hipHostRegister(ptr, size, hipHostRegisterDefault));
    return HJD_OK;
}

int hjd_host_unregister(void* ptr)
{
    if (!ptr) return set_error(HJD_E_INVALID, "NULL host pointer");
    HJD_HIP(hipHostUnregister(ptr));
    return HJD_OK;
}

}  // extern "C"
