// hjd_gdec.hpp -- the GPU entropy decoder object (include/hjd_host.h hjd_gdec_*),
// private to hjd_gdec.hip, which owns it, hjd_gdec_post.hip, whose calls run
// stages behind its pixel kernels, and hjd_gstream.hip, whose slots stage into
// it and issue it.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "hjd.h"
#include "hjd_entropy_prep.hpp"
#include "hjd_internal.h"
#include "hjd_post.hpp"   // HJD_HIP

struct hjd_gdec {
    hjd_ctx* ctx = nullptr;
    int device = 0, num_cu = 256;
    hjd::ent::Staging st;               // the host side of the batch; st.h_stage is pinned
    hjd::ent::UploadPlan uploads;       // of the call being issued (kept for its storage: no allocation per call)
    // Every buffer of the decoder (st.h_stage and those below) comes from alloc(), which notes it here
    // (true: pinned host memory), so hjd_gdec_destroy frees this list and names none of them;
    // release() frees one early.
    std::vector<std::pair<void*, bool>> owned;
    template <class T> int alloc(T*& p, size_t bytes, bool host = false)
    {
        void* v = nullptr;
        HJD_HIP(host ? hipHostMalloc(&v, bytes, hipHostMallocDefault) : hipMalloc(&v, bytes));
        owned.emplace_back(v, host);
        p = static_cast<T*>(v);
        return HJD_OK;
    }
    void release(void* p)
    {
        for (size_t k = 0; k < owned.size(); ++k)
            if (owned[k].first == p) {
                (void)(owned[k].second ? hipHostFree(p) : hipFree(p));
                owned.erase(owned.begin() + static_cast<ptrdiff_t>(k));
                return;
            }
    }
    uint8_t* d_blob = nullptr;
    uint64_t* d_entries = nullptr;
    hjd::ent::SubStats* d_stats = nullptr;
    uint64_t* d_mids = nullptr;
    hjd::ent::SubStats* d_stats1 = nullptr;
    uint64_t* d_wentries = nullptr;
    uint32_t* d_linked = nullptr;
    hjd::ent::SubStats* d_agg = nullptr;
    uint32_t* h_status = nullptr;       // pinned; the device's status words are in the batch header (H.status)
    int16_t* d_coefs = nullptr;
    uint8_t* d_raw = nullptr;           // raw scan bytes of device-destuffed frames (same offsets as the data area)
    uint32_t* d_tiles = nullptr;        // destuff scratch [3][max_tiles]
    uint8_t* d_crops = nullptr;         // the scratch of a call with stages (hjd_gdec_post.hip): the crops the pixel
                                        // kernels write, then what one stage hands the next (oriented crops, the
                                        // antialiased filter's intermediates, the batch the colour, filter and tone stages
                                        // read, the filter stage's batch for a tone stage behind it, the colour
                                        // stage's partial sums, the tone stage's histograms and curves);
    size_t crops_bytes = 0;             // grow-only, (re)allocated by a call that needs more, behind the previous call
    bool spec = false;                  // speculative sync (latency decoders: ent_spec/cand/sync_spec kernels)
    hjd::ent::SpecRec* d_spec = nullptr;   // [max_subs][kMaxBpm]
    hjd::ent::CandRec* d_cand = nullptr;
    uint8_t* d_cmap = nullptr;
    uint8_t* d_cslot = nullptr;
    uint32_t* d_chainfn = nullptr;
    uint32_t* d_chain_broken = nullptr;
    hjd::ent::SubStats* d_agg2 = nullptr;   // [group] (ent_chain_lb_kernel)
    uint32_t chain_epoch = 0;           // the last launch's look-back tag
    int64_t chain_fn_rows = 0;          // capacity of d_chainfn in chunk functions
    uint8_t* d_steps = nullptr;         // [table][1 << kStepBits] (ent_steps_kernel)
    std::vector<uint8_t> steps_tabs;    // the tables d_steps was last derived from (host copy, batch order)
    double host_us[3] = {0, 0, 0};      // host time per phase (wait for staging, stage, issue): HJD_GDEC_HOST_TIMES
    int64_t host_calls = 0;
    hipEvent_t staged = nullptr, done = nullptr;
    int64_t last_h2d = 0;               // bytes the last issue moved host -> device
    int64_t last_host_scan_bytes = 0;   // scan bytes the host CPU read + wrote for the staged frames
    bool pending = false;
    bool staged_by_done = false;        // the last issue pulled its staging: `done` also means staged
    // the batch in flight (hjd_debug_gdec_state, hjd_gdec_sync)
    uint32_t batch_sub_bits = 0;        // its S (0: caps.sub_bits)
    bool batch_spec = false;            // it took the speculative sync
    bool batch_lookback = false;        // ... and ran ent_chain_lb_kernel
    uint32_t batch_chain_chunks = 0;    // its chain_chunks
    uint32_t batch_lead = 0;            // its lead-in in bits (0: round-based sync)
    int nframes_issued = 0;
    // the lead-in ladder (spec_lead_bits)
    uint32_t lead_step = 0;             // the ladder step for the next batch
    uint32_t lead_left = 0;             // clean batches before it steps down
    uint32_t lead_hold = 0;             // the clean run a step down waits for (kLeadBatches at first)
    bool lead_stepped_down = false;     // the batch in flight runs one step lower than the last
    int first_error = HJD_OK;
    // settings of the next calls
    int out_format = HJD_OUT_BGRX;      // pixel output format (hjd_gdec_set_output_format)
    int scale = 1;                      // decode scale of hjd_gdec_decode: 1, 2, 4 or 8 (hjd_gdec_set_scale)
    hjd_internal::NormRecord norm = hjd_internal::norm_identity();   // float formats (hjd_gdec_set_normalize)
};

namespace hjd {
namespace ent {

// D2H sink of one frame (hjd_gstream_submit_host): where its pixels go once decoded.
struct HostCopy {
    void* host;          // destination (pinned host memory recommended), or null
    int32_t host_pitch;
    int32_t width, height;
};

// What follows the pixel kernels of a call (hjd_gdec_post.hip).  Planar images in device memory:
// image i at ptrs[i], rows pitches[i] apart, dims[i].w x dims[i].h (x, y not read; null where nobody asks).
struct PostImages {
    void* const* ptrs;
    const int32_t* pitches;
    const hjd_rect* dims;
};

// One stage: its kind's launch (resize_aa: its two) over one record per image.  It reads `in` -- the
// images the pixel kernels wrote (the call's d_outs, HJD_OUT_RGB_PLANAR in the decoder's scratch), or
// the previous stage's outputs -- and knows no more of what preceded it.
enum class PostKind { orient, resize, resize_aa, warp, color, conv, tone };
struct PostStage {
    PostKind kind;
    PostImages in;
    int out_format;                // the decoder's, or (a stage follows) HJD_OUT_RGB_PLANAR
    PostImages out;                // orient: image i to out.ptrs[i] at out.pitches[i]
    struct { void* ptr; int w, h, pitch; } batch;   // resize, warp, color, conv, tone: image i to ptr + i * 3 * pitch * h
    const int32_t* orientations;   // orient: per image, 1..8
    const int32_t* flags;          // resize, warp: per image, or null
    void* const* mids;             // resize_aa: image i's intermediate (hjd_resize_aa.hpp) in the scratch
    const int32_t (*mats)[6];      // warp: per image, orientation composed, translation shifted to the crop
    const uint32_t* fills;         // warp: per image, or null
    int64_t tiles;                 // orient: the launch's tiles
    int max_h;                     // resize_aa: the tallest input, which sizes the horizontal launch
    const int32_t (*colors)[21];   // color: per image, m[9] p[9] t[3] (include/hjd.h)
    uint32_t* sums;                // color: the table of partial sums in the scratch, or null (every p is 0)
    const hjd_conv_filter* convs;  // conv: per image (include/hjd.h)
    const hjd_tone_curve* tones;   // tone: per image (include/hjd.h)
    uint32_t* hist;                // tone: the tables of partial histograms and of composed curves in the scratch,
    uint8_t* luts;                 // or null (every mode is 0)
    size_t recs_off, recs_bytes;   // its records in the batch header, from H.recs
};

// The stages of a call in launch order (orient -> resize or resize_aa -> color -> conv -> tone, or
// warp -> color -> conv -> tone, each optional), built once by its entry point.  Their records follow the pixel
// kernels' tables, each stage's at a 16-byte aligned offset.
struct PostPlan {
    int nstages;
    PostStage stage[5];
    size_t recs_bytes;             // the tables and every stage's records (Staging::assemble)
};

// One call of the decoder: everything that belongs to the call and not to
// the object.  gdec_run reads all of it; gdec_issue (frames already staged in
// g->st) all but datas, sizes and n.
struct GdecCall {
    GdecCall(const uint8_t* const* datas_ = nullptr, const size_t* sizes_ = nullptr, int n_ = 0, void* stream_ = nullptr)
        : datas(datas_), sizes(sizes_), n(n_), stream(static_cast<hipStream_t>(stream_)) {}
    const uint8_t* const* datas = nullptr;
    const size_t* sizes = nullptr;
    int n = 0;
    void* const* d_outs = nullptr;      // pixels (with pitches), or null: coefficients only
    const int32_t* pitches = nullptr;
    const hjd_rect* rois = nullptr;     // hjd_gdec_decode_roi: one rectangle per image
    int16_t* coefs_out = nullptr;       // null: the decoder's own buffer
    int64_t* block_offsets = nullptr;
    hipStream_t stream = nullptr;
    const HostCopy* host = nullptr;     // per frame, or null
    const PostPlan* post = nullptr;     // stages behind the pixel kernels, which then write planar bytes; or null
    // early pull of a latency decoder's lone image (gdec_early_pull)
    hjd_gdec* early_g = nullptr;        // non-null while the call's host destuff may pull
    size_t prepulled = 0;               // data-area bytes of frame 0 already pulled
};

// Upload the staged frames and run the entropy kernels (+ the pixel kernel
// when c.d_outs is given, + the stages of c.post) on c.stream.
int gdec_issue(hjd_gdec* g, GdecCall& c);

// Stage the call's JPEGs on the calling thread, then issue.
int gdec_run(hjd_gdec* g, GdecCall& c);

// Per-frame admission, the same for every hjd_gdec_decode* call: parse the file's header, check the
// rectangle (roi, map's of it, or neither: the whole scaled frame) against the frame, its sampling and
// the scale, and give the crop the pixel kernels will write -- or a refusal prefixed "frame i:".
// CropMapFn: a rectangle that depends on the stored frame's size at the decoder's scale, sw x sh.
typedef int (*CropMapFn)(const void* ctx, int i, int sw, int sh, const hjd_rect* roi, hjd_rect* crop);
struct Admit {
    int scale;              // the decoder's
    bool lenient;           // a file that is null or does not parse passes: staging refuses it in its own words
    const char* cap_fmt;    // a stage follows: its refusal of a crop above kResizeMaxDim (i, w, h, the cap); or null
    CropMapFn map;          // or null
    const void* ctx;
};
int admit_frame(const Admit& a, const uint8_t* data, size_t size, int i, const hjd_rect* roi, hjd_rect* crop);

// All gdec_issue asks of a call's stages besides plan.recs_bytes: write every stage's records into the
// staged header (with each *_item_check), and launch every stage on the stream behind the pixel kernels.
int post_write_records(hjd_gdec* g, const PostPlan& plan, int n);
int post_launch(hjd_gdec* g, const PostPlan& plan, int n, hipStream_t stream);

// Destuff mode of a JPEG and, for the device modes, its place in the raw
// area (PlanFn); with host_fallback, HJD_DESTUFF=auto picks the host path for
// a scan that does not fit instead (fits stays true).
int plan_raw(const Staging& st, const uint8_t* data, size_t size, RawCursor& cur, int& mode, uint64_t& raw_off,
             bool& fits, size_t data_room, uint64_t reserve, bool host_fallback);

// S of the stream's decoders (hjd_gstream_create).
int stream_sub_bits(int max_frames);

}  // namespace ent
}  // namespace hjd
