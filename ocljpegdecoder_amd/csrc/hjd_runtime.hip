// hjd_runtime.hip -- C-ABI runtime of the MI355X pixel back-end (include/hjd.h).
//
// Replaces the reference's OpenCL host runtime (src/oclDCT8x8.cpp:25-341):
// device selection, buffers, kernel selection per colour space and launch.
// Unlike the reference there is no file-static state here: contexts and plans
// are handles, so several images / frames / devices can be in flight.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <new>
#include <string>
#include <vector>

#include "hjd.h"
#include "hjd_internal.h"
#include "hjd_kernels.hpp"

using hjd::FrameDev;
using hjd_internal::DecodeShape;
using hjd_internal::SamplingGeom;
using hjd_internal::sampling_geom;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HJD_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(HJD_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),    \
                        __FILE__, __LINE__);                                                 \
    } while (0)

using hjd_internal::kZigzag;

}  // namespace

int hjd_internal::set_error(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int hjd_internal::norm_check(const float* a, const float* b)
{
    if (!a || !b) return set_error(HJD_E_INVALID, "normalisation constants: a or b is NULL");
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(a[c]) || !std::isfinite(b[c]))
            return set_error(HJD_E_INVALID, "normalisation constants must be finite (channel %d: a = %g, b = %g)", c,
                             static_cast<double>(a[c]), static_cast<double>(b[c]));
    return HJD_OK;
}

struct hjd_ctx {
    int device = 0;
    int num_cu = 256;
};

struct hjd_plan {
    hjd_ctx* ctx = nullptr;
    int input_format = 0;
    int sampling = -1;          // common sampling of all frames (kernel template)
    int nframes = 0;
    int64_t tasks = 0;
    int64_t pixels = 0;
    int64_t coef_bytes = 0;
    FrameDev* d_frames = nullptr;
    int* d_qt = nullptr;        // natural-order tables [nq][64]
    int variant = 0;            // kernel variant bits (hjd_plan_set_variant)
    int out_format = HJD_OUT_BGRX;   // common output format of all frames
    int kernel_mode = HJD_KERNEL_AUTO;
    int tuned_grid = 0;         // hjd_plan_autotune's / hjd_plan_set_chunk's grid (0: the shape default)
    int tuned_per_wave = 0;     // its tasks per wave
    int autotune_launches = 0;  // kernel launches of the last hjd_plan_autotune
    int autotune_cached = 0;    // 1: that call reused a cached choice
    int scale = 1;              // hjd_plan_create_scaled: 1, 2, 4 or 8
    int roi = 0;                // hjd_plan_create_roi with rectangles: the RoiDev table follows d_frames
    size_t norm_off = 0;        // float formats: byte offset of the NormDev record in d_frames (after both tables)
};

constexpr int64_t kDefaultLatencyMaxTasks = 1024;   // measured: profiles/r01_latency_kernel.json

// ---------------------------------------------------------------------------
// Tuning overrides.  kTuning is the list of them: the environment variable's
// name, the field of hjd_internal::Tuning it fills and how its string is
// parsed (a null string: the variable is not set).  The environment is read
// once, when tuning() is first called; hjd_debug_set_tuning() goes through the
// same rows.  "Per call" overrides act from the next call on a live object,
// "at create" ones on objects created after the change.
// ---------------------------------------------------------------------------
namespace {

using hjd_internal::kTuneUnset;
using hjd_internal::Tuning;

int64_t parse_int(const char* s) { return s ? atoi(s) : kTuneUnset; }
int64_t parse_lat_tasks(const char* s) { return s ? atoll(s) : kDefaultLatencyMaxTasks; }
int64_t parse_tasks_per_wave(const char* s) { return s ? atoll(s) : 0; }
int64_t parse_not_0(const char* s) { return !(s && s[0] == '0'); }           // on unless the value starts with 0
int64_t parse_present(const char* s) { return s != nullptr; }                // on when set, to anything
int64_t parse_flag(const char* s) { return s && *s && strcmp(s, "0") != 0; }   // on when set, not empty, not "0"
int64_t parse_destuff(const char* s)
{
    if (s && !strcmp(s, "host")) return hjd_internal::kPolicyHost;
    if (s && !strcmp(s, "device")) return hjd_internal::kPolicyDevice;
    return hjd_internal::kPolicyAuto;
}
int64_t parse_d16_probe(const char* s)
{
    if (s && !strcmp(s, "fail")) return hjd_internal::kProbeFail;
    if (s && !strcmp(s, "hipfail")) return hjd_internal::kProbeHipFail;
    return hjd_internal::kProbeRun;
}
int64_t parse_compat_copy(const char* s)   // idct_compat.hip CopyMode
{
    return s && !strcmp(s, "staged") ? 1 : s && !strcmp(s, "register") ? 2 : 0;
}

const struct TuneRow {
    const char* name;
    hjd_internal::TuneField Tuning::*field;
    int64_t (*parse)(const char*);
} kTuning[] = {
    // host | auto | device: where a scan's byte stuffing is removed.  Per call (each frame).
    {"HJD_DESTUFF", &Tuning::destuff, parse_destuff},
    // Lead-in bits of the speculative sync's runs, instead of the adaptive ladder.  Per call (each batch).
    {"HJD_SPEC_LEAD", &Tuning::spec_lead, parse_int},
    // Subsequence bits S of dense scans, instead of the tiers.  Per call (each batch).
    {"HJD_DENSE_SUB_BITS", &Tuning::dense_sub_bits, parse_int},
    // 0: the 4:4:4 kernels gather with v_perm even where the d16 probe passed.  Per call (each launch).
    {"HJD_D16", &Tuning::d16, parse_not_0},
    // 0: hjd_plan_autotune neither reads nor fills the process-wide cache.  Per call.
    {"HJD_AUTOTUNE_CACHE", &Tuning::autotune_cache, parse_not_0},
    // Subsequence bits S of GPU entropy decoders and streams created with sub_bits 0.  At create.
    {"HJD_SUB_BITS", &Tuning::sub_bits, parse_int},
    // 0 | 1: round-based or speculative sync, instead of the choice by max_frames.  At create; the
    // host emulation (off unless 1) takes it per call.
    {"HJD_SYNC_SPEC", &Tuning::sync_spec, parse_int},
    // Set: the host emulation prints its sync rounds and overflow levels.  Per call.
    {"HJD_EMU_ROUNDS", &Tuning::emu_rounds, parse_present},
    // Guessed block-in-MCU phases / bit offsets of hjd_debug_entropy_sync_check.  Per call.
    {"HJD_SYNC_PHASES", &Tuning::sync_phases, parse_int},
    {"HJD_SYNC_OFFSETS", &Tuning::sync_offsets, parse_int},
    // Set: hjd_gdec_destroy prints the decoder's host time per call.  At destroy.
    {"HJD_GDEC_HOST_TIMES", &Tuning::gdec_host_times, parse_present},
    // 0: a stream's workers and pinned staging are not bound to the GPU's NUMA node.  At create.
    {"HJD_NUMA", &Tuning::numa, parse_not_0},
    // 0: a stream worker takes one job at a time, not two interleaved.  At create (each worker's start).
    {"HJD_STREAM_PAIR", &Tuning::stream_pair, parse_not_0},
    // Most tasks an HJD_KERNEL_AUTO launch gives the latency kernel.  Per call (each launch).
    {"HJD_LAT_TASKS", &Tuning::lat_tasks, parse_lat_tasks},
    // > 0: tasks per wave of the throughput kernel, instead of the per-sampling default.  Per call.
    {"HJD_TASKS_PER_WAVE", &Tuning::tasks_per_wave, parse_tasks_per_wave},
    // fail | hipfail: the d16 probe reports a half-preserving part / its HIP calls fail.  At the
    // first hjd_ctx_create of a device (a completed probe is cached).
    {"HJD_D16_PROBE", &Tuning::d16_probe, parse_d16_probe},
    // idct.h shim: pageable | staged | register host copies; statistics line per image; the
    // reference's per-image teardown.  At create (each clidct_create).
    {"HJD_COMPAT_COPY", &Tuning::compat_copy, parse_compat_copy},
    {"HJD_COMPAT_STATS", &Tuning::compat_stats, parse_flag},
    {"HJD_COMPAT_TEARDOWN", &Tuning::compat_teardown, parse_flag},
};
constexpr size_t kTuningRows = sizeof(kTuning) / sizeof(kTuning[0]);

struct TuningState {
    Tuning now;
    int64_t start[kTuningRows];   // what the environment gave (hjd_debug_set_tuning(name, NULL))
    TuningState()
    {
        for (size_t i = 0; i < kTuningRows; ++i) {
            start[i] = kTuning[i].parse(getenv(kTuning[i].name));
            (now.*kTuning[i].field).v.store(start[i], std::memory_order_relaxed);
        }
    }
};
TuningState& tuning_state()
{
    static TuningState s;
    return s;
}

}  // namespace

const Tuning& hjd_internal::tuning() { return tuning_state().now; }

extern "C" int hjd_debug_set_tuning(const char* name, const char* value)
{
    TuningState& s = tuning_state();
    for (size_t i = 0; name && i < kTuningRows; ++i)
        if (!strcmp(name, kTuning[i].name)) {
            (s.now.*kTuning[i].field).v.store(value ? kTuning[i].parse(value) : s.start[i], std::memory_order_relaxed);
            return HJD_OK;
        }
    return fail(HJD_E_INVALID, "hjd_debug_set_tuning: no override named %s", name ? name : "(null)");
}

// Launches of at most this many tasks take the latency kernel (one workgroup
// per task) in HJD_KERNEL_AUTO mode; HJD_LAT_TASKS overrides it (tuning).
static int64_t latency_max_tasks() { return hjd_internal::tuning().lat_tasks.get(); }

// The 4:4:4 kernels gather coefficient pairs with ds_read_u16_d16_hi
// (hjd::kVarD16), which relies on d16 LDS loads zeroing the other half of
// the register.  MI355X as deployed (sramecc+) does that
// (profiles/r03_d16_probe.txt); a half-preserving part would corrupt the
// pairs.  So the variant is taken only where the one-wave hardware probe
// (hjd_probe.hip, run by hjd_ctx_create) completed and saw every lane's low
// half zeroed; the v_perm kernels are the fallback.  HJD_D16=0 forces the
// fallback (A/B); nothing forces the d16 kernels onto a part the probe did not
// pass.  Launches only read the cached answer.
bool hjd_internal::d16_gather_selected(int device)
{
    if (!tuning().d16.get()) return false;
    return device >= 0 && hjd_internal::d16_probe_cached(device) == 1;
}

static int geometry(int width, int height, int sampling, int& mcu_w, int& mcu_h, int& bpm, int& tasks_mcus);
static int64_t default_per_wave(int sampling, int fmt);
static int grid_for_chunk(int64_t tasks, int64_t per_wave, bool occupancy_floor = true);

int hjd_internal::ctx_num_cu(const hjd_ctx* ctx) { return ctx->num_cu; }

// A shape as shape_check takes it, with the default kernel mode and no variant.
static DecodeShape make_shape(int sampling, int scale, int input_format = HJD_IN_Q16_ZIGZAG,
                                            int out_format = HJD_OUT_BGRX, bool roi = false)
{
    DecodeShape s;
    s.sampling = sampling;
    s.scale = scale;
    s.input_format = input_format;
    s.out_format = out_format;
    s.roi = roi;
    return s;
}

// The ROI's task set: MCU rows myf..myl times the strips
// that cover MCU columns mxf..mxl, anchored at mxf.
int hjd_internal::roi_geom(int width, int height, int sampling, int scale, const hjd_rect* roi, RoiGeom* g)
{
    int mw, mh, bpm, tasks_mcus;
    int rc = geometry(width, height, sampling, mw, mh, bpm, tasks_mcus);
    if (rc) return rc;
    if ((rc = shape_check(make_shape(sampling, scale)))) return rc;
    const int lg = scale_log2(scale);
    if (!roi || !g) return set_error(HJD_E_INVALID, "roi is NULL");
    const int sw = scaled_dim(width, scale), sh = scaled_dim(height, scale);
    if (roi->w < 1 || roi->h < 1)
        return set_error(HJD_E_INVALID, "roi (%d,%d,%d,%d): empty rectangle (w, h >= 1)", roi->x, roi->y, roi->w, roi->h);
    if (roi->x < 0 || roi->y < 0)
        return set_error(HJD_E_INVALID, "roi (%d,%d,%d,%d): negative origin", roi->x, roi->y, roi->w, roi->h);
    if (static_cast<int64_t>(roi->x) + roi->w > sw || static_cast<int64_t>(roi->y) + roi->h > sh)
        return set_error(HJD_E_INVALID, "roi (%d,%d,%d,%d) reaches past the %dx%d output grid", roi->x, roi->y, roi->w,
                         roi->h, sw, sh);
    SamplingGeom sg;
    sampling_geom(sampling, &sg);
    const int pw = sg.mcu_px_w >> lg, ph = sg.mcu_px_h >> lg;   // MCU size on the output grid
    g->mxf = roi->x / pw;
    g->myf = roi->y / ph;
    const int mxl = (roi->x + roi->w - 1) / pw, myl = (roi->y + roi->h - 1) / ph;
    g->strips = (mxl - g->mxf + 1 + tasks_mcus - 1) / tasks_mcus;
    g->rows = myl - g->myf + 1;
    g->dx = roi->x - g->mxf * pw;
    g->dy = roi->y - g->myf * ph;
    g->mcu_w = mw;
    g->rem_w = mw - g->mxf;
    g->bpm = bpm;
    g->tasks = static_cast<int64_t>(g->strips) * g->rows;
    g->blocks = static_cast<int64_t>(g->rows) * std::min(g->strips * tasks_mcus, g->rem_w) * bpm;
    return HJD_OK;
}

// Re-anchor a whole-frame record at the ROI's first MCU (hjd::RoiDev).
// d.out_base and d.pitch already describe the ROI's own destination.
static void apply_roi(FrameDev& d, hjd_internal::RoiRecord& side, const hjd_internal::RoiGeom& g, const hjd_rect& roi,
                      int out_format, uintptr_t base_bits)
{
    d.coef_base += (static_cast<int64_t>(g.myf) * g.mcu_w + g.mxf) * g.bpm;
    d.out_base -= static_cast<int64_t>(g.dy) * d.pitch +
                  static_cast<int64_t>(g.dx) * hjd_internal::out_format_row_bytes(out_format);
    d.width = g.dx + roi.w;
    d.height = g.dy + roi.h;
    d.mcu_w = g.rem_w;
    d.strips = g.strips;
    d.vec_ok = hjd_internal::out_vector_ok(out_format, d.pitch, d.out_base, base_bits) ? 1 : 0;
    side.row_stride = g.mcu_w;
    side.dx = g.dx;
    side.dy = g.dy;
    side.reserved = 0;
}

int64_t hjd_internal::make_frame_record(int width, int height, int sampling, int64_t coef_base, int64_t out_base,
                                        int pitch, const int qt_index[3], FrameRecord* rec, int out_format,
                                        uintptr_t base_bits, int scale, const hjd_rect* roi, RoiRecord* side)
{
    int mw, mh, bpm, tasks_mcus;
    int rc = geometry(width, height, sampling, mw, mh, bpm, tasks_mcus);
    if (rc) return rc;
    if ((rc = shape_check(make_shape(sampling, scale)))) return rc;
    if (pitch > kMaxOutPitch)   // every caller's records: plans, the GPU decoder, the stream pipeline
        return set_error(HJD_E_INVALID, "out_pitch %d is above HJD_MAX_OUT_PITCH (%d)", pitch, kMaxOutPitch);
    static_assert(sizeof(FrameRecord) == sizeof(FrameDev), "record layout");
    FrameDev d;
    memset(&d, 0, sizeof(d));
    d.coef_base = coef_base;
    d.out_base = out_base;
    d.task_begin = 0;
    d.width = scaled_dim(width, scale);
    d.height = scaled_dim(height, scale);
    d.pitch = pitch;
    d.sampling = sampling;
    d.mcu_w = mw;
    d.strips = (mw + tasks_mcus - 1) / tasks_mcus;
    for (int c = 0; c < 3; ++c) d.qt[c] = qt_index ? qt_index[c] : 0;
    d.vec_ok = out_vector_ok(out_format, pitch, out_base, base_bits) ? 1 : 0;
    if (roi) {
        RoiGeom g;
        if (!side) return set_error(HJD_E_INVALID, "a ROI record needs its side record");
        rc = roi_geom(width, height, sampling, scale, roi, &g);
        if (rc) return rc;
        apply_roi(d, *side, g, *roi, out_format, base_bits);
        mh = g.rows;
    }
    memcpy(rec, &d, sizeof(d));
    return static_cast<int64_t>(d.strips) * mh;
}

// ---------------------------------------------------------------------------
// The fused pixel kernel's launch: which shapes are legal
// (shape_check), the table of every decode_kernel / decode_kernel_lat the
// library instantiates, keyed by its template arguments, and the selection of
// one entry for a shape (select_key).
// ---------------------------------------------------------------------------
// A shape takes the latency kernel (one workgroup per task): on request, or a
// small HJD_KERNEL_AUTO launch of whole full-size frames with the default grid.
static bool takes_latency(const DecodeShape& s)
{
    return s.stages == 0 && s.scale == 1 && !s.roi &&
           (s.kernel_mode == HJD_KERNEL_LATENCY ||
            (s.kernel_mode == HJD_KERNEL_AUTO && s.grid_blocks == 0 && s.tasks <= latency_max_tasks()));
}

int hjd_internal::shape_check(const DecodeShape& s)
{
    const int lg = scale_log2(s.scale);
    const bool i32 = s.input_format == HJD_IN_I32_NATURAL;
    const bool whole = lg == 0 && !s.roi;   // whole frames at full size
    SamplingGeom sg;
    if (lg < 0) return set_error(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", s.scale);
    if (s.input_format != HJD_IN_Q16_ZIGZAG && !i32)
        return set_error(HJD_E_INVALID, "unknown input format %d", s.input_format);
    if (!whole && i32)
        return set_error(HJD_E_INVALID, "scaled and ROI decode take HJD_IN_Q16_ZIGZAG input, not HJD_IN_I32_NATURAL");
    if (!out_format_bytes(s.out_format)) return set_error(HJD_E_INVALID, "unknown output format %d", s.out_format);
    if (out_format_float_bytes(s.out_format) && i32)
        return set_error(HJD_E_INVALID, "the float output formats take HJD_IN_Q16_ZIGZAG input, not HJD_IN_I32_NATURAL");
    if (!sampling_geom(s.sampling, &sg))
        return set_error(HJD_E_INVALID, "unsupported sampling %d (4:4:4, 4:2:0, 4:2:2, gray, 4:1:1 or 4:4:0)",
                         s.sampling);
    if (lg > 0 && !scaled_sampling_ok(s.sampling))
        return set_error(HJD_E_INVALID,
                         "scaled decode (scale %d) serves 4:4:4, 4:2:0 and gray, not 4:2:2, 4:1:1 or 4:4:0 (sampling %d)",
                         s.scale, s.sampling);
    if (s.variant < 0 || s.variant > 3) return set_error(HJD_E_INVALID, "unknown kernel variant %d", s.variant);
    // the latency kernels ignore the variant bits, so a byte format passes with them where the launch takes one
    if (s.variant != 0 && s.out_format != HJD_OUT_BGRX && (out_format_float_bytes(s.out_format) || !takes_latency(s)))
        return set_error(HJD_E_INVALID, "kernel variants are BGRX-only");
    if (s.variant != 0 && !whole) return set_error(HJD_E_INVALID, "scaled and ROI decode have no kernel variants");
    if (s.kernel_mode != HJD_KERNEL_AUTO && s.kernel_mode != HJD_KERNEL_PERSISTENT && s.kernel_mode != HJD_KERNEL_LATENCY)
        return set_error(HJD_E_INVALID, "unknown kernel mode %d", s.kernel_mode);
    if (s.kernel_mode == HJD_KERNEL_LATENCY && !whole)
        return set_error(HJD_E_INVALID, "scaled and ROI decode have no latency kernel");
    if (s.stages != 0) {   // the stage-skipping measurement variants
        constexpr int kStages[8] = {4, 8, 16, 20, 24, 64, 80, 256};
        if (std::find(kStages, kStages + 8, s.stages) == kStages + 8)
            return set_error(HJD_E_INVALID, "unknown stage variant %d", s.stages);
        if (!whole) return set_error(HJD_E_INVALID, "stage variants are not built for scaled and ROI plans");
        if (i32 || s.out_format != HJD_OUT_BGRX || sg.index > 1 || s.variant != 0)
            return set_error(HJD_E_INVALID, "stage variants: 4:2:0 / 4:4:4, int16 zigzag in, BGRX out, variant 0");
    }
    return HJD_OK;
}

namespace {

// The kernels' variant bits of each output format, beside hjd_internal::kOutFormats.
constexpr int kOutKernelBits[] = {0,  hjd::kOutBgr24, hjd::kOutRgb24, hjd::kOutPlanar,
                                  -1, hjd::kOutPlanar | hjd::kOutF16, hjd::kOutPlanar | hjd::kOutF32};
static_assert(sizeof(kOutKernelBits) / sizeof(int) == hjd_internal::kOutFormatRows, "one entry per HJD_OUT_* value");

using KLat = void (*)(const void*, const int*, const FrameDev*, int, int64_t, uint8_t*);
using KPer = void (*)(const void*, const int*, const FrameDev*, int, int64_t, uint8_t*, int64_t, int64_t);
struct KernelEntry {
    int key[4];   // latency, S, F, V: decode_kernel_lat<S, F, V> or decode_kernel<S, F, V>
    KLat lat;
    KPer per;
    bool operator<(const KernelEntry& o) const { return std::lexicographical_compare(key, key + 4, o.key, o.key + 4); }
};

// Every pixel kernel of the library, named once.  P / L make a persistent / a
// latency entry whose key is the template arguments its pointer is taken with.
#define P(S, F, V) {{0, S, F, (V)}, nullptr, hjd::decode_kernel<S, F, (V)>},
#define L(S, F, V) {{1, S, F, (V)}, hjd::decode_kernel_lat<S, F, (V)>, nullptr},
#define ALL6(M, F, V) M(0, F, V) M(1, F, V) M(2, F, V) M(3, F, V) M(4, F, V) M(5, F, V)
#define SCALED1(M, V) M(0, 0, V) M(1, 0, V) M(3, 0, V)   // 4:4:4, 4:2:0 and gray
#define SCALED(V) SCALED1(P, (V) | (1 << hjd::kScaleShift)) SCALED1(P, (V) | (2 << hjd::kScaleShift)) \
                  SCALED1(P, (V) | (3 << hjd::kScaleShift))
// One output format (bits O) with int16 input: whole frames, persistent (its
// 4:4:4 d16 twin) and latency; scaled; ROI at scale 1 and scaled.  37 kernels.
#define FORMAT(O) ALL6(P, 0, O) P(0, 0, (O) | hjd::kVarD16) ALL6(L, 0, O) SCALED(O) ALL6(P, 0, (O) | hjd::kVarRoi) \
                  SCALED((O) | hjd::kVarRoi)
#define FORMAT_I32(O) ALL6(P, 1, O) ALL6(L, 1, O)   // int32 input: whole frames only.  12 kernels.
#define STAGES(S, D) P(S, 0, 4 | (D)) P(S, 0, 8 | (D)) P(S, 0, 16 | (D)) P(S, 0, 20 | (D)) P(S, 0, 24 | (D)) \
                     P(S, 0, 64 | (D)) P(S, 0, 80 | (D)) P(S, 0, 256 | (D))
const KernelEntry kKernelList[] = {
    FORMAT(0) FORMAT(hjd::kOutBgr24) FORMAT(hjd::kOutRgb24) FORMAT(hjd::kOutPlanar)
    FORMAT(hjd::kOutPlanar | hjd::kOutF16) FORMAT(hjd::kOutPlanar | hjd::kOutF32)
    FORMAT_I32(0) FORMAT_I32(hjd::kOutBgr24) FORMAT_I32(hjd::kOutRgb24) FORMAT_I32(hjd::kOutPlanar)
    // BGRX kernel variants (hjd_plan_set_variant), both inputs; the d16 twin keeps the store bit
    ALL6(P, 0, 1) ALL6(P, 0, 2) ALL6(P, 0, 3) ALL6(P, 1, 1) ALL6(P, 1, 2) ALL6(P, 1, 3)
    P(0, 0, hjd::kVarPlainStores | hjd::kVarD16)
    // stage-skipping measurement variants: 4:2:0, 4:4:4 and its d16 twin
    STAGES(1, 0) STAGES(0, 0) STAGES(0, hjd::kVarD16)
};
#undef STAGES
#undef FORMAT_I32
#undef FORMAT
#undef SCALED
#undef SCALED1
#undef ALL6
#undef L
#undef P
constexpr int kKernels = sizeof(kKernelList) / sizeof(kKernelList[0]);
static_assert(kKernels == 6 * 37 + 4 * 12 + 37 + 24, "331 pixel kernels");

// The table sorted by key (once, at its first use).
const KernelEntry* kernel_table()
{
    static const std::vector<KernelEntry> sorted = [] {
        std::vector<KernelEntry> t(kKernelList, kKernelList + kKernels);
        std::sort(t.begin(), t.end());
        return t;
    }();
    return sorted.data();
}

// The table entry a shape takes (HJD_OK), or HJD_E_INVALID.  d16: whether the
// 4:4:4 kernels gather with d16 loads; < 0: as d16_gather_selected(device) says.
int select_kernel(const DecodeShape& s, int d16, int device, const KernelEntry** out)
{
    int rc = hjd_internal::shape_check(s);
    if (rc) return rc;
    SamplingGeom sg;
    sampling_geom(s.sampling, &sg);
    KernelEntry want = {{takes_latency(s), sg.index, s.input_format == HJD_IN_Q16_ZIGZAG ? 0 : 1,
                         kOutKernelBits[s.out_format]}, nullptr, nullptr};
    int& V = want.key[3];
    if (want.key[0]) {   // the latency kernels have no variants: bits 0-1 are ignored
        if (s.tasks > INT32_MAX) return hjd_internal::set_error(HJD_E_INVALID, "too many tasks for the latency kernel");
    } else {
        V |= (hjd_internal::scale_log2(s.scale) << hjd::kScaleShift) | (s.roi ? hjd::kVarRoi : 0) | s.variant | s.stages;
        // the d16 twin: 4:4:4 whole frames from int16 input, contiguous task order
        if (s.sampling == HJD_YUV444 && want.key[2] == 0 && s.scale == 1 && !s.roi &&
            (s.variant & hjd::kVarWgInterleave) == 0 && (d16 < 0 ? hjd_internal::d16_gather_selected(device) : d16 != 0))
            V |= hjd::kVarD16;
    }
    const KernelEntry* t = kernel_table();
    const KernelEntry* e = std::lower_bound(t, t + kKernels, want);
    if (e == t + kKernels || want < *e)
        return hjd_internal::set_error(HJD_E_INVALID,
                                       "no %s kernel <%d, %d, %d> for sampling %d, input format %d, output format %d, "
                                       "scale %d, roi %d, variant %d, stages %d",
                                       want.key[0] ? "latency" : "persistent", want.key[1], want.key[2], V, s.sampling,
                                       s.input_format, s.out_format, s.scale, s.roi, s.variant, s.stages);
    *out = e;
    return HJD_OK;
}

}  // namespace

int hjd_internal::launch_decode(const DecodeLaunch& l)
{
    HJD_HIP(hipSetDevice(l.device));
    const KernelEntry* k;
    int rc = select_kernel(l, -1, l.device, &k);
    if (rc) return rc;
    hipStream_t stream = static_cast<hipStream_t>(l.stream);
    const FrameDev* frames = reinterpret_cast<const FrameDev*>(l.d_frames);
    uint8_t* out = static_cast<uint8_t*>(l.d_out);
    if (k->lat) {
        hipLaunchKernelGGL(k->lat, dim3(static_cast<uint32_t>(l.tasks)), dim3(hjd::kLatThreads), 0, stream, l.d_coefs,
                           l.d_qt_nat, frames, l.nframes, l.tasks, out);
    } else {
        const int fmt = k->key[2];
        const int grid = l.grid_blocks > 0 ? l.grid_blocks : grid_for_chunk(l.tasks, default_per_wave(l.sampling, fmt));
        // the task split of the persistent kernels (see decode_kernel): default
        // order over grid * 4 waves, wg-interleave over grid groups of 4-task quads
        const bool quads = (l.variant & hjd::kVarWgInterleave) != 0;
        const int64_t split_n = quads ? static_cast<int64_t>(grid) : static_cast<int64_t>(grid) * hjd::kWavesPerGroup;
        const int64_t split_t = quads ? (l.tasks + hjd::kWavesPerGroup - 1) / hjd::kWavesPerGroup : l.tasks;
        hipLaunchKernelGGL(k->per, dim3(grid), dim3(hjd::kGroupThreads), 0, stream, l.d_coefs, l.d_qt_nat, frames,
                           l.nframes, l.tasks, out, split_t / split_n, split_t % split_n);
    }
    HJD_HIP(hipGetLastError());
    return HJD_OK;
}

extern "C" {

int hjd_abi_version(void) { return HJD_ABI_VERSION; }

const char* hjd_last_error(void) { return g_last_error.c_str(); }

int hjd_device_count(int* count)
{
    if (!count) return fail(HJD_E_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        if (e == hipErrorNoDevice) return HJD_OK;
        return fail(HJD_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return HJD_OK;
}

int hjd_ctx_create(int device, hjd_ctx** out)
{
    if (!out) return fail(HJD_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    int rc = hjd_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return fail(HJD_E_NO_DEVICE, "device %d not present (%d devices)", device, n);
    HJD_HIP(hipSetDevice(device));
    hjd_ctx* c = new (std::nothrow) hjd_ctx;
    if (!c) return fail(HJD_E_NOMEM, "context allocation");
    c->device = device;
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0)
        c->num_cu = cu;
    // the d16 gather probe runs here, once per device, so that no launch (which
    // may be inside a stream capture) ever has to run it; a failed probe leaves
    // no HIP error behind and the launches use the v_perm kernels
    (void)hjd_internal::d16_probe(device);
    *out = c;
    return HJD_OK;
}

int hjd_ctx_destroy(hjd_ctx* ctx)
{
    delete ctx;
    return HJD_OK;
}

int hjd_ctx_device(const hjd_ctx* ctx) { return ctx ? ctx->device : -1; }

static int geometry(int width, int height, int sampling, int& mcu_w, int& mcu_h, int& bpm, int& tasks_mcus)
{
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535)
        return fail(HJD_E_INVALID, "invalid dimensions %dx%d", width, height);
    SamplingGeom g;
    if (!sampling_geom(sampling, &g))
        return fail(HJD_E_INVALID, "unsupported sampling %d (4:4:4, 4:2:0, 4:2:2, gray, 4:1:1 or 4:4:0)",
                    sampling);
    bpm = g.bpm;
    tasks_mcus = g.mcus_per_task;
    mcu_w = (width - 1) / g.mcu_px_w + 1;   // src/decoder.cpp:189-190
    mcu_h = (height - 1) / g.mcu_px_h + 1;
    return HJD_OK;
}

int hjd_frame_blocks(int width, int height, int sampling, int64_t* nblocks)
{
    int mw, mh, bpm, tasks_mcus;
    int rc = geometry(width, height, sampling, mw, mh, bpm, tasks_mcus);
    if (rc) return rc;
    if (!nblocks) return fail(HJD_E_INVALID, "nblocks is NULL");
    *nblocks = static_cast<int64_t>(mw) * mh * bpm;
    return HJD_OK;
}

int hjd_scaled_size(int width, int height, int scale, int* out_w, int* out_h)
{
    int rc = hjd_internal::shape_check(make_shape(HJD_YUV420, scale));
    if (rc) return rc;
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535)
        return fail(HJD_E_INVALID, "invalid dimensions %dx%d", width, height);
    if (!out_w || !out_h) return fail(HJD_E_INVALID, "out_w or out_h is NULL");
    *out_w = hjd_internal::scaled_dim(width, scale);
    *out_h = hjd_internal::scaled_dim(height, scale);
    return HJD_OK;
}

int hjd_roi_geometry(int width, int height, int sampling, int scale, const hjd_rect* roi, int64_t* tasks,
                     int64_t* blocks)
{
    hjd_internal::RoiGeom g;
    int rc = hjd_internal::roi_geom(width, height, sampling, scale, roi, &g);
    if (rc) return rc;
    if (tasks) *tasks = g.tasks;
    if (blocks) *blocks = g.blocks;
    return HJD_OK;
}

// One frame of a plan of the checked shape `s` whose first frame is `first`:
// valid dimensions, the plan's sampling and output format, a sampling the
// shape serves, a valid rectangle, and a pitch and offset that fit what the
// frame writes (the ROI's size, else the scaled frame's).  pixels, blocks:
// what it writes and reads.  i: the frame's index, for the message.
static int check_frame(const hjd_frame& f, const hjd_frame& first, DecodeShape s, const hjd_rect* roi,
                       int i, int64_t* pixels, int64_t* blocks)
{
    int mw, mh, bpm, tasks_mcus;
    int rc = geometry(f.width, f.height, f.sampling, mw, mh, bpm, tasks_mcus);
    if (rc) return fail(rc, "frame %d: %s", i, std::string(g_last_error).c_str());
    if (f.sampling != first.sampling)
        return fail(HJD_E_INVALID, "frame %d: mixed sampling in one plan (use one plan per sampling)", i);
    if (f.out_format != first.out_format)
        return fail(HJD_E_INVALID, "frame %d: mixed output formats in one plan (use one plan per format)", i);
    hjd_internal::RoiGeom rg;
    s.sampling = f.sampling;
    rc = hjd_internal::shape_check(s);
    if (!rc && roi) rc = hjd_internal::roi_geom(f.width, f.height, f.sampling, s.scale, roi, &rg);
    if (rc) return fail(rc, "frame %d: %s", i, std::string(g_last_error).c_str());
    // the output is the ROI where there is one: pitch and payload refer to it
    const int sw = roi ? roi->w : hjd_internal::scaled_dim(f.width, s.scale);
    const int sh = roi ? roi->h : hjd_internal::scaled_dim(f.height, s.scale);
    const uint64_t amask = static_cast<uint64_t>(hjd_internal::out_format_pitch_mask(f.out_format));
    if (f.out_pitch < static_cast<int64_t>(hjd_internal::out_format_row_bytes(f.out_format)) * sw ||
        (f.out_pitch & amask) || (f.out_offset & amask))
        return fail(HJD_E_INVALID, "frame %d: bad output pitch/offset", i);
    if (f.out_pitch > hjd_internal::kMaxOutPitch)   // (the kernel's 32-bit lane offset: hjd_internal.h)
        return fail(HJD_E_INVALID, "frame %d: out_pitch %d is above HJD_MAX_OUT_PITCH (%d)", i, f.out_pitch,
                    hjd_internal::kMaxOutPitch);
    *pixels = static_cast<int64_t>(sw) * sh;
    *blocks = roi ? rg.blocks : static_cast<int64_t>(mw) * mh * bpm;
    return HJD_OK;
}

int hjd_frame_check(const hjd_frame* frame, int input_format, int scale, const hjd_rect* roi)
{
    if (!frame) return fail(HJD_E_INVALID, "frame is NULL");
    // the plan's rules first, on 4:2:0, which every shape serves; check_frame adds the frame's sampling
    const DecodeShape shape = make_shape(HJD_YUV420, scale, input_format, frame->out_format, roi != nullptr);
    int rc = hjd_internal::shape_check(shape);
    if (rc) return rc;
    int64_t pixels, blocks;
    return check_frame(*frame, *frame, shape, roi, 0, &pixels, &blocks);
}

int hjd_plan_create(hjd_ctx* ctx, const hjd_frame* frames, int nframes, int input_format,
                    const int32_t* qtables, int nq, hjd_plan** out)
{
    return hjd_plan_create_roi(ctx, frames, nframes, input_format, qtables, nq, 1, nullptr, out);
}

int hjd_plan_create_scaled(hjd_ctx* ctx, const hjd_frame* frames, int nframes, int input_format,
                           const int32_t* qtables, int nq, int scale, hjd_plan** out)
{
    return hjd_plan_create_roi(ctx, frames, nframes, input_format, qtables, nq, scale, nullptr, out);
}

int hjd_plan_create_roi(hjd_ctx* ctx, const hjd_frame* frames, int nframes, int input_format,
                        const int32_t* qtables, int nq, int scale, const hjd_rect* rois, hjd_plan** out)
{
    if (!ctx || !out || (!frames && nframes > 0) || nframes < 0)
        return fail(HJD_E_INVALID, "invalid plan arguments");
    *out = nullptr;
    const bool q16 = input_format == HJD_IN_Q16_ZIGZAG;
    int sampling = nframes > 0 ? frames[0].sampling : HJD_YUV420;
    const int out_format = nframes > 0 ? frames[0].out_format : HJD_OUT_BGRX;
    // the plan's rules first, on 4:2:0, which every shape serves; check_frame adds each frame's sampling
    const DecodeShape shape = make_shape(HJD_YUV420, scale, input_format, out_format, rois != nullptr);
    int rc = hjd_internal::shape_check(shape);
    if (rc) return rc;
    if (q16 && (!qtables || nq <= 0)) return fail(HJD_E_INVALID, "quantisation tables required for HJD_IN_Q16_ZIGZAG");

    std::vector<hjd_internal::FrameRecord> fd(static_cast<size_t>(std::max(nframes, 1)));
    std::vector<hjd_internal::RoiRecord> sides(rois ? fd.size() : 0);
    int64_t tasks = 0, pixels = 0, blocks = 0;
    for (int i = 0; i < nframes; ++i) {
        const hjd_frame& f = frames[i];
        int64_t fpixels, fblocks;
        rc = check_frame(f, frames[0], shape, rois ? &rois[i] : nullptr, i, &fpixels, &fblocks);
        if (rc) return rc;
        for (int c = 0; q16 && c < 3; ++c)
            if (f.qt_index[c] < 0 || f.qt_index[c] >= nq)
                return fail(HJD_E_INVALID, "frame %d: qt_index[%d]=%d out of range", i, c, f.qt_index[c]);
        const int64_t t = hjd_internal::make_frame_record(
            f.width, f.height, f.sampling, static_cast<int64_t>(f.coef_offset), static_cast<int64_t>(f.out_offset),
            f.out_pitch, q16 ? f.qt_index : nullptr, &fd[i], out_format, 0, scale, rois ? &rois[i] : nullptr,
            rois ? &sides[i] : nullptr);
        if (t < 0) return static_cast<int>(t);
        fd[i].task_begin = tasks;
        tasks += t;
        pixels += fpixels;
        blocks += fblocks;
    }

    HJD_HIP(hipSetDevice(ctx->device));
    hjd_plan* p = new (std::nothrow) hjd_plan;
    if (!p) return fail(HJD_E_NOMEM, "plan allocation");
    p->ctx = ctx;
    p->input_format = input_format;
    p->sampling = sampling;
    p->out_format = out_format;
    p->scale = scale;
    p->roi = rois ? 1 : 0;
    p->nframes = nframes;
    p->tasks = tasks;
    p->pixels = pixels;
    p->coef_bytes = blocks * (input_format == HJD_IN_Q16_ZIGZAG ? 128 : 256);

    // qtables: file (zigzag) order -> natural order, so a lane reads its row's
    // 8 factors contiguously.
    const int nqt = input_format == HJD_IN_Q16_ZIGZAG ? nq : 1;
    std::vector<int32_t> qnat(static_cast<size_t>(nqt) * 64, 0);
    if (input_format == HJD_IN_Q16_ZIGZAG)
        for (int t = 0; t < nq; ++t)
            for (int k = 0; k < 64; ++k) qnat[t * 64 + kZigzag[k]] = qtables[t * 64 + k];

    // the frame table (hjd_internal::frame_table): a ROI plan's RoiDev table follows the nframes
    // records, a float plan's NormDev record both; a = 1, b = 0 until hjd_plan_set_normalize
    static_assert(sizeof(hjd_internal::FrameRecord) == sizeof(FrameDev), "frame record layout");
    static_assert(sizeof(hjd_internal::RoiRecord) == sizeof(hjd::RoiDev), "side record layout");
    const bool norm = hjd_internal::out_format_float_bytes(out_format) != 0;
    const hjd_internal::FrameTable tab = hjd_internal::frame_table(nframes, rois != nullptr, norm);
    p->norm_off = norm ? tab.norm : 0;
    const hjd_internal::NormRecord ident = hjd_internal::norm_identity();
    // (an empty plan still holds fd's one record)
    hipError_t e = hipMalloc(&p->d_frames,
                             hjd_internal::frame_table(static_cast<int>(fd.size()), rois != nullptr, norm).bytes);
    if (e == hipSuccess) e = hipMalloc(&p->d_qt, qnat.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(p->d_frames, fd.data(), fd.size() * sizeof(FrameDev), hipMemcpyHostToDevice);
    if (e == hipSuccess && rois && nframes > 0)
        e = hipMemcpy(reinterpret_cast<char*>(p->d_frames) + tab.side, sides.data(),
                      static_cast<size_t>(nframes) * sizeof(hjd::RoiDev), hipMemcpyHostToDevice);
    if (e == hipSuccess && norm)
        e = hipMemcpy(reinterpret_cast<char*>(p->d_frames) + p->norm_off, &ident, sizeof(ident), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_qt, qnat.data(), qnat.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p->d_frames);
        (void)hipFree(p->d_qt);
        delete p;
        return fail(HJD_E_HIP, "plan upload: %s", hipGetErrorString(e));
    }
    *out = p;
    return HJD_OK;
}

int hjd_plan_destroy(hjd_plan* plan)
{
    if (!plan) return HJD_OK;
    (void)hipSetDevice(plan->ctx->device);
    (void)hipFree(plan->d_frames);
    (void)hipFree(plan->d_qt);
    delete plan;
    return HJD_OK;
}

// A launch of this plan, without the caller's buffers: its shape with the
// default grid, its device and its tables.
static hjd_internal::DecodeLaunch plan_launch(const hjd_plan* p)
{
    hjd_internal::DecodeLaunch l;
    l.sampling = p->sampling;
    l.input_format = p->input_format;
    l.out_format = p->out_format;
    l.scale = p->scale;
    l.roi = p->roi != 0;
    l.variant = p->variant;
    l.kernel_mode = p->kernel_mode;
    l.tasks = p->tasks;
    l.device = p->ctx->device;
    l.d_qt_nat = p->d_qt;
    l.d_frames = reinterpret_cast<const hjd_internal::FrameRecord*>(p->d_frames);
    l.nframes = p->nframes;
    return l;
}

int hjd_plan_set_variant(hjd_plan* plan, int variant)
{
    if (!plan) return fail(HJD_E_INVALID, "plan is NULL");
    hjd_internal::DecodeLaunch l = plan_launch(plan);
    l.variant = variant;
    // The bits must suit the plan's persistent kernel, whichever kernel its launches take; as
    // documented (hjd.h), a BGR24 plan takes them like a BGRX one and fails at a persistent launch.
    l.kernel_mode = HJD_KERNEL_PERSISTENT;
    if (l.out_format == HJD_OUT_BGR24) l.out_format = HJD_OUT_BGRX;
    int rc = hjd_internal::shape_check(l);
    if (rc) return rc;
    plan->variant = variant;
    return HJD_OK;
}

int hjd_plan_set_normalize(hjd_plan* plan, const float a[3], const float b[3])
{
    int rc = hjd_internal::norm_check(a, b);
    if (rc) return rc;
    if (!plan) return fail(HJD_E_INVALID, "plan is NULL");
    if (!hjd_internal::out_format_float_bytes(plan->out_format))
        return fail(HJD_E_INVALID, "hjd_plan_set_normalize: output format %d is not HJD_OUT_RGB_PLANAR_F16 / _F32",
                    plan->out_format);
    hjd_internal::NormRecord r = hjd_internal::norm_identity();
    for (int c = 0; c < 3; ++c) {
        r.a[c] = a[c];
        r.b[c] = b[c];
    }
    HJD_HIP(hipSetDevice(plan->ctx->device));
    // synchronous, like the plan's own upload: launches already enqueued keep what they read
    HJD_HIP(hipDeviceSynchronize());
    HJD_HIP(hipMemcpy(reinterpret_cast<char*>(plan->d_frames) + plan->norm_off, &r, sizeof(r), hipMemcpyHostToDevice));
    return HJD_OK;
}

int hjd_plan_set_chunk(hjd_plan* plan, int tasks)
{
    if (!plan || tasks < 0 || tasks > 4096) return fail(HJD_E_INVALID, "invalid chunk arguments");
    plan->tuned_per_wave = tasks;
    // exactly `tasks` per wave: no occupancy floor (unlike the shape default)
    plan->tuned_grid = tasks ? grid_for_chunk(std::max<int64_t>(plan->tasks, 1), tasks, false) : 0;   // 0: default
    return HJD_OK;
}

int hjd_plan_set_kernel(hjd_plan* plan, int mode)
{
    if (!plan) return fail(HJD_E_INVALID, "plan is NULL");
    hjd_internal::DecodeLaunch l = plan_launch(plan);
    l.kernel_mode = mode;
    l.variant = 0;   // the mode alone: a BGR24 plan's variant bits fail at its persistent launches (hjd.h)
    int rc = hjd_internal::shape_check(l);
    if (rc) return rc;
    plan->kernel_mode = mode;
    return HJD_OK;
}

int64_t hjd_plan_tasks(const hjd_plan* plan) { return plan ? plan->tasks : -1; }
int64_t hjd_plan_pixels(const hjd_plan* plan) { return plan ? plan->pixels : -1; }
int hjd_plan_scale(const hjd_plan* plan) { return plan ? plan->scale : -1; }
int hjd_plan_has_roi(const hjd_plan* plan) { return plan ? plan->roi : -1; }
int64_t hjd_plan_coef_bytes(const hjd_plan* plan) { return plan ? plan->coef_bytes : -1; }

// Grid of the fused kernel: short contiguous task chunks per wave and many
// more workgroups than fit at once (measured on MI355X, profiles/
// r01_tune_grid_*.json): the hardware dispatches groups in order, so the
// resident waves always work inside a narrow window of the batch and HBM sees
// far better locality than with 4096 persistent waves spread over the whole
// batch (4:2:0 +12 %, 4:4:4 +13 % over one persistent wave per slot).  With
// the XCD-contiguous group order (hjd_kernels.hpp group_order) the best chunk
// is 2 tasks per wave at 4:2:0 (+3.9 % over 1 on 1024-frame batches) and 16 at
// the VALU-heavier samplings 4:4:4, 4:2:2 and 4:4:0 (+1.3 % over 8 at 4:4:4;
// profiles/r02_tune_tasks_per_wave.json).  The lighter, memory-bound shapes
// want one task per wave: grayscale (0.69 -> 0.80 of 8 TB/s), 4:1:1 (0.65-0.71
// -> 0.76) and both int32 (idct.h) formats (4:2:0 0.67 -> 0.76-0.78, 4:4:4
// 0.74-0.75 -> 0.765-0.77), same box (profiles/r03_tune_tasks_per_wave_ext.json).
// HJD_TASKS_PER_WAVE overrides it (tuning).
static int64_t default_per_wave(int sampling, int fmt)
{
    const int64_t env = hjd_internal::tuning().tasks_per_wave.get();
    if (env > 0) return env;
    if (fmt != 0 || sampling == HJD_GRAY || sampling == HJD_YUV411_H4V1) return 1;
    return sampling == HJD_YUV420 ? 2 : 16;
}

// Tasks per wave a chunk request turns into: with the occupancy floor (the
// shape default and the autotune candidates) never fewer than ~4 waves per
// SIMD (256 CUs x 4 SIMDs), since a single 4:4:4 frame at 16 tasks per wave
// would leave most of the chip idle; hjd_plan_set_chunk pins it exactly.
static int64_t effective_per_wave(int64_t tasks, int64_t per_wave, bool occupancy_floor)
{
    if (occupancy_floor) per_wave = std::min<int64_t>(per_wave, tasks / (4 * 1024));
    return std::max<int64_t>(1, per_wave);
}

// Groups for `per_wave` tasks per wave.
static int grid_for_chunk(int64_t tasks, int64_t per_wave, bool occupancy_floor)
{
    per_wave = effective_per_wave(tasks, per_wave, occupancy_floor);
    const int64_t waves = (tasks + per_wave - 1) / per_wave;
    const int64_t groups = (waves + hjd::kWavesPerGroup - 1) / hjd::kWavesPerGroup;
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(groups, int64_t(1) << 24)));
}

// A default launch of this plan takes the persistent kernel (not the latency one).
static bool plan_is_persistent(const hjd_plan* p) { return !takes_latency(plan_launch(p)); }

static int default_grid(const hjd_ctx* ctx, int64_t work_waves)
{
    const int64_t cap = static_cast<int64_t>(ctx->num_cu) * 4;
    const int64_t need = (work_waves + hjd::kWavesPerGroup - 1) / hjd::kWavesPerGroup;
    return static_cast<int>(std::max<int64_t>(1, std::min(cap, need)));
}

int hjd_plan_launch(hjd_plan* plan, const void* d_coefs, void* d_out, void* stream, int grid_blocks)
{
    if (!plan) return fail(HJD_E_INVALID, "plan is NULL");
    if (plan->tasks == 0) return HJD_OK;
    if (!d_coefs || !d_out) return fail(HJD_E_INVALID, "NULL device buffer");
    if ((reinterpret_cast<uintptr_t>(d_coefs) | reinterpret_cast<uintptr_t>(d_out)) & 15)
        return fail(HJD_E_INVALID, "device buffers must be 16-byte aligned");
    if (grid_blocks < 0) return fail(HJD_E_INVALID, "grid_blocks < 0");
    // hjd_plan_autotune's / hjd_plan_set_chunk's chunk, for plans that take the
    // persistent kernel anyway (a small AUTO plan keeps the latency kernel)
    if (grid_blocks == 0 && plan->tuned_grid > 0 && plan_is_persistent(plan)) grid_blocks = plan->tuned_grid;
    hjd_internal::DecodeLaunch l = plan_launch(plan);
    l.d_coefs = d_coefs;
    l.d_out = d_out;
    l.stream = stream;
    l.grid_blocks = grid_blocks;
    return hjd_internal::launch_decode(l);
}

// The fused kernel's launch adapted to the device it runs on (VERDICT r3:
// the same 4:2:0 kernel ran ~10 % slower on some MI355X boxes, its memory
// side with it, while 4:4:4 did not; which per-wave chunk and store policy
// keep HBM busiest differs by box and shape: profiles/r04c_tpw_sweep.json).
// Times every candidate -- 1, 2, 4, 8 and 16 tasks per wave x nt / plain
// output stores (BGRX) -- on the plan's own buffers, `rounds` interleaved
// rounds of one warm + two timed launches each, keeps the fastest (minimum
// over rounds) for the plan's later default launches.  All candidates give
// identical pixels.  Synchronous; plans small enough for the latency kernel
// are left as they are.
//
// The choice is cached per process: device x sampling x input format x output
// format x the plan's other variant bits x task-count octave (floor(log2
// tasks)).  A later plan of the same key takes the cached shape with no
// launch (the search cost ~1 s per plan).  HJD_AUTOTUNE_CACHE=0
// disables the cache; hjd_autotune_cache_clear() empties it.
namespace {
// A cached choice applies to plans of the same kernel and batch geometry
// (frame count and task count), not just the same size octave.
struct TuneKey {
    int device, sampling, input_format, out_format, keep_variant, nframes;
    int64_t tasks;
    int scale, roi;
    bool operator<(const TuneKey& o) const
    {
        return std::tie(device, sampling, input_format, out_format, keep_variant, nframes, tasks, scale, roi) <
               std::tie(o.device, o.sampling, o.input_format, o.out_format, o.keep_variant, o.nframes, o.tasks, o.scale,
                        o.roi);
    }
};
std::mutex g_tune_mu;
std::map<TuneKey, std::pair<int, int>> g_tune;   // -> (tasks per wave, store bit)

bool tune_cache_enabled() { return hjd_internal::tuning().autotune_cache.get() != 0; }
}  // namespace

int hjd_autotune_cache_clear(void)
{
    std::lock_guard<std::mutex> lock(g_tune_mu);
    g_tune.clear();
    return HJD_OK;
}

int hjd_plan_autotune(hjd_plan* plan, const void* d_coefs, void* d_out, void* stream, int rounds,
                      int32_t* tasks_per_wave, int32_t* variant)
{
    if (!plan || rounds < 0 || rounds > 16) return fail(HJD_E_INVALID, "invalid autotune arguments");
    if (!d_coefs || !d_out || ((reinterpret_cast<uintptr_t>(d_coefs) | reinterpret_cast<uintptr_t>(d_out)) & 15))
        return fail(HJD_E_INVALID, "NULL or unaligned device buffer");
    if (rounds == 0) rounds = 2;
    auto report = [&]() {
        if (tasks_per_wave) *tasks_per_wave = plan->tuned_per_wave;
        if (variant) *variant = plan->variant;
        return HJD_OK;
    };
    plan->autotune_launches = 0;
    plan->autotune_cached = 0;
    if (plan->tasks == 0 || !plan_is_persistent(plan)) return report();
    const int keep = plan->variant & ~1;
    const TuneKey key{plan->ctx->device, plan->sampling, plan->input_format, plan->out_format, keep, plan->nframes,
                      plan->tasks, plan->scale, plan->roi};
    if (tune_cache_enabled()) {
        std::lock_guard<std::mutex> lock(g_tune_mu);
        auto it = g_tune.find(key);
        if (it != g_tune.end()) {
            plan->tuned_per_wave = it->second.first;
            plan->tuned_grid = grid_for_chunk(plan->tasks, it->second.first);
            plan->variant = keep | it->second.second;
            plan->autotune_cached = 1;
            return report();
        }
    }
    struct Cand {
        int64_t per_wave;   // tasks per wave
        int store;          // variant bit 0
        int grid;
        float best_ms;
    };
    std::vector<Cand> cands;
    for (int64_t pw : {1, 2, 4, 8, 16}) {
        const int g = grid_for_chunk(plan->tasks, pw);
        bool dup = false;
        for (const Cand& c : cands) dup |= c.grid == g;
        if (dup) continue;
        // the store policy is a BGRX variant bit; scaled plans have no variants (chunks only)
        for (int st = 0; st < (plan->out_format == HJD_OUT_BGRX && plan->scale == 1 && !plan->roi ? 2 : 1); ++st)
            cands.push_back({pw, st, g, 1e30f});
    }
    HJD_HIP(hipSetDevice(plan->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipEvent_t e0, e1;
    HJD_HIP(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail(HJD_E_HIP, "hipEventCreate");
    }
    int rc = HJD_OK;
    for (int r = 0; r < rounds && rc == HJD_OK; ++r) {
        for (Cand& c : cands) {
            hjd_internal::DecodeLaunch l = plan_launch(plan);
            l.variant = keep | c.store;
            l.kernel_mode = HJD_KERNEL_PERSISTENT;
            l.grid_blocks = c.grid;
            l.d_coefs = d_coefs;
            l.d_out = d_out;
            l.stream = s;
            auto go = [&]() {
                plan->autotune_launches++;
                return hjd_internal::launch_decode(l);
            };
            float ms = 0;
            if ((rc = go()) || (rc = hipEventRecord(e0, s) == hipSuccess ? HJD_OK : HJD_E_HIP) || (rc = go()) ||
                (rc = go()) || (rc = hipEventRecord(e1, s) == hipSuccess ? HJD_OK : HJD_E_HIP) ||
                (rc = hipEventSynchronize(e1) == hipSuccess ? HJD_OK : HJD_E_HIP) ||
                (rc = hipEventElapsedTime(&ms, e0, e1) == hipSuccess ? HJD_OK : HJD_E_HIP))
                break;
            c.best_ms = std::min(c.best_ms, ms / 2);
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc == HJD_E_HIP ? fail(HJD_E_HIP, "autotune timing failed") : rc;
    const Cand* best = &cands[0];
    for (const Cand& c : cands)
        if (c.best_ms < best->best_ms) best = &c;
    plan->tuned_grid = best->grid;
    plan->tuned_per_wave = static_cast<int>(best->per_wave);
    plan->variant = keep | best->store;
    if (tune_cache_enabled()) {
        std::lock_guard<std::mutex> lock(g_tune_mu);
        g_tune[key] = {static_cast<int>(best->per_wave), best->store};
    }
    return report();
}

int hjd_plan_launch_shape(const hjd_plan* plan, hjd_launch_shape* out)
{
    if (!plan || !out) return fail(HJD_E_INVALID, "invalid arguments");
    hjd_launch_shape r;
    memset(&r, 0, sizeof(r));
    r.variant = plan->variant;
    r.autotune_launches = plan->autotune_launches;
    r.autotune_cached = plan->autotune_cached;
    if (plan->tasks > 0 && !plan_is_persistent(plan)) {
        r.kernel = HJD_KERNEL_LATENCY;
        r.grid = static_cast<int32_t>(std::min<int64_t>(plan->tasks, INT32_MAX));
        r.tasks_per_wave = 1;
        r.max_tasks_per_wave = 1;
    } else {
        r.kernel = HJD_KERNEL_PERSISTENT;
        const int fmt = plan->input_format == HJD_IN_Q16_ZIGZAG ? 0 : 1;
        const int64_t t = std::max<int64_t>(plan->tasks, 1);
        const bool pinned = plan->tuned_grid > 0;
        r.tasks_per_wave = static_cast<int32_t>(
            pinned ? effective_per_wave(t, plan->tuned_per_wave, false)
                   : effective_per_wave(t, default_per_wave(plan->sampling, fmt), true));
        r.grid = pinned ? plan->tuned_grid : grid_for_chunk(t, default_per_wave(plan->sampling, fmt));
        if ((plan->variant & hjd::kVarWgInterleave) != 0) {   // groups take quads of tasks
            const int64_t quads = (t + hjd::kWavesPerGroup - 1) / hjd::kWavesPerGroup;
            r.max_tasks_per_wave = static_cast<int32_t>((quads + r.grid - 1) / r.grid);
        } else {
            const int64_t waves = static_cast<int64_t>(r.grid) * hjd::kWavesPerGroup;
            r.max_tasks_per_wave = static_cast<int32_t>((t + waves - 1) / waves);
        }
    }
    *out = r;
    return HJD_OK;
}

int hjd_debug_plan_launch_stages(hjd_plan* plan, int stages, const void* d_coefs, void* d_out, void* stream,
                                 int grid_blocks)
{
    if (!plan) return fail(HJD_E_INVALID, "plan is NULL");
    hjd_internal::DecodeLaunch l = plan_launch(plan);
    l.variant = 0;
    l.stages = stages;
    l.kernel_mode = HJD_KERNEL_PERSISTENT;
    int rc = hjd_internal::shape_check(l);
    if (rc) return rc;
    if (plan->tasks == 0) return HJD_OK;
    if (!d_coefs || !d_out || ((reinterpret_cast<uintptr_t>(d_coefs) | reinterpret_cast<uintptr_t>(d_out)) & 15))
        return fail(HJD_E_INVALID, "NULL or unaligned device buffer");
    l.d_coefs = d_coefs;
    l.d_out = d_out;
    l.stream = stream;
    l.grid_blocks = grid_blocks > 0 ? grid_blocks : plan->tuned_grid;
    return hjd_internal::launch_decode(l);
}

// The table entry a shape takes, without a device: d16 stands for the probe's
// answer.  key: {latency, S, F, V}, the template arguments of the entry found.
int hjd_debug_kernel_key(int sampling, int input_format, int out_format, int scale, int roi, int variant, int stages,
                         int kernel_mode, int64_t tasks, int grid_blocks, int d16, int32_t key[4])
{
    if (!key) return fail(HJD_E_INVALID, "key is NULL");
    DecodeShape s = make_shape(sampling, scale, input_format, out_format, roi != 0);
    s.variant = variant;
    s.stages = stages;
    s.kernel_mode = kernel_mode;
    s.tasks = tasks;
    s.grid_blocks = grid_blocks;
    const KernelEntry* k;
    int rc = select_kernel(s, d16 != 0, -1, &k);
    if (rc) return rc;
    std::copy(k->key, k->key + 4, key);
    return HJD_OK;
}

// The keys of the table, four ints each (at most `cap` entries are written); returns their count.
int hjd_debug_kernel_table(int32_t* keys, int cap)
{
    for (int i = 0; keys && i < std::min(cap, kKernels); ++i) std::copy(kKernelList[i].key, kKernelList[i].key + 4, keys + 4 * i);
    return kKernels;
}

int hjd_idct_blocks(hjd_ctx* ctx, const int32_t* d_in, int32_t* d_out, int64_t nblocks, void* stream)
{
    if (!ctx || nblocks < 0 || ((!d_in || !d_out) && nblocks > 0)) return fail(HJD_E_INVALID, "invalid arguments");
    if (nblocks == 0) return HJD_OK;
    HJD_HIP(hipSetDevice(ctx->device));
    const int grid = default_grid(ctx, (nblocks + 7) / 8);
    hipLaunchKernelGGL(hjd::idct_blocks_kernel, dim3(grid), dim3(hjd::kGroupThreads), 0,
                       static_cast<hipStream_t>(stream), d_in, d_out, nblocks);
    HJD_HIP(hipGetLastError());
    return HJD_OK;
}

int hjd_debug_csc(hjd_ctx* ctx, const int32_t* d_y, const int32_t* d_u, const int32_t* d_v, uint32_t* d_out,
                  int64_t n, int mode, void* stream)
{
    if (!ctx || n < 0 || (mode != 0 && mode != 1)) return fail(HJD_E_INVALID, "invalid arguments");
    if (n == 0) return HJD_OK;
    HJD_HIP(hipSetDevice(ctx->device));
    const int grid = static_cast<int>(std::min<int64_t>((n + 255) / 256, 65536));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == 0)
        hipLaunchKernelGGL(hjd::csc_kernel<0>, dim3(grid), dim3(256), 0, s, d_y, d_u, d_v, d_out, n);
    else
        hipLaunchKernelGGL(hjd::csc_kernel<1>, dim3(grid), dim3(256), 0, s, d_y, d_u, d_v, d_out, n);
    HJD_HIP(hipGetLastError());
    return HJD_OK;
}

int hjd_debug_csc_exhaustive(hjd_ctx* ctx, uint32_t* d_out, int mode, void* stream)
{
    if (!ctx || !d_out || (mode != 0 && mode != 1)) return fail(HJD_E_INVALID, "invalid arguments");
    HJD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == 0)
        hipLaunchKernelGGL(hjd::csc_exhaustive_kernel<0>, dim3(8192), dim3(256), 0, s, d_out);
    else
        hipLaunchKernelGGL(hjd::csc_exhaustive_kernel<1>, dim3(8192), dim3(256), 0, s, d_out);
    HJD_HIP(hipGetLastError());
    return HJD_OK;
}

}  // extern "C"
