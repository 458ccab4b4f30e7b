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

// JPEG zigzag: natural index of zigzag position k (src/zigzag.h:15-40).
constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                             12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                             58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

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

// launch_decode variant bits 8 and up: a stage-skipping measurement variant
// (hjd_debug_plan_launch_stages), stages << kStageShift | plan variant bits.
constexpr int kStageShift = 8;

int hjd_internal::ctx_num_cu(const hjd_ctx* ctx) { return ctx->num_cu; }

// The ROI's task set: MCU rows myf..myl times the strips
// that cover MCU columns mxf..mxl, anchored at mxf.
int hjd_internal::roi_geom(int width, int height, int sampling, int scale, const hjd_rect* roi, RoiGeom* g)
{
    int mw, mh, bpm, tasks_mcus;
    int rc = geometry(width, height, sampling, mw, mh, bpm, tasks_mcus);
    if (rc) return rc;
    const int lg = scale_log2(scale);
    if (lg < 0) return set_error(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", scale);
    if (scale > 1 && !scaled_sampling_ok(sampling))
        return set_error(HJD_E_INVALID, "scaled decode (scale %d) serves 4:4:4, 4:2:0 and gray, not sampling %d", scale,
                         sampling);
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
    if (scale_log2(scale) < 0) return set_error(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", scale);
    if (scale > 1 && !scaled_sampling_ok(sampling))
        return set_error(HJD_E_INVALID, "scaled decode (scale %d) serves 4:4:4, 4:2:0 and gray, not sampling %d", scale,
                         sampling);
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

int hjd_internal::launch_decode(int device, int num_cu, int sampling, int input_format, int variant,
                                const void* d_coefs, const int32_t* d_qt_nat, const FrameRecord* d_frames,
                                int nframes, int64_t tasks, void* d_out, void* stream, int grid_blocks, int out_format,
                                int kernel_mode, int scale, bool roi)
{
    HJD_HIP(hipSetDevice(device));
    const int fmt = input_format == HJD_IN_Q16_ZIGZAG ? 0 : 1;
    (void)num_cu;
    SamplingGeom sg;
    if (!sampling_geom(sampling, &sg)) return set_error(HJD_E_INVALID, "unsupported sampling %d", sampling);
    const int grid = grid_blocks > 0 ? grid_blocks : grid_for_chunk(tasks, default_per_wave(sampling, fmt));
    if (!out_format_bytes(out_format))
        return set_error(HJD_E_INVALID, "unknown output format %d", out_format);
    using K = void (*)(const void*, const int*, const FrameDev*, int, int64_t, uint8_t*);   // latency kernels
    using KP = void (*)(const void*, const int*, const FrameDev*, int, int64_t, uint8_t*, int64_t, int64_t);
    const bool latency = kernel_mode == HJD_KERNEL_LATENCY ||
                         (kernel_mode == HJD_KERNEL_AUTO && grid_blocks == 0 && tasks <= latency_max_tasks());
    // the task split of the persistent kernels (see decode_kernel): default
    // order over grid * 4 waves, wg-interleave over grid groups of 4-task quads
    const int64_t split_n = (variant & 2) ? static_cast<int64_t>(grid) : static_cast<int64_t>(grid) * hjd::kWavesPerGroup;
    const int64_t split_t = (variant & 2) ? (tasks + hjd::kWavesPerGroup - 1) / hjd::kWavesPerGroup : tasks;
    const int64_t chunk = split_t / split_n, rem = split_t % split_n;
    if (out_format_float_bytes(out_format)) {   // normalised float planes: int16 input, no variants
        const int lg = scale_log2(scale);
        const int fi = out_format == HJD_OUT_RGB_PLANAR_F16 ? 0 : 1;
        if (lg < 0) return set_error(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", scale);
        if (fmt != 0) return set_error(HJD_E_INVALID, "the float output formats take HJD_IN_Q16_ZIGZAG input only");
        if (variant != 0) return set_error(HJD_E_INVALID, "kernel variants are BGRX-only");
        if (lg > 0 && !scaled_sampling_ok(sampling))
            return set_error(HJD_E_INVALID, "scaled decode serves 4:4:4, 4:2:0 and gray, not sampling %d", sampling);
        if ((roi || lg > 0) && kernel_mode == HJD_KERNEL_LATENCY)
            return set_error(HJD_E_INVALID, "scaled and ROI decode have no latency kernel");
#define HJD_KN(S, X) hjd::decode_kernel<S, 0, hjd::kOutPlanar | hjd::kOutF16 | (X)>, \
                     hjd::decode_kernel<S, 0, hjd::kOutPlanar | hjd::kOutF32 | (X)>
#define HJD_KN6(X) HJD_KN(0, X), HJD_KN(1, X), HJD_KN(2, X), HJD_KN(3, X), HJD_KN(4, X), HJD_KN(5, X)
#define HJD_KN3(L, X) HJD_KN(0, ((L) << hjd::kScaleShift) | (X)), HJD_KN(1, ((L) << hjd::kScaleShift) | (X)), \
                      HJD_KN(3, ((L) << hjd::kScaleShift) | (X))
        // scale 1: [sampling index][F16, F32]; scaled: [log2 scale - 1][4:4:4, 4:2:0, gray][F16, F32]
        static const KP kNorm1[12] = {HJD_KN6(0)};
        static const KP kNormD16[2] = {HJD_KN(0, hjd::kVarD16)};
        static const KP kNormScaled[18] = {HJD_KN3(1, 0), HJD_KN3(2, 0), HJD_KN3(3, 0)};
        static const KP kNormRoi1[12] = {HJD_KN6(hjd::kVarRoi)};
        static const KP kNormRoiScaled[18] = {HJD_KN3(1, hjd::kVarRoi), HJD_KN3(2, hjd::kVarRoi),
                                              HJD_KN3(3, hjd::kVarRoi)};
#undef HJD_KN3
#undef HJD_KN6
#undef HJD_KN
        if (!roi && lg == 0 && latency) {
#define HJD_KNL(S) hjd::decode_kernel_lat<S, 0, hjd::kOutPlanar | hjd::kOutF16>, \
                   hjd::decode_kernel_lat<S, 0, hjd::kOutPlanar | hjd::kOutF32>
            static const K kNormLat[12] = {HJD_KNL(0), HJD_KNL(1), HJD_KNL(2), HJD_KNL(3), HJD_KNL(4), HJD_KNL(5)};
#undef HJD_KNL
            if (tasks > (int64_t(1) << 31) - 1) return set_error(HJD_E_INVALID, "too many tasks for the latency kernel");
            hipLaunchKernelGGL(kNormLat[2 * sg.index + fi], dim3(static_cast<uint32_t>(tasks)), dim3(hjd::kLatThreads), 0,
                               static_cast<hipStream_t>(stream), d_coefs, d_qt_nat,
                               reinterpret_cast<const FrameDev*>(d_frames), nframes, tasks, static_cast<uint8_t*>(d_out));
            HJD_HIP(hipGetLastError());
            return HJD_OK;
        }
        const int srow = sampling == HJD_YUV444 ? 0 : sampling == HJD_YUV420 ? 1 : 2;
        KP k = lg > 0 ? (roi ? kNormRoiScaled : kNormScaled)[6 * (lg - 1) + 2 * srow + fi]
                      : (roi ? kNormRoi1 : kNorm1)[2 * sg.index + fi];
        if (!roi && lg == 0 && sampling == HJD_YUV444 && hjd_internal::d16_gather_selected(device)) k = kNormD16[fi];
        hipLaunchKernelGGL(k, dim3(grid), dim3(hjd::kGroupThreads), 0, static_cast<hipStream_t>(stream), d_coefs,
                           d_qt_nat, reinterpret_cast<const FrameDev*>(d_frames), nframes, tasks,
                           static_cast<uint8_t*>(d_out), chunk, rem);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    }
    if (roi) {   // ROI decode: the persistent kernel only
        const int lg = scale_log2(scale);
        if (lg < 0) return set_error(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", scale);
        if (lg > 0 && !scaled_sampling_ok(sampling))
            return set_error(HJD_E_INVALID, "scaled decode serves 4:4:4, 4:2:0 and gray, not sampling %d", sampling);
        if (fmt != 0) return set_error(HJD_E_INVALID, "ROI decode takes HJD_IN_Q16_ZIGZAG input only");
        if (variant != 0) return set_error(HJD_E_INVALID, "ROI decode has no kernel variants");
        if (kernel_mode == HJD_KERNEL_LATENCY) return set_error(HJD_E_INVALID, "ROI decode has no latency kernel");
#define HJD_KR1(S, V, L) hjd::decode_kernel<S, 0, (V) | ((L) << hjd::kScaleShift) | hjd::kVarRoi>
#define HJD_KR4(S, L) HJD_KR1(S, 0, L), HJD_KR1(S, hjd::kOutBgr24, L), HJD_KR1(S, hjd::kOutRgb24, L), \
                      HJD_KR1(S, hjd::kOutPlanar, L)
#define HJD_KR(L) HJD_KR4(0, L), HJD_KR4(1, L), HJD_KR4(3, L)
        // scale 1: [sampling index][output format]; scaled: [log2 scale - 1][4:4:4, 4:2:0, gray][output format]
        static const KP kRoi1[24] = {HJD_KR4(0, 0), HJD_KR4(1, 0), HJD_KR4(2, 0), HJD_KR4(3, 0), HJD_KR4(4, 0),
                                     HJD_KR4(5, 0)};
        static const KP kRoiScaled[36] = {HJD_KR(1), HJD_KR(2), HJD_KR(3)};
#undef HJD_KR
#undef HJD_KR4
#undef HJD_KR1
        const int srow = sampling == HJD_YUV444 ? 0 : sampling == HJD_YUV420 ? 1 : 2;
        const KP k = lg == 0 ? kRoi1[4 * sg.index + out_format] : kRoiScaled[12 * (lg - 1) + 4 * srow + out_format];
        hipLaunchKernelGGL(k, dim3(grid), dim3(hjd::kGroupThreads), 0, static_cast<hipStream_t>(stream), d_coefs,
                           d_qt_nat, reinterpret_cast<const FrameDev*>(d_frames), nframes, tasks,
                           static_cast<uint8_t*>(d_out), chunk, rem);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    }
    if (scale != 1) {   // scaled decode: the persistent kernel only, [log2 scale - 1][sampling][output format]
        const int lg = scale_log2(scale);
        if (lg < 0) return set_error(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", scale);
        if (!scaled_sampling_ok(sampling))
            return set_error(HJD_E_INVALID, "scaled decode serves 4:4:4, 4:2:0 and gray, not sampling %d", sampling);
        if (fmt != 0) return set_error(HJD_E_INVALID, "scaled decode takes HJD_IN_Q16_ZIGZAG input only");
        if (variant != 0) return set_error(HJD_E_INVALID, "scaled decode has no kernel variants");
        if (kernel_mode == HJD_KERNEL_LATENCY)
            return set_error(HJD_E_INVALID, "scaled decode has no latency kernel");
#define HJD_KS1(S, V, L) hjd::decode_kernel<S, 0, (V) | ((L) << hjd::kScaleShift)>
#define HJD_KS4(S, L) HJD_KS1(S, 0, L), HJD_KS1(S, hjd::kOutBgr24, L), HJD_KS1(S, hjd::kOutRgb24, L), \
                      HJD_KS1(S, hjd::kOutPlanar, L)
#define HJD_KS(L) HJD_KS4(0, L), HJD_KS4(1, L), HJD_KS4(3, L)
        static const KP kScaled[36] = {HJD_KS(1), HJD_KS(2), HJD_KS(3)};
#undef HJD_KS
#undef HJD_KS4
#undef HJD_KS1
        const int srow = sampling == HJD_YUV444 ? 0 : sampling == HJD_YUV420 ? 1 : 2;
        hipLaunchKernelGGL(kScaled[12 * (lg - 1) + 4 * srow + out_format], dim3(grid), dim3(hjd::kGroupThreads), 0,
                           static_cast<hipStream_t>(stream), d_coefs, d_qt_nat,
                           reinterpret_cast<const FrameDev*>(d_frames), nframes, tasks, static_cast<uint8_t*>(d_out),
                           chunk, rem);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    }
    if (latency && (variant >> kStageShift) == 0) {   // [output format][sampling index][input format]
#define HJD_KL(V) hjd::decode_kernel_lat<0, 0, V>, hjd::decode_kernel_lat<0, 1, V>, \
                  hjd::decode_kernel_lat<1, 0, V>, hjd::decode_kernel_lat<1, 1, V>, \
                  hjd::decode_kernel_lat<2, 0, V>, hjd::decode_kernel_lat<2, 1, V>, \
                  hjd::decode_kernel_lat<3, 0, V>, hjd::decode_kernel_lat<3, 1, V>, \
                  hjd::decode_kernel_lat<4, 0, V>, hjd::decode_kernel_lat<4, 1, V>, \
                  hjd::decode_kernel_lat<5, 0, V>, hjd::decode_kernel_lat<5, 1, V>
        static const K kLat[48] = {HJD_KL(0), HJD_KL(hjd::kOutBgr24), HJD_KL(hjd::kOutRgb24),
                                   HJD_KL(hjd::kOutPlanar)};
#undef HJD_KL
        if (tasks > (int64_t(1) << 31) - 1) return set_error(HJD_E_INVALID, "too many tasks for the latency kernel");
        const K k = kLat[12 * out_format + ((sg.index << 1) | fmt)];
        hipLaunchKernelGGL(k, dim3(static_cast<uint32_t>(tasks)), dim3(hjd::kLatThreads), 0,
                           static_cast<hipStream_t>(stream), d_coefs, d_qt_nat,
                           reinterpret_cast<const FrameDev*>(d_frames), nframes, tasks, static_cast<uint8_t*>(d_out));
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    }
    if (out_format != HJD_OUT_BGRX) {   // [output format - 1][sampling index][input format], default variant
#define HJD_KF(V) hjd::decode_kernel<0, 0, V>, hjd::decode_kernel<0, 1, V>, hjd::decode_kernel<1, 0, V>, \
                  hjd::decode_kernel<1, 1, V>, hjd::decode_kernel<2, 0, V>, hjd::decode_kernel<2, 1, V>, \
                  hjd::decode_kernel<3, 0, V>, hjd::decode_kernel<3, 1, V>, hjd::decode_kernel<4, 0, V>, \
                  hjd::decode_kernel<4, 1, V>, hjd::decode_kernel<5, 0, V>, hjd::decode_kernel<5, 1, V>
        static const KP kTable24[36] = {HJD_KF(hjd::kOutBgr24), HJD_KF(hjd::kOutRgb24), HJD_KF(hjd::kOutPlanar)};
#undef HJD_KF
        static const KP kD16[3] = {hjd::decode_kernel<0, 0, hjd::kOutBgr24 | hjd::kVarD16>,
                                   hjd::decode_kernel<0, 0, hjd::kOutRgb24 | hjd::kVarD16>,
                                   hjd::decode_kernel<0, 0, hjd::kOutPlanar | hjd::kVarD16>};
        if ((variant & 3) != 0) return set_error(HJD_E_INVALID, "kernel variants are BGRX-only");
        KP k24 = kTable24[12 * (out_format - 1) + ((sg.index << 1) | fmt)];
        if (sampling == HJD_YUV444 && fmt == 0 && hjd_internal::d16_gather_selected(device)) k24 = kD16[out_format - 1];
        hipLaunchKernelGGL(k24, dim3(grid), dim3(hjd::kGroupThreads), 0,
                           static_cast<hipStream_t>(stream), d_coefs, d_qt_nat,
                           reinterpret_cast<const FrameDev*>(d_frames), nframes, tasks, static_cast<uint8_t*>(d_out),
                           chunk, rem);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    }
    if (fmt == 0 && (variant >> kStageShift) != 0) {   // stage-skipping measurement variants
        if (sg.index > 1) return hjd_internal::set_error(HJD_E_INVALID, "ablation variants are 4:4:4/4:2:0 only");
        constexpr int kStages[8] = {4, 8, 16, 20, 24, 64, 80, 256};
        const int stages = variant >> kStageShift;
        int si = -1;
        for (int i = 0; i < 8; ++i)
            if (kStages[i] == stages) si = i;
        if (si < 0) return hjd_internal::set_error(HJD_E_INVALID, "unknown ablation variant %d", stages);
#define HJD_ST(S, B) {hjd::decode_kernel<S, 0, 4 | (B)>, hjd::decode_kernel<S, 0, 8 | (B)>,                  \
                      hjd::decode_kernel<S, 0, 16 | (B)>, hjd::decode_kernel<S, 0, 20 | (B)>,                \
                      hjd::decode_kernel<S, 0, 24 | (B)>, hjd::decode_kernel<S, 0, 64 | (B)>,                \
                      hjd::decode_kernel<S, 0, 80 | (B)>, hjd::decode_kernel<S, 0, 256 | (B)>}
        // [4:2:0, 4:4:4, 4:4:4 d16 gather][stages]
        static const KP kStageK[3][8] = {HJD_ST(1, 0), HJD_ST(0, 0), HJD_ST(0, hjd::kVarD16)};
#undef HJD_ST
        const int col = sampling == HJD_YUV420 ? 0 : hjd_internal::d16_gather_selected(device) ? 2 : 1;   // as the product gathers
        const KP k = kStageK[col][si];
        hipLaunchKernelGGL(k, dim3(grid), dim3(hjd::kGroupThreads), 0, static_cast<hipStream_t>(stream), d_coefs,
                           d_qt_nat, reinterpret_cast<const FrameDev*>(d_frames), nframes, tasks,
                           static_cast<uint8_t*>(d_out), chunk, rem);
        HJD_HIP(hipGetLastError());
        return HJD_OK;
    }
    // [sampling index][input format][variant bits 0-1]
    const int key = (sg.index << 3) | (fmt << 2) | (variant & 3);
#define HJD_K4(S, F) hjd::decode_kernel<S, F, 0>, hjd::decode_kernel<S, F, 1>, hjd::decode_kernel<S, F, 2>, \
                     hjd::decode_kernel<S, F, 3>
    static const KP kTable[48] = {HJD_K4(0, 0), HJD_K4(0, 1), HJD_K4(1, 0), HJD_K4(1, 1),
                                 HJD_K4(2, 0), HJD_K4(2, 1), HJD_K4(3, 0), HJD_K4(3, 1),
                                 HJD_K4(4, 0), HJD_K4(4, 1), HJD_K4(5, 0), HJD_K4(5, 1)};
#undef HJD_K4
    KP k = kTable[key];
    if (sampling == HJD_YUV444 && fmt == 0 && (variant & 2) == 0 && hjd_internal::d16_gather_selected(device))
        k = (variant & 1) ? hjd::decode_kernel<0, 0, hjd::kVarPlainStores | hjd::kVarD16>
                          : hjd::decode_kernel<0, 0, hjd::kVarD16>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(hjd::kGroupThreads), 0, static_cast<hipStream_t>(stream),
                       d_coefs, d_qt_nat, reinterpret_cast<const FrameDev*>(d_frames), nframes, tasks,
                       static_cast<uint8_t*>(d_out), chunk, rem);
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
    if (hjd_internal::scale_log2(scale) < 0) return fail(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", scale);
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

// One frame's geometry and output layout, as a plan of `scale` (and ROIs)
// takes it: sw x sh is what the frame writes (the ROI's size, else the scaled
// frame's), rg the ROI's geometry.  i: the frame's index, for the message.
static int check_frame(const hjd_frame& f, int input_format, int scale, const hjd_rect* roi, int i,
                       hjd_internal::RoiGeom* rg, int* sw, int* sh)
{
    int mw, mh, bpm, tasks_mcus;
    int rc = geometry(f.width, f.height, f.sampling, mw, mh, bpm, tasks_mcus);
    if (rc) return fail(rc, "frame %d: %s", i, std::string(g_last_error).c_str());
    const int rbytes = hjd_internal::out_format_row_bytes(f.out_format);
    if (!rbytes) return fail(HJD_E_INVALID, "unknown output format %d", f.out_format);
    if (hjd_internal::out_format_float_bytes(f.out_format) && input_format != HJD_IN_Q16_ZIGZAG)
        return fail(HJD_E_INVALID, "the float output formats take HJD_IN_Q16_ZIGZAG input, not HJD_IN_I32_NATURAL");
    if (scale > 1 && !hjd_internal::scaled_sampling_ok(f.sampling))
        return fail(HJD_E_INVALID,
                    "frame %d: scaled decode (scale %d) serves 4:4:4, 4:2:0 and gray, not 4:2:2, 4:1:1 or 4:4:0 "
                    "(sampling %d)", i, scale, f.sampling);
    *sw = hjd_internal::scaled_dim(f.width, scale);
    *sh = hjd_internal::scaled_dim(f.height, scale);
    if (roi) {   // the output is the ROI: pitch and payload refer to it
        rc = hjd_internal::roi_geom(f.width, f.height, f.sampling, scale, roi, rg);
        if (rc) return fail(rc, "frame %d: %s", i, std::string(g_last_error).c_str());
        *sw = roi->w;
        *sh = roi->h;
    }
    // BGRX / BGR24: 4-byte pitches and offsets; the RGB formats take any; the
    // float planes multiples of their element size
    const uint64_t amask = static_cast<uint64_t>(hjd_internal::out_format_pitch_mask(f.out_format));
    if (f.out_pitch < static_cast<int64_t>(rbytes) * *sw || (f.out_pitch & amask) || (f.out_offset & amask))
        return fail(HJD_E_INVALID, "frame %d: bad output pitch/offset", i);
    return HJD_OK;
}

int hjd_frame_check(const hjd_frame* frame, int input_format, int scale, const hjd_rect* roi)
{
    if (!frame) return fail(HJD_E_INVALID, "frame is NULL");
    if (hjd_internal::scale_log2(scale) < 0) return fail(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", scale);
    if (input_format != HJD_IN_Q16_ZIGZAG && input_format != HJD_IN_I32_NATURAL)
        return fail(HJD_E_INVALID, "unknown input format %d", input_format);
    if ((scale > 1 || roi) && input_format == HJD_IN_I32_NATURAL)
        return fail(HJD_E_INVALID, "scaled and ROI decode take HJD_IN_Q16_ZIGZAG input, not HJD_IN_I32_NATURAL");
    hjd_internal::RoiGeom rg;
    int sw, sh;
    return check_frame(*frame, input_format, scale, roi, 0, &rg, &sw, &sh);
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
    if (hjd_internal::scale_log2(scale) < 0) return fail(HJD_E_INVALID, "scale %d is not 1, 2, 4 or 8", scale);
    if (scale > 1 && input_format == HJD_IN_I32_NATURAL)
        return fail(HJD_E_INVALID, "scaled decode (scale %d) takes HJD_IN_Q16_ZIGZAG input, not HJD_IN_I32_NATURAL", scale);
    if (input_format != HJD_IN_Q16_ZIGZAG && input_format != HJD_IN_I32_NATURAL)
        return fail(HJD_E_INVALID, "unknown input format %d", input_format);
    if (rois && input_format == HJD_IN_I32_NATURAL)
        return fail(HJD_E_INVALID, "ROI decode takes HJD_IN_Q16_ZIGZAG input, not HJD_IN_I32_NATURAL");
    if (input_format == HJD_IN_Q16_ZIGZAG && (!qtables || nq <= 0))
        return fail(HJD_E_INVALID, "quantisation tables required for HJD_IN_Q16_ZIGZAG");

    std::vector<FrameDev> fd(static_cast<size_t>(std::max(nframes, 1)));
    std::vector<hjd_internal::RoiRecord> sides(rois ? fd.size() : 0);
    int64_t tasks = 0, pixels = 0, blocks = 0;
    int sampling = nframes > 0 ? frames[0].sampling : HJD_YUV420;
    const int out_format = nframes > 0 ? frames[0].out_format : HJD_OUT_BGRX;
    const int obytes = hjd_internal::out_format_bytes(out_format);
    if (!obytes) return fail(HJD_E_INVALID, "unknown output format %d", out_format);
    if (hjd_internal::out_format_float_bytes(out_format) && input_format != HJD_IN_Q16_ZIGZAG)
        return fail(HJD_E_INVALID, "the float output formats take HJD_IN_Q16_ZIGZAG input, not HJD_IN_I32_NATURAL");
    for (int i = 0; i < nframes; ++i) {
        const hjd_frame& f = frames[i];
        int mw, mh, bpm, tasks_mcus;
        int rc = geometry(f.width, f.height, f.sampling, mw, mh, bpm, tasks_mcus);
        if (rc) return fail(rc, "frame %d: %s", i, g_last_error.c_str());
        if (f.sampling != sampling)
            return fail(HJD_E_INVALID, "frame %d: mixed sampling in one plan (use one plan per sampling)", i);
        if (f.out_format != out_format)
            return fail(HJD_E_INVALID, "frame %d: mixed output formats in one plan (use one plan per format)", i);
        int sw, sh;
        hjd_internal::RoiGeom rg;
        rc = check_frame(f, input_format, scale, rois ? &rois[i] : nullptr, i, &rg, &sw, &sh);
        if (rc) return rc;
        FrameDev& d = fd[i];
        if (input_format == HJD_IN_Q16_ZIGZAG) {
            for (int c = 0; c < 3; ++c)
                if (f.qt_index[c] < 0 || f.qt_index[c] >= nq)
                    return fail(HJD_E_INVALID, "frame %d: qt_index[%d]=%d out of range", i, c, f.qt_index[c]);
        }
        d.coef_base = static_cast<int64_t>(f.coef_offset);
        d.out_base = static_cast<int64_t>(f.out_offset);
        d.task_begin = tasks;
        d.width = sw;
        d.height = sh;
        d.pitch = f.out_pitch;
        d.sampling = f.sampling;
        d.mcu_w = mw;
        d.strips = (mw + tasks_mcus - 1) / tasks_mcus;
        for (int c = 0; c < 3; ++c) d.qt[c] = input_format == HJD_IN_Q16_ZIGZAG ? f.qt_index[c] : 0;
        d.vec_ok = hjd_internal::out_vector_ok(out_format, f.out_pitch, static_cast<int64_t>(f.out_offset)) ? 1 : 0;
        if (rois) {
            apply_roi(d, sides[i], rg, rois[i], out_format, 0);
            tasks += rg.tasks;
            blocks += rg.blocks;
        } else {
            tasks += static_cast<int64_t>(d.strips) * mh;
            blocks += static_cast<int64_t>(mw) * mh * bpm;
        }
        pixels += static_cast<int64_t>(sw) * sh;
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

    // a ROI plan's RoiDev table follows the nframes records (frames + nframes)
    static_assert(sizeof(hjd_internal::RoiRecord) == sizeof(hjd::RoiDev), "side record layout");
    const size_t side_off = static_cast<size_t>(nframes) * sizeof(FrameDev);
    // a float plan's NormDev record follows both tables; a = 1, b = 0 until hjd_plan_set_normalize
    static_assert(sizeof(hjd_internal::NormRecord) == sizeof(hjd::NormDev), "norm record layout");
    const bool norm = hjd_internal::out_format_float_bytes(out_format) != 0;
    p->norm_off = norm ? side_off + (rois ? static_cast<size_t>(nframes) * sizeof(hjd::RoiDev) : 0) : 0;
    const hjd_internal::NormRecord ident = hjd_internal::norm_identity();
    hipError_t e = hipMalloc(&p->d_frames, std::max(fd.size() * sizeof(FrameDev) + sides.size() * sizeof(hjd::RoiDev),
                                                    p->norm_off) + (norm ? sizeof(hjd::NormDev) : 0));
    if (e == hipSuccess) e = hipMalloc(&p->d_qt, qnat.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(p->d_frames, fd.data(), fd.size() * sizeof(FrameDev), hipMemcpyHostToDevice);
    if (e == hipSuccess && rois && nframes > 0)
        e = hipMemcpy(reinterpret_cast<char*>(p->d_frames) + side_off, sides.data(),
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

int hjd_plan_set_variant(hjd_plan* plan, int variant)
{
    if (!plan) return fail(HJD_E_INVALID, "plan is NULL");
    if (variant < 0 || variant > 3) return fail(HJD_E_INVALID, "unknown kernel variant %d", variant);
    if (variant != 0 && (hjd_internal::out_format_any_alignment(plan->out_format) ||
                         hjd_internal::out_format_float_bytes(plan->out_format)))
        return fail(HJD_E_INVALID, "kernel variants are BGRX-only");
    if (variant != 0 && plan->scale != 1)
        return fail(HJD_E_INVALID, "a scaled plan (scale %d) has no kernel variants", plan->scale);
    if (variant != 0 && plan->roi) return fail(HJD_E_INVALID, "a ROI plan has no kernel variants");
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
    if (mode != HJD_KERNEL_AUTO && mode != HJD_KERNEL_PERSISTENT && mode != HJD_KERNEL_LATENCY)
        return fail(HJD_E_INVALID, "unknown kernel mode %d", mode);
    if (mode == HJD_KERNEL_LATENCY && plan->scale != 1)
        return fail(HJD_E_INVALID, "a scaled plan (scale %d) has no latency kernel", plan->scale);
    if (mode == HJD_KERNEL_LATENCY && plan->roi) return fail(HJD_E_INVALID, "a ROI plan has no latency kernel");
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
static bool plan_is_persistent(const hjd_plan* p)
{
    return p->kernel_mode == HJD_KERNEL_PERSISTENT || p->scale != 1 || p->roi ||   // scaled / ROI: no latency kernel
           (p->kernel_mode == HJD_KERNEL_AUTO && p->tasks > latency_max_tasks());
}

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
    return hjd_internal::launch_decode(plan->ctx->device, plan->ctx->num_cu, plan->sampling, plan->input_format,
                                       plan->variant, d_coefs, plan->d_qt,
                                       reinterpret_cast<const hjd_internal::FrameRecord*>(plan->d_frames),
                                       plan->nframes, plan->tasks, d_out, stream, grid_blocks, plan->out_format,
                                       plan->scale != 1 || plan->roi ? HJD_KERNEL_PERSISTENT : plan->kernel_mode,
                                       plan->scale, plan->roi != 0);
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
            const int v = keep | c.store;
            auto go = [&]() {
                plan->autotune_launches++;
                return hjd_internal::launch_decode(plan->ctx->device, plan->ctx->num_cu, plan->sampling,
                                                   plan->input_format, v, d_coefs, plan->d_qt,
                                                   reinterpret_cast<const hjd_internal::FrameRecord*>(plan->d_frames),
                                                   plan->nframes, plan->tasks, d_out, s, c.grid, plan->out_format,
                                                   HJD_KERNEL_PERSISTENT, plan->scale, plan->roi != 0);
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
    if (stages != 4 && stages != 16 && stages != 20 && stages != 64 && stages != 80 && stages != 8 && stages != 24 &&
        stages != 256)
        return fail(HJD_E_INVALID, "unknown stage variant %d", stages);
    if (plan->scale != 1)
        return fail(HJD_E_INVALID, "stage variants are not built for scaled plans (scale %d)", plan->scale);
    if (plan->roi) return fail(HJD_E_INVALID, "stage variants are not built for ROI plans");
    if (plan->input_format != HJD_IN_Q16_ZIGZAG || plan->out_format != HJD_OUT_BGRX ||
        (plan->sampling != HJD_YUV420 && plan->sampling != HJD_YUV444))
        return fail(HJD_E_INVALID, "stage variants: 4:2:0 / 4:4:4, int16 zigzag in, BGRX out");
    if (plan->tasks == 0) return HJD_OK;
    if (!d_coefs || !d_out || ((reinterpret_cast<uintptr_t>(d_coefs) | reinterpret_cast<uintptr_t>(d_out)) & 15))
        return fail(HJD_E_INVALID, "NULL or unaligned device buffer");
    return hjd_internal::launch_decode(plan->ctx->device, plan->ctx->num_cu, plan->sampling, plan->input_format,
                                       stages << kStageShift, d_coefs, plan->d_qt,
                                       reinterpret_cast<const hjd_internal::FrameRecord*>(plan->d_frames),
                                       plan->nframes, plan->tasks, d_out, stream,
                                       grid_blocks > 0 ? grid_blocks : plan->tuned_grid,
                                       plan->out_format, HJD_KERNEL_PERSISTENT);
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
