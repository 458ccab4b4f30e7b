// hjd_gstream.hip -- the GPU-entropy stream (include/hjd_host.h hjd_gstream_*;
// DESIGN.md s10): submit JPEGs one by one; worker threads parse and destuff
// them into the pinned staging of the open batch (nslots batches rotate, each
// an hjd_gdec on its own HIP stream, so one batch's upload overlaps another's
// kernels); the thread that completes a closed batch issues it.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>

#include "hjd_gdec.hpp"
#include "hjd_host.h"

using hjd_internal::set_error;
using hjd_internal::tuning;
using namespace hjd::ent;

namespace {

struct GBatch {
    int slot = 0;
    int nframes = 0;
    size_t bytes = 0;
    int64_t blocks = 0;
    int prepared = 0;
    bool closed = false;
    bool issued = false;
    std::vector<void*> outs;         // device destination, or null for a host-output frame
    std::vector<int32_t> pitches;
    std::vector<void*> host_outs;    // host destination (D2H sink), or null
    RawCursor raw;                   // raw-area placement of device-destuffed scans
};

struct GJob {
    GBatch* batch;
    int index;
    const uint8_t* data;
    size_t size;
    size_t data_off;
    size_t cap;
    int mode;                        // kDestuff*
    uint64_t raw_off;
};

}  // namespace

struct hjd_gstream {
    hjd_ctx* ctx = nullptr;
    int device = 0;
    std::vector<hjd_gdec*> slots;
    std::vector<hipStream_t> streams;
    std::vector<uint8_t*> scratch;       // per slot: device pixels of host-output frames (D2H sink)
    std::vector<size_t> scratch_bytes;
    std::vector<GBatch*> slot_batch;   // batch currently owning each slot (nullptr = free)
    int next_slot = 0;
    GBatch* open = nullptr;

    std::mutex mu;
    std::mutex api_mu;          // serialises submit/sync callers (batch opening drops `mu` while it waits)
    std::condition_variable cv_jobs, cv_state;
    std::deque<GJob> queue;
    bool stop = false;
    std::vector<std::thread> workers;
    int64_t batches_in_flight = 0;     // created and not yet issued

    std::atomic<int64_t> images{0}, pixels{0}, prep_ns{0}, h2d_bytes{0}, batches{0}, host_scan_bytes{0};
    int first_error = HJD_OK;
    std::string first_error_msg;
    int local_cpus = 0;   // CPUs of the GPU's NUMA node the workers are bound to (0: unbound)
    int out_format = HJD_OUT_BGRX;

    void record_error(int rc, const std::string& msg)
    {
        if (first_error == HJD_OK) {
            first_error = rc;
            first_error_msg = msg;
        }
    }
    int open_batch(std::unique_lock<std::mutex>& lk);
    void issue_locked(GBatch* b);
    void worker();
};

// Caller holds mu.  Waits for the next slot's previous batch to be issued and
// its uploads to finish before reusing the slot's pinned staging.
int hjd_gstream::open_batch(std::unique_lock<std::mutex>& lk)
{
    const int s = next_slot;
    next_slot = (next_slot + 1) % static_cast<int>(slots.size());
    cv_state.wait(lk, [&] { return !slot_batch[s] || slot_batch[s]->issued; });
    if (slot_batch[s]) {
        delete slot_batch[s];
        slot_batch[s] = nullptr;
        hjd_gdec* g = slots[s];
        if (g->pending) {
            lk.unlock();
            const hipError_t e = hipEventSynchronize(g->staged_by_done ? g->done : g->staged);
            lk.lock();
            if (e != hipSuccess) return set_error(HJD_E_HIP, "hipEventSynchronize: %s", hipGetErrorString(e));
        }
        // statuses of the slot's previous batch
        if (g->pending) {
            lk.unlock();
            const int rc = hjd_gdec_sync(g, nullptr);
            const std::string msg = rc ? hjd_last_error() : "";
            lk.lock();
            if (rc) record_error(rc, msg);
        }
    }
    GBatch* b = new GBatch;
    b->slot = s;
    slot_batch[s] = b;
    open = b;
    ++batches_in_flight;
    return HJD_OK;
}

// Caller holds mu; b is closed and fully prepared.
void hjd_gstream::issue_locked(GBatch* b)
{
    if (b->issued) return;
    hjd_gdec* g = slots[b->slot];
    // drop frames whose preparation failed (already recorded)
    std::vector<void*> outs;
    std::vector<int32_t> pitches;
    std::vector<HostCopy> host;
    std::vector<Prepared> keep;
    size_t used = 0, scratch_need = 0;
    for (int i = 0; i < b->nframes; ++i) {
        Prepared& p = g->st.frames[i];
        if (p.rc != HJD_OK) continue;
        used = std::max(used, align_up(p.data_end(), 16));
        images++;
        pixels += static_cast<int64_t>(p.width) * p.height;
        if (b->host_outs[i]) {
            host.push_back(HostCopy{b->host_outs[i], b->pitches[i], p.width, p.height});
            outs.push_back(reinterpret_cast<void*>(scratch_need));   // offset, rebased below
            pitches.push_back(align_up(static_cast<size_t>(hjd_internal::out_format_row_bytes(out_format)) * p.width, 16));
            scratch_need += align_up(static_cast<size_t>(pitches.back()) *
                                         static_cast<size_t>(hjd_internal::out_format_rows(out_format, p.height)), 256);
        } else {
            host.push_back(HostCopy{nullptr, 0, p.width, p.height});
            outs.push_back(b->outs[i]);
            pitches.push_back(b->pitches[i]);
        }
        keep.push_back(std::move(p));
    }
    g->st.frames.swap(keep);
    g->st.data_used = used;
    int rc = HJD_OK;
    if (scratch_need > scratch_bytes[b->slot]) {   // grows rarely; the slot's previous batch is complete
        if (scratch[b->slot]) (void)hipFree(scratch[b->slot]);
        scratch[b->slot] = nullptr;
        scratch_bytes[b->slot] = 0;
        if (hipMalloc(reinterpret_cast<void**>(&scratch[b->slot]), scratch_need) != hipSuccess)
            rc = set_error(HJD_E_NOMEM, "device scratch for host outputs (%zu bytes)", scratch_need);
        else
            scratch_bytes[b->slot] = scratch_need;
    }
    for (size_t i = 0; i < outs.size(); ++i)
        if (host[i].host) outs[i] = scratch[b->slot] + reinterpret_cast<size_t>(outs[i]);
    if (rc) record_error(rc, hjd_last_error());
    if (!g->st.frames.empty() && rc == HJD_OK) {
        GdecCall c;
        c.d_outs = outs.data();
        c.pitches = pitches.data();
        c.stream = streams[b->slot];
        c.host = host.data();
        rc = gdec_issue(g, c);
        if (rc) record_error(rc, hjd_last_error());
        h2d_bytes += g->last_h2d;
        host_scan_bytes += g->last_host_scan_bytes;
        batches++;
    }
    b->issued = true;
    --batches_in_flight;
    cv_state.notify_all();
}

void hjd_gstream::worker()
{
    (void)hipSetDevice(device);
    for (;;) {
        GJob job;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_jobs.wait(lk, [&] { return stop || !queue.empty(); });
            if (queue.empty()) return;
            job = queue.front();
            queue.pop_front();
        }
        hjd_gdec* g = slots[job.batch->slot];
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = g->st.prepare_frame(job.index, job.data, job.size, job.data_off, job.cap, job.mode, job.raw_off);
        prep_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        const std::string msg = rc ? hjd_last_error() : "";
        std::unique_lock<std::mutex> lk(mu);
        if (rc) record_error(rc, msg);
        GBatch* b = job.batch;
        ++b->prepared;
        if (b->closed && b->prepared == b->nframes) issue_locked(b);
        cv_state.notify_all();
    }
}

extern "C" {

int hjd_gstream_create(hjd_ctx* ctx, int max_frames, int64_t max_scan_bytes, int64_t max_blocks, int nslots,
                       int nthreads, hjd_gstream** out)
{
    if (!ctx || !out || nslots < 2 || nslots > 16) return set_error(HJD_E_INVALID, "invalid gstream arguments (nslots 2..16)");
    *out = nullptr;
    if (nthreads <= 0) nthreads = hjd_internal::default_worker_threads(hjd_ctx_device(ctx));
    hjd_gstream* st = new (std::nothrow) hjd_gstream;
    if (!st) return set_error(HJD_E_NOMEM, "gstream allocation");
    st->ctx = ctx;
    st->device = hjd_ctx_device(ctx);
    st->slots.assign(nslots, nullptr);
    st->streams.assign(nslots, nullptr);
    st->scratch.assign(nslots, nullptr);
    st->scratch_bytes.assign(nslots, 0);
    st->slot_batch.assign(nslots, nullptr);
    // NUMA locality: pinned staging is allocated, and the
    // workers run, on the CPUs of the GPU's NUMA node (HJD_NUMA=0 disables).
    const hjd_internal::CpuSet local =
        tuning().numa.get() ? hjd_internal::device_local_cpus(st->device) : hjd_internal::CpuSet{};
    const std::vector<int> prev = hjd_internal::bind_current_thread(local);
    for (int s = 0; s < nslots; ++s) {
        int rc = hjd_gdec_create(ctx, max_frames, max_scan_bytes, max_blocks, stream_sub_bits(max_frames),
                                 &st->slots[s]);
        if (rc == HJD_OK && hipStreamCreateWithFlags(&st->streams[s], hipStreamNonBlocking) != hipSuccess)
            rc = set_error(HJD_E_HIP, "hipStreamCreate");
        if (rc) {
            hjd_internal::restore_current_thread(prev);
            hjd_gstream_destroy(st);
            return rc;
        }
    }
    hjd_internal::restore_current_thread(prev);
    st->local_cpus = static_cast<int>(local.cpus.size());
    for (int t = 0; t < nthreads; ++t)
        st->workers.emplace_back([st, local] {
            hjd_internal::bind_current_thread(local);
            st->worker();
        });
    *out = st;
    return HJD_OK;
}

static int gstream_submit(hjd_gstream* st, const uint8_t* data, size_t size, void* d_out, void* h_out,
                          int32_t out_pitch)
{
    hjd_internal::ScanHeader h;
    int rc = hjd_internal::parse_scan_header(data, size, &h);
    if (rc) return rc;
    if (out_pitch < hjd_internal::out_format_row_bytes(st->out_format) * h.width)
        return set_error(HJD_E_INVALID, "output pitch too small");
    const size_t need = h.extra_scans > 0 ? data_need(size) : align_up(size + kDataPad, 16);
    std::lock_guard<std::mutex> api(st->api_mu);
    std::unique_lock<std::mutex> lk(st->mu);
    hjd_gdec* g0 = st->slots[0];
    if (need > g0->st.data_cap() || h.nblocks > g0->st.caps.max_blocks)
        return set_error(HJD_E_INVALID, "JPEG larger than one batch's capacity");
    int mode = kDestuffHost;
    uint64_t raw_off = 0;
    bool fits = true;
    if (st->open) {
        GBatch* b = st->open;
        hjd_gdec* g = st->slots[b->slot];
        RawCursor cur = b->raw;
        rc = plan_raw(g->st, data, size, cur, mode, raw_off, fits, g->st.data_cap(), 0, false);
        if (rc) return rc;
        if (!fits || b->nframes == g->st.caps.max_frames || b->bytes + need > g->st.data_cap() ||
            b->blocks + h.nblocks > g->st.caps.max_blocks) {
            b->closed = true;
            st->open = nullptr;
            if (b->prepared == b->nframes) st->issue_locked(b);
        } else {
            b->raw = cur;
        }
    }
    if (!st->open) {
        rc = st->open_batch(lk);
        if (rc) return rc;
        GBatch* b = st->open;
        rc = plan_raw(st->slots[b->slot]->st, data, size, b->raw, mode, raw_off, fits, g0->st.data_cap(), 0, false);
        if (rc) return rc;
        if (!fits) return set_error(HJD_E_INVALID, "JPEG larger than one batch's capacity");
    }
    GBatch* b = st->open;
    hjd_gdec* g = st->slots[b->slot];
    if (b->nframes == 0) g->st.frames.assign(static_cast<size_t>(g->st.caps.max_frames), Prepared());
    GJob job{b, b->nframes, data, size, b->bytes, need, mode, raw_off};
    b->outs.push_back(d_out);
    b->host_outs.push_back(h_out);
    b->pitches.push_back(out_pitch);
    b->nframes++;
    b->bytes += need;
    b->blocks += h.nblocks;
    st->queue.push_back(job);
    lk.unlock();
    st->cv_jobs.notify_one();
    return HJD_OK;
}

int hjd_gstream_submit(hjd_gstream* st, const uint8_t* data, size_t size, void* d_out, int32_t out_pitch)
{
    const int fmt = st ? st->out_format : HJD_OUT_BGRX;
    const uintptr_t amask = hjd_internal::out_format_align_mask(fmt);
    const int pmask = hjd_internal::out_format_any_alignment(fmt) ? 0 : 3;
    if (!st || !data || !d_out || out_pitch <= 0 || (out_pitch & pmask) || (reinterpret_cast<uintptr_t>(d_out) & amask))
        return set_error(HJD_E_INVALID, "invalid submit arguments (d_out must be 16-byte (BGR24: 4-byte) aligned)");
    return gstream_submit(st, data, size, d_out, nullptr, out_pitch);
}

int hjd_gstream_submit_host(hjd_gstream* st, const uint8_t* data, size_t size, void* h_out, int32_t out_pitch)
{
    if (!st || !data || !h_out || out_pitch <= 0) return set_error(HJD_E_INVALID, "invalid submit arguments");
    return gstream_submit(st, data, size, nullptr, h_out, out_pitch);
}

int hjd_gstream_set_output_format(hjd_gstream* st, int out_format)
{
    if (!st) return set_error(HJD_E_INVALID, "gstream is NULL");
    if (!hjd_internal::out_format_bytes(out_format)) return set_error(HJD_E_INVALID, "unknown output format %d", out_format);
    if (hjd_internal::out_format_float_bytes(out_format))
        return set_error(HJD_E_INVALID, "hjd_gstream does not serve the float output formats (format %d): use hjd_gdec "
                                        "or a plan", out_format);
    std::lock_guard<std::mutex> api(st->api_mu);
    std::lock_guard<std::mutex> lk(st->mu);
    if (st->open || st->batches_in_flight)
        return set_error(HJD_E_STATE, "output format can only change between hjd_gstream_sync and the next submit");
    st->out_format = out_format;
    for (hjd_gdec* g : st->slots) g->out_format = out_format;
    return HJD_OK;
}

int hjd_gstream_sync(hjd_gstream* st, int64_t stats[5])
{
    if (!st) return set_error(HJD_E_INVALID, "gstream is NULL");
    std::lock_guard<std::mutex> api(st->api_mu);
    {
        std::unique_lock<std::mutex> lk(st->mu);
        if (st->open) {
            GBatch* b = st->open;
            b->closed = true;
            st->open = nullptr;
            if (b->prepared == b->nframes) st->issue_locked(b);
        }
        st->cv_state.wait(lk, [&] { return st->batches_in_flight == 0; });
    }
    for (size_t s = 0; s < st->slots.size(); ++s) {
        hjd_gdec* g = st->slots[s];
        if (!g->pending) continue;
        const int rc = hjd_gdec_sync(g, nullptr);
        if (rc) {
            std::lock_guard<std::mutex> lk(st->mu);
            st->record_error(rc, hjd_last_error());
        }
    }
    if (stats) {
        stats[0] = st->images;
        stats[1] = st->pixels;
        stats[2] = st->prep_ns;
        stats[3] = st->h2d_bytes;
        stats[4] = st->batches;
    }
    std::lock_guard<std::mutex> lk(st->mu);
    if (st->first_error != HJD_OK) {
        const int rc = st->first_error;
        st->first_error = HJD_OK;
        return set_error(rc, "%s", st->first_error_msg.c_str());
    }
    return HJD_OK;
}

int hjd_gstream_host_bytes(hjd_gstream* st, int64_t* host_scan_bytes)
{
    if (!st || !host_scan_bytes) return set_error(HJD_E_INVALID, "NULL argument");
    *host_scan_bytes = st->host_scan_bytes;
    return HJD_OK;
}

int hjd_gstream_destroy(hjd_gstream* st)
{
    if (!st) return HJD_OK;
    (void)hjd_gstream_sync(st, nullptr);
    {
        std::lock_guard<std::mutex> lk(st->mu);
        st->stop = true;
    }
    st->cv_jobs.notify_all();
    for (auto& t : st->workers) t.join();
    for (size_t s = 0; s < st->slots.size(); ++s) {
        delete st->slot_batch[s];
        if (st->slots[s]) hjd_gdec_destroy(st->slots[s]);
        if (st->streams[s]) (void)hipStreamDestroy(st->streams[s]);
        if (st->scratch[s]) (void)hipFree(st->scratch[s]);
    }
    delete st;
    return HJD_OK;
}

}  // extern "C"
