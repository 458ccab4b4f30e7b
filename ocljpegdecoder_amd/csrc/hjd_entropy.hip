// hjd_entropy.hip -- GPU entropy decoding of baseline JPEG scans (include/hjd_host.h,
// SURVEY.md s8(f) rank 3): the kernels and their launches, the
// only entropy unit with device code (the file map is in DESIGN.md s10).
//
// The host side prepares a batch (hjd_entropy_prep.cpp) under the layout of
// hjd_entropy_batch.hpp and hjd_gdec.hip issues it; hjd_entropy_emulate.cpp
// runs the same steps on the host.  Device side (one batch of frames per
// launch chain):
//   ent_sync_kernel   a group stages its bit window in LDS; each thread decodes
//                     its S-bit subsequence from a guessed entry, then the group
//                     iterates entry(k+1) = run(entry(k)) until nothing changes.
//                     Groups own 248 subsequences and also decode the 8 before
//                     them ("warm-up"), shared with the previous group;
//   ent_link_kernel   one thread per group: the chains of consecutive groups are
//                     joined if some warm-up entry equals the predecessor's entry
//                     for the same subsequence (a pure comparison, no decoding);
//   ent_fallback_kernel  frames with an unjoined boundary are redone sequentially
//                     (not seen on real data at the default S; correct anyway);
//   ent_write_kernel  ordered segmented scan of the statistics (block index, DC
//                     predictors) and a final run per subsequence that writes
//                     int16 zigzag blocks straight to HBM in MCU-major order;
// then the fused pixel kernel (hjd_kernels.hpp) turns the blocks into BGRX.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "hjd.h"
#include "hjd_entropy_batch.hpp"
#include "hjd_host.h"
#include "hjd_internal.h"

using hjd_internal::set_error;
using namespace hjd::ent;

#define HJD_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return set_error(HJD_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace {

// A frame's step tables from the batch's (ent_steps_kernel) into LDS.
__device__ __forceinline__ void copy_steps(uint8_t* steps, const EntBatchDev& b, const EntFrame& F, int tid,
                                           int nthreads)
{
    const uint4* src = reinterpret_cast<const uint4*>(b.steps_g + (static_cast<size_t>(F.tab_base) << kStepBits));
    uint4* dst = reinterpret_cast<uint4*>(steps);
    for (int i = tid; i < (F.ntab << kStepBits) / 16; i += nthreads) dst[i] = src[i];
}

// ---------------------------------------------------------------------------
// Kernels (gfx950)
// ---------------------------------------------------------------------------

// The frame's Huffman tables and block records into LDS (caller syncs).  The
// jinfo entries are read from the global frame record (a per-thread index into
// a register copy would put the record in scratch).
__device__ __forceinline__ void load_tables(HuffLut* lds, BlockInfo* blocks, const HuffLut* g, const EntFrame& F,
                                            const EntFrame* Fg, int tid, int nthreads)
{
    const u32x4* src = reinterpret_cast<const u32x4*>(g);
    u32x4* dst = reinterpret_cast<u32x4*>(lds);
    const int n = F.ntab * static_cast<int>(sizeof(HuffLut) / 16);
    for (int i = tid; i < n; i += nthreads) dst[i] = src[i];
    if (tid < kMaxBpm) blocks[tid] = block_info(Fg->jinfo[tid]);
}

__device__ __forceinline__ SubStats shfl_down_stats(const SubStats& s, int d)
{
    SubStats r;
    r.nblk = static_cast<uint32_t>(__shfl_down(static_cast<int>(s.nblk), d));
    r.flags = static_cast<uint32_t>(__shfl_down(static_cast<int>(s.flags), d));
    r.dc[0] = __shfl_down(s.dc[0], d);
    r.dc[1] = __shfl_down(s.dc[1], d);
    r.dc[2] = __shfl_down(s.dc[2], d);
    return r;
}

__device__ __forceinline__ SubStats shfl_up_stats(const SubStats& s, int d)
{
    SubStats r;
    r.nblk = static_cast<uint32_t>(__shfl_up(static_cast<int>(s.nblk), d));
    r.flags = static_cast<uint32_t>(__shfl_up(static_cast<int>(s.flags), d));
    r.dc[0] = __shfl_up(s.dc[0], d);
    r.dc[1] = __shfl_up(s.dc[1], d);
    r.dc[2] = __shfl_up(s.dc[2], d);
    return r;
}

// Ordered inclusive scan of one value per thread over the workgroup: each wave
// scans its 64 lanes by shuffles, then the waves' totals are combined through
// LDS (two barriers instead of two per step).  On return buf[t] holds thread
// t's inclusive result and the workgroup is synchronised.
template <int N = kGroupSubs>
__device__ __forceinline__ SubStats block_scan_inclusive(SubStats v, SubStats* buf, int tid)
{
    static_assert(N % 64 == 0 && N / 64 <= 16, "whole waves");
    const int lane = tid & 63, wv = tid >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const SubStats o = shfl_up_stats(v, d);
        if (lane >= d) v = stats_combine(o, v);
    }
    __shared__ SubStats wsum[N / 64];
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    SubStats pre = stats_identity();
    for (int w = 0; w < wv; ++w) pre = stats_combine(pre, wsum[w]);
    v = stats_combine(pre, v);
    buf[tid] = v;
    __syncthreads();
    return v;
}

// Ordered reduction over one wave's lanes (lane order = subsequence order);
// the result is valid in lane 0.
__device__ __forceinline__ SubStats wave_reduce_ordered(SubStats v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const SubStats o = shfl_down_stats(v, d);
        if ((lane & (2 * d - 1)) == 0) v = stats_combine(v, o);
    }
    return v;
}


// LDS layout of the sync kernel after the group's tables (dynamic shared memory).
struct SyncLds {
    uint64_t x[kGroupSubs];      // current exit of each subsequence
    uint64_t used[kGroupSubs];   // entry each subsequence was last run from
    SubStats st[kGroupSubs];     // statistics of that run
    uint16_t list[2][kGroupSubs];
    int32_t nlist[2];
    SubStats wsum[kGroupSubs / 64];
};

__host__ __device__ constexpr size_t sync_lds_bytes(uint32_t ntab)
{
    return (sizeof(HuffLut) + (1u << kStepBits)) * ntab + sizeof(SyncLds);
}

__global__ __launch_bounds__(kGroupSubs) void ent_sync_kernel(EntBatchDev b)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    HuffLut* tabs = reinterpret_cast<HuffLut*>(smem);
    uint8_t* steps = smem + sizeof(HuffLut) * b.ntab_max;
    SyncLds& L = *reinterpret_cast<SyncLds*>(smem + (sizeof(HuffLut) + (1u << kStepBits)) * b.ntab_max);
    const int tid = threadIdx.x;
    const uint32_t w = blockIdx.x;
    const uint32_t f = b.wg_frame[w];
    const EntFrame F = b.frames[f];
    const uint32_t gl = w - F.wg_base;
    const uint32_t S = b.sub_bits;
    // groups laid out for a device-destuffed frame's upper bound (raw bytes) past its real end
    if (gl >= frame_groups(F.nsub)) return;
    __shared__ BlockInfo blocks[kMaxBpm];
    const RunCtx c = make_ctx(b, F, tabs, blocks, steps);
    load_tables(tabs, blocks, b.tabs + F.tab_base, F, b.frames + f, tid, kGroupSubs);
    copy_steps(steps, b, F, tid, kGroupSubs);
    if (tid < 2) L.nlist[tid] = 0;
    __syncthreads();
    const int64_t k0 = group_sub(gl, 0);
    const int64_t k = k0 + tid;
    const bool valid = k >= 0 && k < static_cast<int64_t>(F.nsub);
    const uint32_t ku = static_cast<uint32_t>(k);
    // phase 1: every subsequence from its guessed entry, in two runs split at
    // its middle (the checkpoint), keeping the state there and the statistics
    // of the second half
    const uint32_t mid = ku * S + S / 2;
    uint64_t used = valid ? guess_entry(c, ku * S) : 0;
    SubStats st = stats_identity(), suf = stats_identity();
    uint64_t cp = used, x = used;
    // the write kernel decodes each subsequence as two halves, from the entry and
    // from the mid-state: every run that produces a subsequence's final entry
    // records its mid-state and first-half statistics (the last such run wins)
    const bool rec = valid && tid >= kWarm;
    if (valid) {
        cp = run<false>(c, used, mid, st, nullptr);
        if (rec) {
            b.mids[F.sub_base + ku] = cp;
            b.stats1[F.sub_base + ku] = st;
        }
        x = run<false>(c, cp, (ku + 1) * S, suf, nullptr);
        st = stats_combine(st, suf);
    }
    L.x[tid] = x;
    __syncthreads();
    // round 0, step A: every subsequence from its predecessor's exit, first to
    // the checkpoint only (all lanes busy).  A run that arrives in phase 1's
    // checkpoint state continues exactly as phase 1 did (a run is a function of
    // its state), so its exit and second-half statistics are known; the
    // others are "pending" and go on in step B.  Measured (syncstats): at
    // 4:2:0 53% of guessed runs are in step by mid-subsequence, at 4:4:4 94%,
    // so round 0 decodes 0.74 / 0.53 of the bits it decoded in full.
    bool pending = false;
    uint64_t resume = 0;
    if (valid && tid > 0 && k > 0) {
        const uint64_t e = L.x[tid - 1];
        if (!same_state(e, used)) {
            SubStats s2 = stats_identity();
            resume = run<false>(c, e, mid, s2, nullptr);
            if (rec) {
                b.mids[F.sub_base + ku] = resume;
                b.stats1[F.sub_base + ku] = s2;
            }
            used = e;
            if (same_state(resume, cp)) {
                st = stats_combine(s2, suf);
            } else {
                pending = true;
                st = s2;
            }
        }
    }
    L.used[tid] = used;
    L.st[tid] = st;
    __syncthreads();   // everyone has read L.x (old) before it is overwritten
    if (pending) {     // park the resume state where the exit goes
        L.x[tid] = resume;
        L.list[1][atomicAdd(&L.nlist[1], 1)] = static_cast<uint16_t>(tid);
    }
    __syncthreads();
    // step B: the pending second halves, compacted onto the first lanes
    if (tid < L.nlist[1]) {
        const int item = L.list[1][tid];
        const uint32_t kk = static_cast<uint32_t>(k0 + item);
        SubStats s2 = stats_identity();
        const uint64_t x2 = run<false>(c, L.x[item], (kk + 1) * S, s2, nullptr);
        L.st[item] = stats_combine(L.st[item], s2);
        L.x[item] = x2;
    }
    __syncthreads();
    // a changed exit changes the successor's entry
    if (pending && !same_state(L.x[tid], x) && tid + 1 < kGroupSubs && k + 1 < static_cast<int64_t>(F.nsub))
        L.list[0][atomicAdd(&L.nlist[0], 1)] = static_cast<uint16_t>(tid + 1);
    __syncthreads();
    // later rounds: only the subsequences whose entry changed, compacted onto the
    // first lanes, so idle waves do not replay a full decode
    for (int r = 0;; r ^= 1) {
        const int n = L.nlist[r];
        if (n == 0) break;
        uint64_t x2 = 0, e = 0;
        SubStats s2 = stats_identity();
        int item = -1;
        if (tid < n) {
            item = L.list[r][tid];
            e = L.x[item - 1];
            const uint32_t kk = static_cast<uint32_t>(k0 + item);
            if (!same_state(e, L.used[item])) {
                const uint64_t m2 = run<false>(c, e, kk * S + S / 2, s2, nullptr);
                if (item >= kWarm) {
                    b.mids[F.sub_base + kk] = m2;
                    b.stats1[F.sub_base + kk] = s2;
                }
                SubStats s3 = stats_identity();
                x2 = run<false>(c, m2, (kk + 1) * S, s3, nullptr);
                s2 = stats_combine(s2, s3);
            } else {
                item = -1;
            }
        }
        if (tid == 0) L.nlist[r ^ 1] = 0;
        __syncthreads();   // all reads of L.x done; the next list is empty
        if (item >= 0) {
            L.used[item] = e;
            L.st[item] = s2;
            if (!same_state(x2, L.x[item])) {
                L.x[item] = x2;
                if (item + 1 < kGroupSubs && k0 + item + 1 < static_cast<int64_t>(F.nsub))
                    L.list[r ^ 1][atomicAdd(&L.nlist[r ^ 1], 1)] = static_cast<uint16_t>(item + 1);
            }
        }
        __syncthreads();
    }
    const bool own = valid && tid >= kWarm;
    used = L.used[tid];
    st = L.st[tid];
    if (own) {
        b.entries[F.sub_base + ku] = used;
        b.stats[F.sub_base + ku] = st;
    } else if (tid < kWarm) {
        b.wentries[static_cast<uint64_t>(w) * kWarm + tid] = used;   // 0 for invalid (frame start group)
    }
    // statistics of the owned range: ordered reduce per wave, then across waves
    const SubStats ws = wave_reduce_ordered(own ? st : stats_identity(), tid & 63);
    if ((tid & 63) == 0) L.wsum[tid >> 6] = ws;
    __syncthreads();
    if (tid == 0) {
        SubStats a = L.wsum[0];
        for (int i = 1; i < kGroupSubs / 64; ++i) a = stats_combine(a, L.wsum[i]);
        b.agg[w] = a;
    }
}

// The AC step tables of every Huffman table of the batch, once per batch (the
// sync / spec / cand kernels copy their frame's from here instead of each
// workgroup deriving them from the LUTs).  Grid (tables, kStepGroups): one
// entry per thread, so the serial chain is one entry's few LUT lookups.
constexpr int kStepsThreads = 256;
constexpr int kStepGroups = (1 << kStepBits) / kStepsThreads;
static_assert(kStepGroups * kStepsThreads == (1 << kStepBits), "step groups");
__global__ __launch_bounds__(kStepsThreads) void ent_steps_kernel(EntBatchDev b)
{
    __shared__ HuffLut t;
    const uint32_t ti = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(b.tabs + ti);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&t);
    for (int i = tid; i < static_cast<int>(sizeof(t.lut) / 4); i += kStepsThreads) dst[i] = src[i];   // the LUT is all step_entry reads
    __syncthreads();
    const uint32_t e = blockIdx.y * kStepsThreads + static_cast<uint32_t>(tid);
    b.steps_g[(static_cast<size_t>(ti) << kStepBits) + e] = step_entry(t, e);
}

// ---- speculative sync (latency decoders) ------------------------------------
// Grid (groups, kMaxBpm): block (w, j) runs guess j of group w's owned
// subsequences (the warm-up ones belong to the previous group).
__global__ __launch_bounds__(kGroupSubs) void ent_spec_kernel(EntBatchDev b)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    HuffLut* tabs = reinterpret_cast<HuffLut*>(smem);
    uint8_t* steps = smem + sizeof(HuffLut) * b.ntab_max;
    __shared__ BlockInfo blocks[kMaxBpm];
    const int tid = threadIdx.x;
    const uint32_t w = blockIdx.x, j = blockIdx.y;
    const uint32_t f = b.wg_frame[w];
    const EntFrame F = b.frames[f];
    const uint32_t gl = w - F.wg_base;
    if (gl >= frame_groups(F.nsub) || j >= F.bpm) return;
    load_tables(tabs, blocks, b.tabs + F.tab_base, F, b.frames + f, tid, kGroupSubs);
    copy_steps(steps, b, F, tid, kGroupSubs);
    __syncthreads();
    const int64_t k = group_sub(gl, tid);
    if (tid < kWarm || k >= static_cast<int64_t>(F.nsub)) return;
    const RunCtx c = make_ctx(b, F, tabs, blocks, steps);
    const uint64_t row = static_cast<uint64_t>(F.sub_base) + static_cast<uint64_t>(k);
    if (j == 0) {   // the subsequence's slot map starts empty (ent_cand_kernel fills what exists)
        uint32_t* m = reinterpret_cast<uint32_t*>(b.cmap + row * kSlotRow);
#pragma unroll
        for (int i = 0; i < kSlotRow / 4; ++i) m[i] = 0xFFFFFFFFu;
    }
    b.spec[row * kMaxBpm + j] = spec_run(c, static_cast<uint32_t>(k), j, b.sub_bits, b.spec_lead);
}

// Grid (groups, kMaxBpm): block (w, i) runs candidate i of group w's owned
// subsequences, with its overflow continuation (cand_chain).
__global__ __launch_bounds__(kGroupSubs) void ent_cand_kernel(EntBatchDev b)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    HuffLut* tabs = reinterpret_cast<HuffLut*>(smem);
    uint8_t* steps = smem + sizeof(HuffLut) * b.ntab_max;
    __shared__ BlockInfo blocks[kMaxBpm];
    const int tid = threadIdx.x;
    const uint32_t w = blockIdx.x, i = blockIdx.y;
    const uint32_t f = b.wg_frame[w];
    const EntFrame F = b.frames[f];
    const uint32_t gl = w - F.wg_base;
    if (gl >= frame_groups(F.nsub) || i >= F.bpm) return;
    load_tables(tabs, blocks, b.tabs + F.tab_base, F, b.frames + f, tid, kGroupSubs);
    copy_steps(steps, b, F, tid, kGroupSubs);
    __syncthreads();
    const int64_t k = group_sub(gl, tid);
    if (tid < kWarm || k >= static_cast<int64_t>(F.nsub)) return;
    const RunCtx c = make_ctx(b, F, tabs, blocks, steps);
    cand_chain(c, b, F, static_cast<uint32_t>(k), i);
}

// One workgroup per frame walks the chain from the frame start (slot 0 of
// subsequence 0) through chunks of kChainChunk subsequences: the chunk's slot
// maps are loaded into LDS (coalesced), thread t composes its kChainRows
// consecutive rows into one function, the group scans those functions, and the
// chunk's entering slot under the prefix is thread t's entering slot.  Where
// the chain leaves every slot (an exit that is none of the successor's
// candidates even after the overflow levels; rare), thread 0 re-runs it from
// the known exit in the repair slot of the following subsequences until it
// lands in a slot again, and the chunk is scanned anew.  The output is the
// chain's slot of every subsequence (cslot): the write kernel reads each
// subsequence's entry, statistics and mid-state from that slot's record.  Last,
// one wave per group reduces the group's statistics (agg).
// Maps and functions are rows of kSlotRow bytes handled as 5 dwords; a lookup
// selects its byte in registers (LDS byte reads cost ~5x more here).
constexpr int kRowWords = kSlotRow / 4;

struct ChainLds {
    uint32_t rows[kChainChunk][kRowWords];      // the chunk's slot maps
    uint32_t fn[2][kChainThreads][kRowWords];   // scan of the threads' functions (double buffer)
    unsigned long long brk;                     // first break: subsequence << 8 | its predecessor's slot
    uint32_t carry;                             // slot entering the chunk
    uint32_t tables_loaded;
    HuffLut tabs[kMaxTables];                   // the frame's tables (repairs only)
    uint8_t steps[kMaxTables << kStepBits];
    BlockInfo blocks[kMaxBpm];
};

struct SlotRow {
    uint32_t w[kRowWords];
};

__device__ __forceinline__ uint32_t row_get(const SlotRow& r, uint32_t a)   // a < kChainSlots
{
    const uint32_t x = a < 8 ? (a < 4 ? r.w[0] : r.w[1]) : a < 16 ? (a < 12 ? r.w[2] : r.w[3]) : r.w[4];
    return (x >> ((a & 3) * 8)) & 0xFFu;
}

__device__ __forceinline__ SlotRow row_load(const uint32_t* p)
{
    SlotRow r;
#pragma unroll
    for (int i = 0; i < kRowWords; ++i) r.w[i] = p[i];
    return r;
}

// f then g: (g . f)(s) = g(f(s)), kNoCand absorbing; bytes past kChainSlots stay kNoCand
// (slot_compose, hjd_entropy.hpp: byte permutes, no per-slot selects)
static_assert(kRowWords == 5 && kNoCand == 0xFF, "slot_compose's row format");
__device__ __forceinline__ SlotRow row_compose(const SlotRow& f, const SlotRow& g)
{
    SlotRow r;
    slot_compose(f.w, g.w, r.w);
    return r;
}

__device__ __forceinline__ SlotRow slot_ident()
{
    SlotRow ident;
#pragma unroll
    for (int i = 0; i < kRowWords; ++i) ident.w[i] = 0xFFFFFFFFu;
#pragma unroll
    for (int s = 0; s < kChainSlots; ++s)
        ident.w[s >> 2] = (ident.w[s >> 2] & ~(0xFFu << ((s & 3) * 8))) | (static_cast<uint32_t>(s) << ((s & 3) * 8));
    return ident;
}

// Rows c0 .. c0 + cn of a frame's slot maps (cm) into rows[]: 4-byte words,
// coalesced, all of a thread's loads in flight at once; rows past cn: none.
__device__ __forceinline__ void chunk_load(uint32_t (*rows)[kRowWords], const uint8_t* cm, uint32_t c0, uint32_t cn,
                                           int tid)
{
    constexpr int kWords = kChainChunk * kRowWords / kChainThreads;   // 10
    const uint32_t* src = reinterpret_cast<const uint32_t*>(cm + static_cast<uint64_t>(c0) * kSlotRow);
    uint32_t* dst = &rows[0][0];
    const uint32_t nw = cn * kRowWords;
    uint32_t t[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) {
        const uint32_t j = static_cast<uint32_t>(tid + i * kChainThreads);
        t[i] = j < nw ? src[j] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int i = 0; i < kWords; ++i) dst[tid + i * kChainThreads] = t[i];
}

// Thread t composes its kChainRows rows of the loaded chunk; the group scans
// the functions (inclusive: fn[cur][t] = thread 0's rows then ... then t's).
// Call after the rows are visible (barrier); returns cur.
__device__ __forceinline__ int chunk_scan(uint32_t (*rows)[kRowWords], uint32_t (*fn)[kChainThreads][kRowWords],
                                          uint32_t cn, int tid)
{
    const uint32_t r0 = static_cast<uint32_t>(tid) * kChainRows;
    SlotRow v = slot_ident();
#pragma unroll 1
    for (uint32_t r = r0; r < r0 + kChainRows && r < cn; ++r) v = row_compose(v, row_load(rows[r]));
#pragma unroll
    for (int i = 0; i < kRowWords; ++i) fn[0][tid][i] = v.w[i];
    __syncthreads();
    int cur = 0;
#pragma unroll 1
    for (int d = 1; d < kChainThreads; d <<= 1) {
        const SlotRow mine = row_load(fn[cur][tid]);
        const SlotRow o = tid >= d ? row_compose(row_load(fn[cur][tid - d]), mine) : mine;
#pragma unroll
        for (int i = 0; i < kRowWords; ++i) fn[cur ^ 1][tid][i] = o.w[i];
        cur ^= 1;
        __syncthreads();
    }
    return cur;
}

// This thread's rows' chain slots (entering at `slot`) into cslot; returns the
// slot after its last row.
__device__ __forceinline__ uint32_t chunk_write_slots(const uint32_t (*rows)[kRowWords], uint8_t* cslot, uint32_t base,
                                                      uint32_t cn, int tid, uint32_t slot)
{
    const uint32_t r0 = static_cast<uint32_t>(tid) * kChainRows;
    uint32_t s = slot;
    uint32_t packed[(kChainRows + 3) / 4] = {};
#pragma unroll
    for (int i = 0; i < kChainRows; ++i) {
        packed[i >> 2] |= (s & 0xFFu) << ((i & 3) * 8);
        if (r0 + i < cn) s = row_get(row_load(rows[r0 + i]), s);
    }
    uint8_t* out = cslot + base + r0;
    if (kChainRows % 4 == 0 && r0 + kChainRows <= cn && ((base + r0) & 3) == 0) {
#pragma unroll
        for (int i = 0; i < kChainRows / 4; ++i) reinterpret_cast<uint32_t*>(out)[i] = packed[i];
    } else {
        for (uint32_t i = 0; i < kChainRows && r0 + i < cn; ++i) out[i] = static_cast<uint8_t>(packed[i >> 2] >> ((i & 3) * 8));
    }
    return s;
}

// Group g of frame F: the ordered reduction of its owned subsequences' chain
// statistics (one wave; lane = its lane) into agg, and the group marked linked.
__device__ __forceinline__ void group_agg(const EntBatchDev& b, const EntFrame& F, uint32_t g, int lane)
{
    const uint32_t w = F.wg_base + g;
    const uint32_t end = (g + 1) * kOwn < F.nsub ? (g + 1) * kOwn : F.nsub;
    SubStats q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // 4 x 64 >= kOwn; the four loads in flight together
        const uint32_t k = g * kOwn + static_cast<uint32_t>(lane) * 4 + i;
        q[i] = k < end ? sub_stats(b, F, k) : stats_identity();
    }
    SubStats a = stats_identity();
#pragma unroll
    for (int i = 0; i < 4; ++i) a = stats_combine(a, q[i]);
    a = wave_reduce_ordered(a, lane);
    if (lane == 0) {
        b.agg[w] = a;
        b.linked[w] = 1u;
    }
}

// Chunk [c0, c0 + cn) of frame F entered at slot `carry`, by one workgroup,
// repairing every break on the way (tid 0 runs the repair; the chunk's maps
// are reloaded after each, and a repair may run on into the next chunk's
// rows): writes the chunk's cslot and returns the slot after its last row.
__device__ __forceinline__ uint32_t walk_chunk(const EntBatchDev& b, uint32_t f, const EntFrame& F, ChainLds& L,
                                               uint32_t c0, uint32_t cn, uint32_t carry, int tid)
{
    const uint32_t n = F.nsub;
    uint8_t* cm = b.cmap + static_cast<uint64_t>(F.sub_base) * kSlotRow;
    const uint32_t r0 = static_cast<uint32_t>(tid) * kChainRows;   // this thread's rows within the chunk
    uint32_t slot;
    for (;;) {
        __syncthreads();
        chunk_load(L.rows, cm, c0, cn, tid);
        if (tid == 0) L.brk = ~0ull;
        __syncthreads();
        const int cur = chunk_scan(L.rows, L.fn, cn, tid);
        slot = tid == 0 ? carry : (carry == kNoCand ? kNoCand : row_get(row_load(L.fn[cur][tid - 1]), carry));
        // the first subsequence without a slot: the row whose map sends the
        // chain's slot to none (subsequence 0's slots all exist)
        uint32_t s = slot;
        for (uint32_t r = r0; r < r0 + kChainRows && r < cn && s != kNoCand; ++r) {
            const uint32_t nx = row_get(row_load(L.rows[r]), s);
            if (nx == kNoCand && c0 + r + 1 < n) {
                atomicMin(&L.brk, (static_cast<unsigned long long>(c0 + r + 1) << 8) | s);
                break;
            }
            s = nx;
        }
        __syncthreads();
        const unsigned long long brk = L.brk;
        if (brk == ~0ull) break;
        if (!L.tables_loaded) {   // the frame's tables, for the repair runs (rare)
            load_tables(L.tabs, L.blocks, b.tabs + F.tab_base, F, b.frames + f, tid, kChainThreads);
            __syncthreads();
            fill_steps(L.steps, L.tabs, F.ntab, tid, kChainThreads);
            __syncthreads();
            if (tid == 0) L.tables_loaded = 1;
        }
        if (tid == 0) {   // (the status bit tells the host a repair ran: hjd_gdec_sync)
            chain_repair(make_ctx(b, F, L.tabs, L.blocks, L.steps), b, F, static_cast<uint32_t>(brk >> 8),
                         static_cast<uint32_t>(brk & 0xFF));
            atomicOr(&b.status[f], kStatusFallback);
        }
    }
    // the chain's slot of each of this thread's rows
    const uint32_t s = chunk_write_slots(L.rows, b.cslot, F.sub_base + c0, cn, tid, slot);
    __syncthreads();
    if (r0 < cn && (r0 + kChainRows >= cn)) L.carry = s;   // the thread holding the chunk's last row
    __syncthreads();
    return L.carry;
}

// The serial walk of frame f by one workgroup (decoders without look-back words).
__device__ __forceinline__ void chain_walk(const EntBatchDev& b, uint32_t f, ChainLds& L, int tid)
{
    const EntFrame F = b.frames[f];
    const uint32_t n = F.nsub;
    if (tid == 0) L.tables_loaded = 0;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += kChainChunk)
        carry = walk_chunk(b, f, F, L, c0, n - c0 < static_cast<uint32_t>(kChainChunk) ? n - c0 : kChainChunk, carry, tid);
    const int wv = tid >> 6, lane = tid & 63;
    for (uint32_t g = wv; g < frame_groups(F.nsub); g += kChainThreads / 64) {
        group_agg(b, F, g, lane);
        if (b.agg2 && lane == 0) b.agg2[F.wg_base + g] = stats_identity();
    }
}

// Every frame walked serially (decoders without look-back words).
__global__ __launch_bounds__(kChainThreads) void ent_chain_kernel(EntBatchDev b)
{
    __shared__ ChainLds L;
    chain_walk(b, blockIdx.x, L, threadIdx.x);
}

// ---- the chain, chunks in parallel (the case without repairs) -----------------
// ent_chain_kernel's walk takes its chunks one after another (a lone FHD
// frame has 16 of 1024 subsequences; 1024 measured best for the look-back
// kernel: 17.3 us per FHD frame against 20.0 at 2048 and 19.8 at 512).  Where no repair is needed the chunks are
// independent given their entering slot, so one kernel over (chunk, frame)
// runs them side by side with a decoupled look-back: every chunk composes its
// maps into one function (the scan) and publishes it, then thread 0 finds the
// slot entering the chunk from the nearest published exit before it and the
// published maps in between (look-back words tagged with the launch's epoch,
// so nothing is cleared between launches; the tag has 24 bits, and the launch
// that takes it back to 1 clears every word first, gdec_issue, so a word of
// the launch one full cycle earlier is never read as this launch's),
// publishes its own exit, and the chunk writes its rows' slots.  A chunk whose predecessor has published
// nothing yet was dispatched after it (lower blockIdx.x first), so the wait
// ends.  Each chunk then reduces the chain statistics of the groups it holds:
// a group's part in its first chunk into agg, its part in the next into agg2
// (so no chunk waits for another's slots).  A chunk whose path leaves every
// slot repairs it itself (walk_chunk) before it publishes its exit; the maps
// send the chunks after it to none, and those wait for that exit instead.
// Breaks in different chunks are repaired side by side (the walk of a whole
// frame by one workgroup after any break cost ~50 us per break on a q90 4:4:4
// FHD frame).
struct ChainParLds {
    uint32_t rows[kChainChunk][kRowWords];
    uint32_t fn[2][kChainThreads][kRowWords];
    uint8_t slots[kChainChunk];   // the chain's slot of each row
    uint32_t carry, broken, published;
};
union ChainLbLds {
    ChainParLds p;
    ChainLds w;   // the walk, after the chunk's own work
};

// Ordered reduction (one wave) of the chain statistics of subsequences
// [lo, hi) of frame F (hi - lo <= 256), slots from LDS (row k at slots[k - c0]).
__device__ __forceinline__ SubStats range_stats(const EntBatchDev& b, const EntFrame& F, uint32_t lo, uint32_t hi,
                                                const uint8_t* slots, uint32_t c0, int lane)
{
    SubStats q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // the four loads in flight together
        const uint32_t k = lo + static_cast<uint32_t>(lane) * 4 + i;
        if (k < hi) {
            const uint64_t row = static_cast<uint64_t>(F.sub_base) + k;
            q[i] = stats_of(reinterpret_cast<const u32x4*>(b.cand + row * kCandRow + slots[k - c0])[1]);
        } else {
            q[i] = stats_identity();
        }
    }
    SubStats a = stats_identity();
#pragma unroll
    for (int i = 0; i < 4; ++i) a = stats_combine(a, q[i]);
    return wave_reduce_ordered(a, lane);
}

__global__ __launch_bounds__(kChainThreads) void ent_chain_lb_kernel(EntBatchDev b)
{
    __shared__ ChainLbLds U;
    ChainParLds& L = U.p;
    const int tid = threadIdx.x;
    const uint32_t c = blockIdx.x, f = blockIdx.y;
    const EntFrame F = b.frames[f];
    const uint32_t n = F.nsub, c0 = c * kChainChunk;
    if (c0 >= n) return;   // (uniform: past this frame's chunks, not counted)
    const uint32_t cn = n - c0 < static_cast<uint32_t>(kChainChunk) ? n - c0 : kChainChunk;
    if (tid == 0) L.broken = 0;
    chunk_load(L.rows, b.cmap + static_cast<uint64_t>(F.sub_base) * kSlotRow, c0, cn, tid);
    __syncthreads();
    const int cur = chunk_scan(L.rows, L.fn, cn, tid);
    // look-back (a word row per chunk: [0] epoch << 8 | exit slot, [1] epoch
    // once [2..6], the chunk's composed map, are written).  The map is published
    // first; the entry slot is then found by walking back to the nearest
    // published exit (chunk 0's entry is slot 0) and applying the maps of the
    // chunks in between, so no chunk waits for its predecessor's exit.
    uint32_t* const lb = b.chainfn + static_cast<uint64_t>(f) * b.chain_chunks * kLbWords;
    if (tid == 0) {   // (one thread writes the map and releases it)
        for (int i = 0; i < kRowWords; ++i) lb[c * kLbWords + 2 + i] = L.fn[cur][kChainThreads - 1][i];
        __hip_atomic_store(lb + c * kLbWords + 1, b.chain_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid < 64 && c <= 64) {   // wave 0: lane i < c reads chunk i's words, all in flight together
        const uint32_t i = static_cast<uint32_t>(tid);
        uint32_t ex = 0, m[kRowWords] = {};
        bool ready = i >= c;
        while (!ready) {
            ex = __hip_atomic_load(lb + i * kLbWords, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            ready = (ex >> 8) == b.chain_epoch ||
                    __hip_atomic_load(lb + i * kLbWords + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == b.chain_epoch;
            if (!ready) __builtin_amdgcn_s_sleep(1);
        }
        const bool has_exit = i < c && (ex >> 8) == b.chain_epoch;
        if (i < c && !has_exit)
            for (int k = 0; k < kRowWords; ++k) m[k] = lb[i * kLbWords + 2 + k];
        // from the last chunk before c with a published exit (else chunk 0,
        // entered at slot 0) through the maps of the chunks after it
        const uint64_t ballot = __ballot(has_exit);
        const int last = ballot ? 63 - __builtin_clzll(ballot) : -1;
        uint32_t sl = last >= 0 ? static_cast<uint32_t>(__shfl(static_cast<int>(ex & 0xFFu), last)) : 0u;
        for (int j = last + 1; j < static_cast<int>(c); ++j) {   // (uniform bounds: the whole wave shuffles)
            SlotRow r;
#pragma unroll
            for (int k = 0; k < kRowWords; ++k) r.w[k] = static_cast<uint32_t>(__shfl(static_cast<int>(m[k]), j));
            if (sl != kNoCand) sl = row_get(r, sl);
        }
        if (tid == 0) L.carry = sl;
    } else if (tid == 0 && c > 64) {   // a long frame: thread 0 walks back
        uint32_t j = c, carry = 0;   // carry: the slot entering chunk j
        while (j > 0) {
            const uint32_t v = __hip_atomic_load(lb + (j - 1) * kLbWords, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if ((v >> 8) == b.chain_epoch) {
                carry = v & 0xFFu;
                break;
            }
            if (__hip_atomic_load(lb + (j - 1) * kLbWords + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) ==
                b.chain_epoch)
                --j;   // its map is there: look further back
            else
                __builtin_amdgcn_s_sleep(1);
        }
        for (; j < c; ++j)   // forward through the maps of chunks j .. c-1
            if (carry != kNoCand) carry = row_get(row_load(lb + j * kLbWords + 2), carry);
        L.carry = carry;
    }
    // The maps send the chain to none where a chunk before this one breaks:
    // that chunk repairs itself and then publishes its exit, so wait for the
    // exit of chunk c - 1 (published exits are never none, but a frame's last
    // chunk's).  This chunk publishes its exit now unless its own path breaks.
    if (tid == 0) {
        uint32_t sl = L.carry;
        while (sl == kNoCand) {
            const uint32_t v = __hip_atomic_load(lb + (c - 1) * kLbWords, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if ((v >> 8) == b.chain_epoch)
                sl = v & 0xFFu;
            else
                __builtin_amdgcn_s_sleep(1);
        }
        const uint32_t exit = row_get(row_load(L.fn[cur][kChainThreads - 1]), sl);
        L.published = exit != kNoCand || c0 + cn >= n;
        if (L.published)
            __hip_atomic_store(lb + c * kLbWords, (b.chain_epoch << 8) | exit, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        L.carry = sl;
    }
    __syncthreads();
    const uint32_t carry = L.carry;
    const bool published = L.published;
    const uint32_t slot = tid == 0 ? carry : (carry == kNoCand ? kNoCand : row_get(row_load(L.fn[cur][tid - 1]), carry));
    // a row whose map sends the chain's slot to none, before the frame's last
    // subsequence: this chunk repairs it below (walk_chunk)
    const uint32_t r0 = static_cast<uint32_t>(tid) * kChainRows;
    uint32_t s = slot;
    for (uint32_t r = r0; r < r0 + kChainRows && r < cn; ++r) {
        L.slots[r] = static_cast<uint8_t>(s);
        if (s == kNoCand) continue;
        const uint32_t nx = row_get(row_load(L.rows[r]), s);
        if (nx == kNoCand && c0 + r + 1 < n) L.broken = 1;
        s = nx;
    }
    chunk_write_slots(L.rows, b.cslot, F.sub_base + c0, cn, tid, slot);
    __syncthreads();
    const bool broken = L.broken;
    const uint8_t* slots = L.slots;
    if (broken) {   // the walk's LDS overlays this kernel's: after the barrier above
        if (tid == 0) U.w.tables_loaded = 0;
        const uint32_t exit = walk_chunk(b, f, F, U.w, c0, cn, carry, tid);
        if (tid == 0 && !published)
            __hip_atomic_store(lb + c * kLbWords, (b.chain_epoch << 8) | exit, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        slots = b.cslot + F.sub_base + c0;   // (written by walk_chunk; its last barrier orders them)
    }
    // group statistics: each group part in this chunk, one wave per part
    const int wv = tid >> 6, lane = tid & 63;
    const uint32_t g0 = c0 / kOwn, g1 = (c0 + cn - 1) / kOwn;
    for (uint32_t g = g0 + static_cast<uint32_t>(wv); g <= g1; g += kChainThreads / 64) {
        const uint32_t glo = g * kOwn, ghi = (g + 1) * kOwn < n ? (g + 1) * kOwn : n;
        const uint32_t lo = glo > c0 ? glo : c0, hi = ghi < c0 + cn ? ghi : c0 + cn;
        const SubStats a = range_stats(b, F, lo, hi, slots, c0, lane);
        if (lane == 0) {
            const uint32_t w = F.wg_base + g;
            if (glo >= c0) {   // the group starts here
                b.agg[w] = a;
                b.linked[w] = 1u;
                if (ghi <= c0 + cn) b.agg2[w] = stats_identity();
            } else {
                b.agg2[w] = a;
            }
        }
    }
}

__global__ __launch_bounds__(256) void ent_link_kernel(EntBatchDev b)
{
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= b.nwg) return;
    const uint32_t f = b.wg_frame[w];
    const EntFrame F = b.frames[f];
    const uint32_t gl = w - F.wg_base;
    if (gl == 0 || gl >= frame_groups(F.nsub)) {   // first group, or past a device-destuffed frame's end
        b.linked[w] = 1;
        return;
    }
    bool joined = false;
    for (int t = 0; t < kWarm && !joined; ++t) {
        const uint64_t k = static_cast<uint64_t>(group_sub(gl, t));
        joined = same_state(b.wentries[static_cast<uint64_t>(w) * kWarm + t], b.entries[F.sub_base + k]);
    }
    b.linked[w] = joined ? 1u : 0u;
    if (!joined) atomicOr(&b.status[f], kStatusFallback);
}


__global__ __launch_bounds__(64) void ent_fallback_kernel(EntBatchDev b)
{
    __shared__ HuffLut tabs[kMaxTables];
    __shared__ BlockInfo blocks[kMaxBpm];
    const int lane = threadIdx.x;
    const uint32_t f = blockIdx.x;
    if (!(b.status[f] & kStatusFallback)) return;
    const EntFrame F = b.frames[f];
    load_tables(tabs, blocks, b.tabs + F.tab_base, F, b.frames + f, lane, 64);
    __syncthreads();
    if (lane == 0) repair_frame(b, f, tabs, blocks);
}

// Several threads per subsequence (write_pieces: halves, or quarters under the
// speculative sync, which records the quarter states): in workgroup (w, p)
// thread t decodes piece p of group subsequence t (from the state recorded at
// the piece's start to the next piece's), so each serial chain is S/2 or S/4
// bits long while the sync kernel keeps its S (the sync kernel
// is fastest at S = 4096, writing at 2048).  A run that starts inside a block
// skips to the next DC unit and a run finishes the block it started past its
// stop, so the pieces write disjoint blocks; a piece's block index and DC
// predictors are the subsequence's prefix combined with the statistics up to
// the piece's start.  The pieces are separate 256-thread workgroups: more CUs
// for a lone frame's few groups, one wave per SIMD.
constexpr int kWriteThreads = kGroupSubs;

// The write kernel's end: with b.host_status set, the last workgroup to
// finish copies the frames' status words into pinned host memory, so no
// status copy follows the kernels (the host reads them after the stream's
// completion event).  Every workgroup counts itself once; the status words
// were all final (agent-scope release) before its count.
__device__ __forceinline__ void write_done(const EntBatchDev& b, int tid)
{
    if (!b.host_status) return;
    __syncthreads();
    if (tid != 0) return;
    const uint32_t nwg = gridDim.x * gridDim.y;
    if (__hip_atomic_fetch_add(b.status + b.nframes, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != nwg - 1) return;
    for (uint32_t f = 0; f < b.nframes; ++f)
        b.host_status[f] = __hip_atomic_load(b.status + f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
}

__global__ __launch_bounds__(kWriteThreads) void ent_write_kernel(EntBatchDev b)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int16_t* stage = reinterpret_cast<int16_t*>(smem);                                  // [256][kStageStride]
    HuffLut* tabs = reinterpret_cast<HuffLut*>(smem + sizeof(int16_t) * kWriteThreads * kStageStride);
    SubStats* buf = reinterpret_cast<SubStats*>(stage);   // scan scratch before any block is staged
    static_assert(sizeof(SubStats) * kWriteThreads <= sizeof(int16_t) * kWriteThreads * kStageStride, "scratch");
    const int tid = threadIdx.x;
    const int t = tid;
    const uint32_t piece = blockIdx.y;
    const uint32_t w = blockIdx.x;
    const uint32_t f = b.wg_frame[w];
    const EntFrame F = b.frames[f];
    const uint32_t gl = w - F.wg_base;
    __shared__ BlockInfo blocks[kMaxBpm];
    if (gl < frame_groups(F.nsub) && piece < write_pieces(b)) {   // (uniform in the workgroup)
        load_tables(tabs, blocks, b.tabs + F.tab_base, F, b.frames + f, tid, kWriteThreads);
        // block index / DC predictors at this group's start: all previous groups of the frame
        SubStats pre = stats_identity();
        for (uint32_t base = 0; base < gl; base += kWriteThreads) {
            SubStats v = stats_identity();
            if (base + tid < gl) {
                v = b.agg[F.wg_base + base + tid];
                if (b.agg2) v = stats_combine(v, b.agg2[F.wg_base + base + tid]);
            }
            block_scan_inclusive<kWriteThreads>(v, buf, tid);
            const SubStats total = buf[kWriteThreads - 1];
            __syncthreads();
            pre = stats_combine(pre, total);
        }
        const int64_t k = group_sub(gl, t);
        const bool own = t >= kWarm && k < static_cast<int64_t>(F.nsub);
        const uint32_t ku = static_cast<uint32_t>(k);
        // subsequence prefixes
        const SubStats mine = own ? sub_stats(b, F, ku) : stats_identity();
        block_scan_inclusive<kWriteThreads>(mine, buf, tid);
        SubStats excl = stats_combine(pre, t > 0 ? buf[t - 1] : stats_identity());
        __syncthreads();   // scratch reads done before blocks are staged
        if (own) {
            SubStats lead;
            const uint64_t entry = piece_entry(b, F, ku, piece, lead);
            excl = stats_combine(excl, lead);
            const uint32_t stop = piece_stop(b, ku, piece);
            const RunCtx c = make_ctx(b, F, tabs, blocks);
            RunOut o;
            o.coefs = b.coefs + F.coef_off * 64;
            o.stage = stage + tid * kStageStride;
            o.blk = excl.nblk;
            o.nblocks = F.nblocks;
            o.nout = F.nout;
            o.pred[0] = excl.dc[0];
            o.pred[1] = excl.dc[1];
            o.pred[2] = excl.dc[2];
            SubStats st = stats_identity();
            run<true>(c, entry, stop, st, &o);
            uint32_t bad = (st.flags & kError) ? kStatusCorrupt : 0;
            if (piece + 1 == write_pieces(b) && ku == F.nsub - 1 && excl.nblk + st.nblk != F.nblocks) bad |= kStatusCount;
            if (bad) __hip_atomic_fetch_or(&b.status[f], bad, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    write_done(b, tid);
}

// ---------------------------------------------------------------------------
// Device destuff kernels.  The byte rules restate destuff() above (and T.81
// B.1.1.5 / F.1.2.3): every 0xFF is the first byte of a pair, so the fate of
// byte i depends only on (r[i-1], r[i], r[i+1]):
//   r[i] = FF: next 00 -> emit FF (stuffing); next FF -> drop (fill byte);
//              next D0..D7 -> drop, restart marker; no next byte or any other
//              next -> the scan ends here (EOI or another marker);
//   r[i] != FF after an FF: drop (the 00 of a stuffed pair, or RSTn's code);
//   otherwise emit r[i].
// ---------------------------------------------------------------------------

// Work split: a 256-thread group takes a 16-KiB tile in 4 passes; in pass p
// thread t takes the 16 bytes at p*4096 + 16t (one coalesced dwordx4 per lane).
// A lane classifies its 16 bytes with word-parallel tests: a 16-bit mask of
// 0xFF bytes, then a loop over those bytes only (0-1 per lane at q90: a 0xFF
// is ~1 byte in 256), giving a drop mask, a marker mask and the scan's end.
constexpr int kPasses = static_cast<int>(kTileBytes / (16 * kTileThreads));   // 4

struct Lane16 {
    uint64_t lo, hi;          // the 16 bytes, little-endian (byte 0 = first in the stream)
    uint32_t drop;            // bytes removed (stuffing 00, fill FF, RSTn pairs, everything from the end on)
    uint32_t marks;           // bit k: an RSTn pair starts at byte k
    uint32_t end;             // frame offset of the scan's end if it lies in these bytes, else kNoEnd
};

__device__ __forceinline__ uint32_t ff_mask4(uint32_t w)
{
    const uint32_t t = ~w;   // FF bytes -> 00; exact zero-byte test
    const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

__device__ __forceinline__ uint32_t byte_at(const Lane16& v, uint32_t k)
{
    return static_cast<uint32_t>((k < 8 ? v.lo >> (8 * k) : v.hi >> (8 * (k - 8))) & 0xFFu);
}

// Classify the 16 region bytes at s (16-B aligned): bytes before `begin` (not
// the scan's) and at or past `lim` (the region's length, or the known scan
// end) are dropped.  Nothing at or past `lim` is loaded: a lane whose 16 bytes
// start there (most of a frame's last tile) issues no load, and a lane that
// straddles it reads at most 15 bytes past the region, inside the 32-byte
// read-ahead every raw placement reserves (RawCursor::place).
__device__ __forceinline__ Lane16 classify16(const uint8_t* r, uint32_t s, uint32_t begin, uint32_t len, uint32_t lim)
{
    Lane16 v;
    v.marks = 0;
    v.end = kNoEnd;
    if (s >= lim) {
        v.lo = v.hi = 0;
        v.drop = 0xFFFFu;
        return v;
    }
    const u32x4 q = *reinterpret_cast<const u32x4*>(r + s);
    v.lo = static_cast<uint64_t>(q.x) | (static_cast<uint64_t>(q.y) << 32);
    v.hi = static_cast<uint64_t>(q.z) | (static_cast<uint64_t>(q.w) << 32);
    uint32_t drop = 0;
    if (lim - s < 16) drop = 0xFFFFu & ~((1u << (lim - s)) - 1u);
    uint32_t ff = ff_mask4(q.x) | (ff_mask4(q.y) << 4) | (ff_mask4(q.z) << 8) | (ff_mask4(q.w) << 12);
    if (s < begin) {                                // only in a frame's first 16 bytes (begin < 16)
        const uint32_t pre = (1u << (begin - s)) - 1u;
        drop |= pre;
        ff &= ~pre;
    }
    const uint32_t prev = s > begin ? r[s - 1] : 0u;
    if (prev == 0xFFu && !(ff & 1u)) drop |= 1u;   // second byte of a pair begun in the previous 16
    if (ff) {
        const uint32_t next16 = s + 16 < len ? r[s + 16] : 0u;
        while (ff) {
            const uint32_t k = __builtin_ctz(ff);
            ff &= ff - 1u;
            if (s + k >= lim) break;
            const bool has_next = s + k + 1 < len;
            const uint32_t nb = k < 15 ? byte_at(v, k + 1) : next16;
            const uint32_t pair = k < 15 ? 3u << k : 1u << k;   // this FF and its second byte, if in these 16
            if (has_next && nb == 0x00u) {
                drop |= (pair & ~(1u << k));                     // FF kept, 00 dropped
            } else if (has_next && nb == 0xFFu) {
                drop |= 1u << k;                                 // fill byte; the next FF leads a pair
            } else if (has_next && nb >= 0xD0u && nb <= 0xD7u) {
                drop |= pair;
                v.marks |= 1u << k;
            } else {                                             // EOI, another marker, or FF at the very end
                v.end = s + k;
                drop |= 0xFFFFu & ~((1u << k) - 1u);
                break;
            }
        }
    }
    v.drop = drop;
    return v;
}

// Pack the kept bytes of v to its low end (lowest first); returns their count.
__device__ __forceinline__ uint32_t compact16(Lane16& v)
{
    const uint32_t keep = ~v.drop & 0xFFFFu;
    const uint32_t n = __builtin_popcount(keep);
    if (n == 16) return n;
    // drops below the highest kept byte need a shift; process them from the top down
    uint32_t holes = v.drop & ((keep ? (2u << (31 - __builtin_clz(keep))) : 1u) - 1u);
    while (holes) {
        const uint32_t k = 31 - __builtin_clz(holes);
        holes &= ~(1u << k);
        if (k >= 8) {
            const uint32_t j = k - 8;
            const uint64_t low = j ? (~0ull >> (64 - 8 * j)) : 0ull;
            v.hi = (v.hi & low) | ((v.hi >> 8) & ~low);
        } else {
            const uint64_t low = k ? (~0ull >> (64 - 8 * k)) : 0ull;
            v.lo = (v.lo & low) | ((v.lo >> 8) & ~low) | (v.hi << 56);
            v.hi >>= 8;
        }
    }
    return n;
}

// Block-wide exclusive scan of two counters (256 threads); returns the totals.
__device__ __forceinline__ void block_scan2(uint32_t& a, uint32_t& b2, uint32_t& tot_a, uint32_t& tot_b, uint32_t* sa,
                                            uint32_t* sb)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t xa = a, xb = b2;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ya = __shfl_up(xa, d), yb = __shfl_up(xb, d);
        if (lane >= d) { xa += ya; xb += yb; }
    }
    if (lane == 63) { sa[wv] = xa; sb[wv] = xb; }
    __syncthreads();
    uint32_t ba = 0, bb = 0;
    for (int i = 0; i < wv; ++i) { ba += sa[i]; bb += sb[i]; }
    tot_a = sa[0] + sa[1] + sa[2] + sa[3];
    tot_b = sb[0] + sb[1] + sb[2] + sb[3];
    a = ba + xa - a;     // exclusive
    b2 = bb + xb - b2;
    __syncthreads();
}

__device__ __forceinline__ uint32_t lane_offset(uint32_t t, int p)
{
    return static_cast<uint32_t>(p) * (16u * kTileThreads) + 16u * t;
}

__global__ __launch_bounds__(kTileThreads) void destuff_count_kernel(EntBatchDev b)
{
    __shared__ uint32_t s_end, sa[4], sb[4];
    const uint32_t t = blockIdx.x;
    const uint32_t f = b.tile_frame[t];
    const RawFrame R = b.rawf[f];
    const uint8_t* r = b.raw + (R.raw_off - R.begin);
    const uint32_t L = raw_region_len(R.begin, R.raw_len);
    const uint32_t s0 = (t - R.tile_base) * kTileBytes;
    if (threadIdx.x == 0) s_end = kNoEnd;
    __syncthreads();
    uint32_t ne[kPasses], nm[kPasses], end = kNoEnd;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        const uint32_t s = s0 + lane_offset(threadIdx.x, p);
        const Lane16 v = classify16(r, s, R.begin, L, L);
        ne[p] = __builtin_popcount(~v.drop & 0xFFFFu);
        nm[p] = __builtin_popcount(v.marks);
        end = min(end, v.end);
    }
    if (end != kNoEnd) atomicMin(&s_end, end);
    __syncthreads();
    const uint32_t tile_end = s_end;
    uint32_t te = 0, tm = 0;
#pragma unroll
    for (int p = 0; p < kPasses; ++p)          // what lies past the scan's end does not count
        if (s0 + lane_offset(threadIdx.x, p) <= tile_end) { te += ne[p]; tm += nm[p]; }
    uint32_t x = te, y = tm;
    block_scan2(x, y, te, tm, sa, sb);
    if (threadIdx.x == 0) {
        b.tiles[t] = te;
        b.tiles[b.ntiles + t] = tm;
        b.tiles[2 * b.ntiles + t] = tile_end;
    }
}

// One group per frame: tile offsets (exclusive scans), the frame's length,
// subsequence count, segment table tail and read-ahead pad; malformed scans
// are flagged kStatusCorrupt (what destuff()/prepare() reject on the host).
__global__ __launch_bounds__(kTileThreads) void destuff_scan_kernel(EntBatchDev b)
{
    __shared__ uint32_t sa[4], sb[4], s_stop;
    const uint32_t f = blockIdx.x;
    RawFrame& R = b.rawf[f];
    if (R.ntiles == 0) return;
    EntFrame& F = const_cast<EntFrame*>(b.frames)[f];
    const int tid = threadIdx.x;
    uint32_t carry_e = 0, carry_m = 0, end = kNoEnd;
    for (uint32_t c0 = 0; c0 < R.ntiles; c0 += kTileThreads) {
        const uint32_t j = c0 + tid;
        const uint32_t t = R.tile_base + j;
        uint32_t e = 0, m = 0, te = kNoEnd;
        if (j < R.ntiles) {
            e = b.tiles[t];
            m = b.tiles[b.ntiles + t];
            te = b.tiles[2 * b.ntiles + t];
        }
        if (tid == 0) s_stop = kNoEnd;
        __syncthreads();
        if (te != kNoEnd) atomicMin(&s_stop, j);     // first tile of the chunk holding the scan's end
        __syncthreads();
        const uint32_t stop = s_stop;
        if (j > stop) e = m = 0;
        uint32_t xe = e, xm = m, tot_e, tot_m;
        block_scan2(xe, xm, tot_e, tot_m, sa, sb);
        if (j < R.ntiles) {
            b.tiles[t] = carry_e + xe;               // byte offset of the tile's output
            b.tiles[b.ntiles + t] = carry_m + xm;    // index of its first marker
        }
        carry_e += tot_e;
        carry_m += tot_m;
        if (stop != kNoEnd) {
            if (tid == 0) s_stop = b.tiles[2 * b.ntiles + R.tile_base + stop];
            __syncthreads();
            end = s_stop;
            break;
        }
    }
    const uint32_t total = carry_e, markers = carry_m;
    const uint32_t bits = total * 8;
    uint32_t* seg = const_cast<uint32_t*>(b.seg_end) + F.seg_base;
    for (uint32_t k = min(markers, F.nseg - 1) + tid; k < F.nseg; k += kTileThreads) seg[k] = bits;
    uint8_t* out = const_cast<uint8_t*>(b.data) + F.data_off + total;
    if (tid < static_cast<int>(kDataPad)) out[tid] = 0xFF;
    if (tid == 0) {
        R.end = end == kNoEnd ? raw_region_len(R.begin, R.raw_len) : end;
        F.data_bits = bits;
        F.nsub = (bits + b.sub_bits - 1) / b.sub_bits;
        if (total == 0 || total >= (1u << 28) || markers != F.nseg - 1) atomicOr(&b.status[f], kStatusCorrupt);
    }
}

__global__ __launch_bounds__(kTileThreads) void destuff_write_kernel(EntBatchDev b)
{
    __shared__ uint32_t sa[4], sb[4];
    __shared__ uint32_t stage[kTileBytes / 4 + 8];      // output bytes of the tile, word-aligned to the output
    const uint32_t t = blockIdx.x;
    const uint32_t f = b.tile_frame[t];
    const RawFrame R = b.rawf[f];
    const EntFrame F = b.frames[f];
    const uint8_t* r = b.raw + (R.raw_off - R.begin);
    const uint32_t L = raw_region_len(R.begin, R.raw_len);
    const uint32_t s0 = (t - R.tile_base) * kTileBytes;
    const uint32_t tile_out = b.tiles[t];
    uint32_t mark_base = b.tiles[b.ntiles + t];
    const uint32_t base = tile_out & ~3u;              // stage word 0 <-> output byte `base`
    const uint32_t lo = tile_out - base;
    for (uint32_t i = threadIdx.x; i < kTileBytes / 4 + 8; i += kTileThreads) stage[i] = 0u;
    __syncthreads();
    uint32_t* seg = const_cast<uint32_t*>(b.seg_end) + F.seg_base;
    uint32_t out_pos = lo;                             // stage byte of this pass's first output
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        const uint32_t s = s0 + lane_offset(threadIdx.x, p);
        Lane16 v = classify16(r, s, R.begin, L, R.end);
        const uint32_t marks = v.marks;                // classify16 stops at the scan's end
        const uint32_t kept_mask = ~v.drop & 0xFFFFu;
        uint32_t n = __builtin_popcount(kept_mask), nm = __builtin_popcount(marks), pe, pm;
        uint32_t xe = n, xm = nm;
        block_scan2(xe, xm, pe, pm, sa, sb);
        // restart markers: ordinal and the destuffed bit offset where the interval ends
        uint32_t mm = marks, ord = mark_base + xm;
        while (mm) {
            const uint32_t k = __builtin_ctz(mm);
            mm &= mm - 1u;
            const uint32_t code = (k < 15 ? byte_at(v, k + 1) : r[s + 16]) - 0xD0u;
            if (code != (ord & 7u)) atomicOr(b.status + f, kStatusCorrupt);   // RSTn out of order
            if (ord + 1 < F.nseg)
                seg[ord] = (tile_out + (out_pos - lo) + xe + __builtin_popcount(kept_mask & ((1u << k) - 1u))) * 8;
            ++ord;
        }
        if (n) {   // the kept bytes, packed, OR-ed into the staged words they cover
            compact16(v);
            const uint32_t o = out_pos + xe;
            const uint32_t sh = 8 * (o & 3u);
            uint32_t w[5];
            const uint32_t x0 = static_cast<uint32_t>(v.lo), x1 = static_cast<uint32_t>(v.lo >> 32);
            const uint32_t x2 = static_cast<uint32_t>(v.hi), x3 = static_cast<uint32_t>(v.hi >> 32);
            // mask off bytes past n before shifting (their content is stale)
            uint32_t m0 = n >= 4 ? ~0u : (1u << (8 * n)) - 1u;
            uint32_t m1 = n >= 8 ? ~0u : n <= 4 ? 0u : (1u << (8 * (n - 4))) - 1u;
            uint32_t m2 = n >= 12 ? ~0u : n <= 8 ? 0u : (1u << (8 * (n - 8))) - 1u;
            uint32_t m3 = n >= 16 ? ~0u : n <= 12 ? 0u : (1u << (8 * (n - 12))) - 1u;
            const uint32_t y0 = x0 & m0, y1 = x1 & m1, y2 = x2 & m2, y3 = x3 & m3;
            if (sh) {
                w[0] = y0 << sh;
                w[1] = (y1 << sh) | (y0 >> (32 - sh));
                w[2] = (y2 << sh) | (y1 >> (32 - sh));
                w[3] = (y3 << sh) | (y2 >> (32 - sh));
                w[4] = y3 >> (32 - sh);
            } else {
                w[0] = y0; w[1] = y1; w[2] = y2; w[3] = y3; w[4] = 0u;
            }
            const uint32_t wbase = o >> 2, nw = (8 * n + sh + 31) / 32;
#pragma unroll
            for (int i = 0; i < 5; ++i)
                if (static_cast<uint32_t>(i) < nw) atomicOr(&stage[wbase + i], w[i]);
        }
        out_pos += pe;
        mark_base += pm;
    }
    __syncthreads();
    // coalesced word stores; the partial words at the tile's two ends by bytes
    uint8_t* out = const_cast<uint8_t*>(b.data) + F.data_off;
    const uint32_t nbytes = out_pos;                   // = lo + the tile's output bytes
    const uint32_t nwords = (nbytes + 3) / 4;
    const uint8_t* sb8 = reinterpret_cast<const uint8_t*>(stage);
    for (uint32_t i = threadIdx.x; i < nwords; i += kTileThreads) {
        const uint32_t b0 = 4 * i, b1 = min(b0 + 4, nbytes);
        if (b0 >= lo && b1 == b0 + 4) {
            *reinterpret_cast<uint32_t*>(out + base + b0) = stage[i];
        } else {
            for (uint32_t k = max(b0, lo); k < b1; ++k) out[base + k] = sb8[k];
        }
    }
}

}  // namespace

int hjd::ent::launch_entropy(const EntBatchDev& b, const uint8_t* tabs_h, std::vector<uint8_t>& steps_tabs,
                             hipStream_t s)
{
    if (b.nwg == 0) return HJD_OK;
    if (b.ntiles) {
        hipLaunchKernelGGL(destuff_count_kernel, dim3(b.ntiles), dim3(kTileThreads), 0, s, b);
        HJD_HIP(hipGetLastError());
        hipLaunchKernelGGL(destuff_scan_kernel, dim3(b.nframes), dim3(kTileThreads), 0, s, b);
        HJD_HIP(hipGetLastError());
        hipLaunchKernelGGL(destuff_write_kernel, dim3(b.ntiles), dim3(kTileThreads), 0, s, b);
        HJD_HIP(hipGetLastError());
    }
    // the step tables depend on the Huffman tables only: a batch whose tables
    // (in batch order) are the previous batch's reuses them
    const size_t tabs_n = sizeof(HuffLut) * b.ntab_total;
    if (steps_tabs.size() != tabs_n || memcmp(steps_tabs.data(), tabs_h, tabs_n) != 0) {
        hipLaunchKernelGGL(ent_steps_kernel, dim3(b.ntab_total, kStepGroups), dim3(kStepsThreads), 0, s, b);
        HJD_HIP(hipGetLastError());
        steps_tabs.assign(tabs_h, tabs_h + tabs_n);
    }
    if (b.spec) {   // speculative sync: latency decoders
        const size_t tl = (sizeof(HuffLut) + (1u << kStepBits)) * b.ntab_max;
        hipLaunchKernelGGL(ent_spec_kernel, dim3(b.nwg, kMaxBpm), dim3(kGroupSubs), tl, s, b);
        HJD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ent_cand_kernel, dim3(b.nwg, kMaxBpm), dim3(kGroupSubs), tl, s, b);
        HJD_HIP(hipGetLastError());
        if (b.chain_broken)   // chunks in parallel (+ group records; a broken frame's last chunk walks it)
            hipLaunchKernelGGL(ent_chain_lb_kernel, dim3(b.chain_chunks, b.nframes), dim3(kChainThreads), 0, s, b);
        else   // every frame walked
            hipLaunchKernelGGL(ent_chain_kernel, dim3(b.nframes), dim3(kChainThreads), 0, s, b);
        HJD_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(ent_sync_kernel, dim3(b.nwg), dim3(kGroupSubs), sync_lds_bytes(b.ntab_max), s, b);
        HJD_HIP(hipGetLastError());
        hipLaunchKernelGGL(ent_link_kernel, dim3((b.nwg + 255) / 256), dim3(256), 0, s, b);
        HJD_HIP(hipGetLastError());
    }
    if (!b.spec) {   // the chain kernel repairs its chains itself: never a fallback
        hipLaunchKernelGGL(ent_fallback_kernel, dim3(b.nframes), dim3(64), 0, s, b);
        HJD_HIP(hipGetLastError());
    }
    constexpr size_t kStageBytes = sizeof(int16_t) * kWriteThreads * kStageStride;
    hipLaunchKernelGGL(ent_write_kernel, dim3(b.nwg, write_pieces(b)), dim3(kWriteThreads),
                       kStageBytes + sizeof(HuffLut) * b.ntab_max, s, b);
    HJD_HIP(hipGetLastError());
    return HJD_OK;
}

// Latency decoders: the staged bytes of a batch whose scans were all
// destuffed on the host (its header, then its data area) are pulled from the
// pinned staging by one kernel instead of two DMA copies: 1 MB moves in 23 us
// against 31 us by DMA (tools/h2d_probe.hip, profiles/r06y_h2d_probe.json;
// 64 workgroups beat 256 and 1024), and the kernel replaces the copy calls.
// Staging and blob share their layout, so a segment is an offset and a length
// (16-B multiples: the header is kAlign-aligned, a data run ends in its pad).
namespace {

constexpr int kPullBlocks = 64;
constexpr int kPullThreads = 256;

__global__ __launch_bounds__(kPullThreads) void pull_kernel(const u32x4* src, u32x4* dst, PullSegs p)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kPullThreads;
    for (uint32_t k = 0; k < p.n; ++k)
        for (uint64_t w = blockIdx.x * static_cast<uint64_t>(kPullThreads) + threadIdx.x; w < p.words[k]; w += stride)
            dst[p.off[k] + w] = src[p.off[k] + w];
}

}  // namespace

hipError_t hjd::ent::launch_pull(const uint8_t* src, uint8_t* dst, const PullSegs& segs, hipStream_t s)
{
    hipLaunchKernelGGL(pull_kernel, dim3(kPullBlocks), dim3(kPullThreads), 0, s, reinterpret_cast<const u32x4*>(src),
                       reinterpret_cast<u32x4*>(dst), segs);
    return hipGetLastError();
}

// Test hook for the destuff step alone (the host routine: hjd_debug_destuff_host):
// the three device kernels on one raw scan, so arbitrary byte strings (stuffing,
// fill bytes, RSTn in and out of order, truncation) can be compared directly.
extern "C" {

int hjd_debug_destuff_gpu(hjd_ctx* ctx, const uint8_t* scan, size_t n, int nseg, uint8_t* out, size_t cap,
                          uint32_t* seg_end, int64_t* out_bytes, uint32_t* status)
{
    if (!ctx || !scan || !out || !seg_end || !out_bytes || !status || n == 0 || nseg < 1 || cap < n + kDataPad)
        return set_error(HJD_E_INVALID, "invalid destuff arguments");
    HJD_HIP(hipSetDevice(hjd_ctx_device(ctx)));
    const uint32_t ntiles = static_cast<uint32_t>((n + kTileBytes - 1) / kTileBytes);
    const size_t area = align_up(n + kDataPad, 16);
    EntFrame F;
    memset(&F, 0, sizeof(F));
    F.nseg = static_cast<uint32_t>(nseg);
    F.data_bits = static_cast<uint32_t>(n * 8);
    RawFrame R{0, static_cast<uint32_t>(n), 0, 0, ntiles, 0, 0};
    std::vector<uint32_t> tf(ntiles, 0);
    uint8_t *d_raw = nullptr, *d_out = nullptr;
    EntFrame* d_f = nullptr;
    RawFrame* d_r = nullptr;
    uint32_t *d_tf = nullptr, *d_tiles = nullptr, *d_seg = nullptr, *d_status = nullptr;
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t x) { if (e == hipSuccess) e = x; return e == hipSuccess; };
    if (ok(hipMalloc(&d_raw, area)) && ok(hipMalloc(&d_out, area)) && ok(hipMalloc(&d_f, sizeof(F))) &&
        ok(hipMalloc(&d_r, sizeof(R))) && ok(hipMalloc(&d_tf, 4 * ntiles)) && ok(hipMalloc(&d_tiles, 12 * ntiles)) &&
        ok(hipMalloc(&d_seg, 4 * static_cast<size_t>(nseg))) && ok(hipMalloc(&d_status, 4)) &&
        ok(hipMemcpy(d_raw, scan, n, hipMemcpyHostToDevice)) && ok(hipMemcpy(d_f, &F, sizeof(F), hipMemcpyHostToDevice)) &&
        ok(hipMemcpy(d_r, &R, sizeof(R), hipMemcpyHostToDevice)) &&
        ok(hipMemcpy(d_tf, tf.data(), 4 * ntiles, hipMemcpyHostToDevice)) && ok(hipMemset(d_status, 0, 4)) &&
        ok(hipMemset(d_seg, 0xEE, 4 * static_cast<size_t>(nseg))) && ok(hipMemset(d_out, 0xEE, area))) {
        EntBatchDev b;
        memset(&b, 0, sizeof(b));
        b.frames = d_f;
        b.seg_end = d_seg;
        b.data = d_out;
        b.status = d_status;
        b.nframes = 1;
        b.sub_bits = 4096;
        b.raw = d_raw;
        b.rawf = d_r;
        b.tile_frame = d_tf;
        b.tiles = d_tiles;
        b.ntiles = ntiles;
        hipLaunchKernelGGL(destuff_count_kernel, dim3(ntiles), dim3(kTileThreads), 0, 0, b);
        hipLaunchKernelGGL(destuff_scan_kernel, dim3(1), dim3(kTileThreads), 0, 0, b);
        hipLaunchKernelGGL(destuff_write_kernel, dim3(ntiles), dim3(kTileThreads), 0, 0, b);
        EntFrame Fo;
        if (ok(hipGetLastError()) && ok(hipDeviceSynchronize()) &&
            ok(hipMemcpy(&Fo, d_f, sizeof(Fo), hipMemcpyDeviceToHost)) &&
            ok(hipMemcpy(out, d_out, area, hipMemcpyDeviceToHost)) &&
            ok(hipMemcpy(seg_end, d_seg, 4 * static_cast<size_t>(nseg), hipMemcpyDeviceToHost)) &&
            ok(hipMemcpy(status, d_status, 4, hipMemcpyDeviceToHost)))
            *out_bytes = Fo.data_bits / 8;
    }
    for (void* p : {static_cast<void*>(d_raw), static_cast<void*>(d_out), static_cast<void*>(d_f),
                    static_cast<void*>(d_r), static_cast<void*>(d_tf), static_cast<void*>(d_tiles),
                    static_cast<void*>(d_seg), static_cast<void*>(d_status)})
        if (p) (void)hipFree(p);
    if (e != hipSuccess) return set_error(HJD_E_HIP, "destuff test hook: %s", hipGetErrorString(e));
    return HJD_OK;
}

}  // extern "C"
