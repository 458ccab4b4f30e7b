// hjd_entropy_batch.hpp -- the layout of one GPU entropy batch, shared by the
// host units that stage it (hjd_entropy_prep.cpp, hjd_gdec.hip), the gfx950
// kernels that decode it (hjd_entropy.hip) and their host emulation
// (hjd_entropy_emulate.cpp): the header's parts, the kernel argument, and the
// __host__ __device__ steps built on them.  Plain C++ outside hipcc, as
// hjd_entropy.hpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include "hjd_entropy.hpp"
#include "hjd_internal.h"

namespace hjd {
namespace ent {

using hjd_internal::align_up;

constexpr size_t kDataPad = 64;      // readable bytes after each frame's bit string (16-B chunks read ahead)
constexpr size_t kAlign = 256;
constexpr int kMaxScans = 3;         // sequential: one scan per component at most (T.81 B.2.3)

constexpr int kDestuffHost = 0;          // memchr/memcpy destuff into pinned staging (destuff())
constexpr int kDestuffFromCaller = 1;    // raw bytes DMA'd from the caller's pinned buffer, destuffed on the GPU
constexpr int kDestuffFromStaging = 2;   // raw bytes memcpy'd into pinned staging, destuffed on the GPU

// Device destuff ("Destuff on the GPU").  A frame whose scan
// bytes reach the device raw (straight from the caller's pinned buffer, or
// copied into pinned staging) is destuffed by three kernels over 16-KiB tiles:
// count -> per-frame scan -> write.  Its destuffed bit string lands where a
// host-destuffed frame's would, at data_off of the data area, so the entropy
// kernels are unchanged; the host only parses the header.
constexpr uint32_t kTileBytes = 16384;
constexpr int kTileThreads = 256;
constexpr uint32_t kNoEnd = 0xFFFFFFFFu;

// The raw bytes of a frame sit at any byte offset of the raw area (so that
// frames adjacent in the caller's memory stay adjacent there and move in one
// DMA); the kernels address them from the 16-B aligned `raw_off - begin` in
// "region" coordinates [0, begin + raw_len) and ignore the first `begin` bytes.
struct RawFrame {          // one per frame of a batch (32 B)
    uint64_t raw_off;      // raw area offset of the first scan byte
    uint32_t raw_len;      // scan bytes from the end of the SOS header to the end of the file
    uint32_t begin;        // raw_off & 15
    uint32_t tile_base;    // first tile of the frame
    uint32_t ntiles;       // 0: destuffed on the host
    uint32_t end;          // region offset where the scan ends (destuff_scan_kernel)
    uint32_t pad;
};
static_assert(sizeof(RawFrame) == 32, "RawFrame layout");

__host__ __device__ __forceinline__ uint32_t raw_region_len(uint32_t begin, uint32_t raw_len) { return begin + raw_len; }

// ---------------------------------------------------------------------------
// Batch layout.  The header (frames | tables | segment ends | group->frame map |
// pixel-kernel records | natural-order qtables) is laid out compactly per batch
// at offset 0; the destuffed scans live at the fixed offset `data`.  Pinned
// staging and the device blob use the same layout, so one copy moves each part.
// ---------------------------------------------------------------------------
struct Caps {
    int max_frames;
    int64_t max_scan_bytes, max_blocks;
    int sub_bits;
    int64_t max_subs, max_wgs, max_segs, max_tiles;
    size_t hdr_cap, data;
};

// Bytes of a batch's pixel-kernel frame tables, one per sampling class
// (hjd_internal::frame_table): the classes share the batch's n records, and
// each carries its own norm record.
inline size_t pixel_tables_bytes(int n, bool roi, bool norm)
{
    return hjd_internal::frame_table(n, roi, norm).bytes +
           (hjd_internal::kSamplingClasses - 1) * hjd_internal::frame_table(0, roi, norm).bytes;
}

inline Caps make_caps(int max_frames, int64_t max_scan_bytes, int64_t max_blocks, int sub_bits)
{
    Caps c;
    c.max_frames = max_frames;
    c.max_scan_bytes = max_scan_bytes;
    c.max_blocks = max_blocks;
    c.sub_bits = sub_bits;
    // entropy frames: one per scan, kMaxScans per JPEG at most
    const int64_t ef = static_cast<int64_t>(max_frames) * kMaxScans;
    c.max_subs = (max_scan_bytes * 8 + sub_bits - 1) / sub_bits + ef;
    c.max_wgs = (c.max_subs + kOwn - 1) / kOwn + ef;
    // restart segments: one per restart interval; a non-interleaved scan (or a
    // gray file) with Ri = 1 has one per block, so blocks + one per entropy frame
    c.max_segs = max_blocks + ef;
    c.max_tiles = max_scan_bytes / kTileBytes + max_frames;
    // (the ResizeRecords: a resized call's records follow the pixel kernel's
    // tables, two per frame with the antialiased filter; an oriented call's
    // OrientRecords lie between the two; a warped call's WarpRecords take
    // their place; a colour call's ColorRecords, a filter call's ConvRecords
    // and a tone call's ToneRecords follow either, in that order)
    const size_t per_frame = (sizeof(EntFrame) + sizeof(HuffLut) * kMaxTables + 8) * kMaxScans + 192 * 4 +
                             sizeof(RawFrame) + 4 + 2 * sizeof(hjd_internal::ResizeRecord) +
                             sizeof(hjd_internal::OrientRecord) + sizeof(hjd_internal::WarpRecord) +
                             sizeof(hjd_internal::ColorRecord) + sizeof(hjd_internal::ConvRecord) +
                             sizeof(hjd_internal::ToneRecord);
    // + the pixel kernel's frame tables at their largest (a ROI call in a float format)
    c.hdr_cap = align_up(per_frame * max_frames + 4 * static_cast<size_t>(c.max_segs + c.max_wgs + c.max_tiles) +
                             pixel_tables_bytes(max_frames, true, true) + 11 * kAlign, kAlign);
    c.data = c.hdr_cap;
    return c;
}

struct HdrOffsets {
    size_t frames, tabs, seg, wg, recs, qt, rawf, tilef, status, used;
};

// Device-side view of a batch (kernel argument).
struct EntBatchDev {
    const EntFrame* frames;
    const HuffLut* tabs;
    const uint32_t* seg_end;
    const uint32_t* wg_frame;
    const uint8_t* data;
    uint64_t* entries;
    SubStats* stats;
    uint64_t* mids;       // [sub] verified state at the first unit boundary >= k*S + S/2
    SubStats* stats1;     // [sub] statistics of the first half (entry -> mid)
    uint64_t* wentries;   // [group][kWarm] warm-up entries
    uint32_t* linked;     // [group] 1 if joined to the previous group's chain
    SubStats* agg;
    SubStats* agg2;       // [group] null, or the rest of agg: a group's statistics in the next chain chunk
    uint32_t* status;     // [nframes], ent_write_kernel's finished-workgroup count, [nframes] chain chunk counts
    uint32_t* host_status;   // null, or pinned host words the last write workgroup copies status to
    int16_t* coefs;
    uint32_t nframes, nwg, sub_bits, ntab_max;   // ntab_max: tables of the largest frame (dynamic LDS)
    uint32_t ntab_total;                         // tables of the batch
    uint8_t* steps_g;                            // [table][1 << kStepBits] AC step entries (ent_steps_kernel)
    uint32_t nsub_total;                         // subsequences of the batch
    // device destuff (ntiles == 0: every frame of the batch was destuffed on the host)
    const uint8_t* raw;          // raw scan bytes, frame f at frames[f].data_off
    RawFrame* rawf;              // [nframes]
    const uint32_t* tile_frame;  // [ntiles] frame of each tile
    uint32_t* tiles;             // [3][ntiles] scratch: emitted bytes, markers, end (then offsets)
    uint32_t ntiles;
    // speculative sync (latency decoders; null otherwise): [sub][kMaxBpm] records
    struct SpecRec* spec;        // [sub][kMaxBpm]
    struct CandRec* cand;        // [sub][kSlots]
    uint8_t* cmap;               // [sub][kSlotRow]
    uint8_t* cslot;              // [sub] the verified chain's slot (ent_chain_lb_kernel / ent_chain_kernel)
    uint32_t spec_lead;          // lead-in of the spec runs (bits)
    uint32_t* chainfn;           // [frame][chain_chunks][kLbWords] look-back words of the chunks (ent_chain_lb_kernel)
    uint32_t* chain_broken;      // non-null: the look-back chain kernel runs (its words are allocated)
    uint32_t chain_chunks;       // chunks of the frame with the most subsequences (grid width)
    uint32_t chain_epoch;        // 1 .. 2^24 - 1, new per launch: tags the look-back words (cleared only when
                                 // the tag wraps back to 1: gdec_issue)
};


// `blocks`: the frame's block_info() records (fill_blocks), LDS on the device.
__host__ __device__ __forceinline__ RunCtx make_ctx(const EntBatchDev& b, const EntFrame& F, const HuffLut* tabs,
                                                    const BlockInfo* blocks, const uint8_t* steps = nullptr)
{
    RunCtx c;
    c.data = b.data + F.data_off;
    c.seg_end = b.seg_end + F.seg_base;
    c.tabs = tabs;
    c.blocks = blocks;
    c.nseg = F.nseg;
    c.data_bits = F.data_bits;
    c.bpm = F.bpm;
    c.seg_blocks = F.seg_blocks;
    c.steps = steps;
    c.layout = F.layout;
    c.geo = F.geo;
    c.mcu_w = F.mcu_w;
    return c;
}

// The frame's AC step tables (step_entry) from its LUTs: [table][1 << kStepBits].
__host__ __device__ __forceinline__ void fill_steps(uint8_t* steps, const HuffLut* tabs, int ntab, int tid,
                                                    int nthreads)
{
    for (int i = tid; i < (ntab << kStepBits); i += nthreads)
        steps[i] = step_entry(tabs[i >> kStepBits], static_cast<uint32_t>(i) & ((1u << kStepBits) - 1));
}

// Host side of the block records (the kernels fill their LDS copy per thread).
inline void fill_blocks(BlockInfo (&t)[kMaxBpm], const EntFrame& F)
{
    for (int j = 0; j < kMaxBpm; ++j) t[j] = block_info(F.jinfo[j]);
}

__host__ __device__ __forceinline__ uint64_t guess_entry(const RunCtx& c, uint32_t start)
{
    return pack_state(start, 0, 0, find_segment(c.seg_end, c.nseg, start));
}

__host__ __device__ __forceinline__ uint32_t frame_groups(uint32_t nsub) { return (nsub + kOwn - 1) / kOwn; }

// Subsequence handled by thread t of frame group gl (may be < 0 or >= nsub).
__host__ __device__ __forceinline__ int64_t group_sub(uint32_t gl, int t)
{
    return static_cast<int64_t>(gl) * kOwn - kWarm + t;
}

// Speculative sync (latency mode, DESIGN.md s10 "Single-image latency").
// The round-based sync guesses one entry per subsequence, (k*S, j = 0,
// z = 0): bits and z fall into step with the true decode within a few hundred
// bits, but the block-in-MCU index j only by chance, so a lone frame's chains
// take ~7 serial rounds of S-bit re-runs to verify (measured by the emulation:
// 4-10 rounds per group on an FHD q90 frame at S = 1024).  Here:
//   ent_spec_kernel   runs every subsequence k from all P = bpm guesses
//                     (k*S - W, j, 0), a lead-in of W bits before its start:
//                     the state at its middle (checkpoint), its exit and the
//                     second half's statistics.  One of the P guesses meets
//                     the true decode within 512 bits for 89 % of starts and
//                     within 1024 for 98 % (one guess: 25 % and 54 %;
//                     hjd_debug_entropy_syncstats with HJD_SYNC_PHASES);
//   ent_cand_kernel   runs k from each of its predecessor's P spec exits
//                     (subsequence 0: from the frame start), stopping at the
//                     middle when the run meets one of k's checkpoints; the
//                     exit's index among k's spec exits is k+1's entry slot
//                     (cmap).  An exit that is none of them opens an overflow
//                     slot of k+1 (two levels), so the maps are total on real
//                     data;
//   ent_chain_kernel  one workgroup per frame composes the slot maps (a scan
//                     over threads, each owning a range of subsequences) from
//                     the frame start: every subsequence's verified entry,
//                     statistics and mid-state follow without serial rounds,
//                     and the group records (agg, wentries, linked) the link,
//                     fallback and write kernels read.
// The chain is exact by construction (every record comes from a real run of
// its subsequence from the entry it names, starting at the frame start); a
// chain that leaves all slots (none seen) falls back to the sequential repair.
// The write kernel decodes a verified subsequence as four quarters, each from
// the state at its first unit boundary >= k*S + q*S/4 (q = 0: the entry):
// the runs below stop there on the way and keep those states.
__host__ __device__ __forceinline__ uint32_t quarter_stop(uint32_t k, uint32_t S, uint32_t q)
{
    return k * S + (q * S) / 4;
}
struct SpecRec {          // spec run of subsequence k from guess (k*S - W, j, 0)
    uint64_t cp;          // state at the first unit boundary >= k*S + S/2
    uint64_t x;           // exit
    SubStats s2;          // statistics cp -> x
    SubStats s3;          // statistics cp -> q3
    uint64_t q3, pad;     // state at the third quarter (as cp at the middle)
};
static_assert(sizeof(SpecRec) == 64, "SpecRec layout");
struct CandRec {          // subsequence k run from the entry of one of its slots
    SubStats s1, s;       // [0] [1] statistics entry -> mid and entry -> exit
    uint64_t e, mid;      // [2] entry, mid-state
    uint64_t y, q1;       // [3] exit, first-quarter state
    SubStats sq1;         // [4] statistics entry -> q1
    SubStats sq3;         // [5] statistics mid -> q3
    uint64_t q3, pad0;    // [6] third-quarter state
    uint64_t pad1, pad2;  // [7]
};
static_assert(sizeof(CandRec) == 128, "CandRec layout");
constexpr uint32_t kNoCand = 0xFF;                   // no slot
constexpr int kOvfLevels = 2;                        // overflow slots: P per level
constexpr int kSlots = (1 + kOvfLevels) * kMaxBpm;   // candidate and overflow slots per subsequence
constexpr int kRepairSlot = kSlots;                  // written by ent_chain_kernel's repair
constexpr int kChainSlots = kSlots + 1;
constexpr int kCandRow = kChainSlots;                // CandRec row stride
constexpr int kSlotRow = 20;                         // cmap row stride (bytes, >= kChainSlots)
static_assert(kSlotRow >= kChainSlots, "cmap row");

// The spec run of subsequence k from guess j, with a lead-in of `lead` bits.
__host__ __device__ __forceinline__ SpecRec spec_run(const RunCtx& c, uint32_t k, uint32_t j, uint32_t S, uint32_t lead)
{
    const uint32_t start = k * S > lead ? k * S - lead : 0u;
    const uint64_t g = guess_entry(c, start);
    SpecRec r;
    // one run through the middle (cp) and the third quarter (q3) to the exit
    const uint32_t mpos[2] = {quarter_stop(k, S, 2), quarter_stop(k, S, 3)};
    uint64_t ms[2];
    SubStats mst[2], s4 = stats_identity();
    r.x = run<false, 2>(c, pack_state(st_pos(g), j, 0, st_seg(g)), (k + 1) * S, s4, nullptr, mpos, ms, mst);
    r.cp = ms[0];
    r.q3 = ms[1];
    r.s3 = mst[1];
    r.s2 = stats_combine(r.s3, s4);
    r.pad = 0;
    return r;
}

// Subsequence k from entry e: to the middle; if that state is one of k's
// spec checkpoints, the rest is that spec run's, else decode on.  sk: k's P
// spec records.  Returns the index of the exit among k's spec exits, or kNoCand.
__host__ __device__ __forceinline__ uint32_t cand_run(const RunCtx& c, uint32_t k, uint64_t e, uint32_t S,
                                                      const SpecRec* sk, uint32_t P, CandRec& out)
{
    out.e = e;
    out.pad0 = out.pad1 = out.pad2 = 0;
    const uint32_t m1 = quarter_stop(k, S, 1), m3 = quarter_stop(k, S, 3);
    SubStats s12 = stats_identity();
    out.mid = run<false, 1>(c, e, quarter_stop(k, S, 2), s12, nullptr, &m1, &out.q1, &out.sq1);
    out.s1 = stats_combine(out.sq1, s12);
    uint32_t jm = kNoCand;
    for (uint32_t j = 0; j < P; ++j)
        if (jm == kNoCand && same_state(out.mid, sk[j].cp)) jm = j;
    if (jm != kNoCand) {
        out.y = sk[jm].x;
        out.q3 = sk[jm].q3;
        out.sq3 = sk[jm].s3;
        out.s = stats_combine(out.s1, sk[jm].s2);
    } else {
        SubStats s4 = stats_identity();
        out.y = run<false, 1>(c, out.mid, (k + 1) * S, s4, nullptr, &m3, &out.q3, &out.sq3);
        out.s = stats_combine(out.s1, stats_combine(out.sq3, s4));
    }
    uint32_t idx = kNoCand;
    for (uint32_t j = 0; j < P; ++j)
        if (idx == kNoCand && same_state(out.y, sk[j].x)) idx = j;
    return idx;
}

// Candidate c < P of subsequence k (entry: spec exit c of k-1, or the frame
// start), and its overflow continuation: while the exit is none of the
// successor's spec exits, the successor is run from it in overflow slot
// (level + 1) * P + c, up to kOvfLevels levels.  Each slot has exactly one writer.
__host__ __device__ __forceinline__ void cand_chain(const RunCtx& c, const EntBatchDev& b, const EntFrame& F,
                                                    uint32_t k, uint32_t cidx)
{
    const uint32_t P = F.bpm, S = b.sub_bits;
    uint64_t e = k == 0 ? guess_entry(c, 0)
                        : b.spec[(static_cast<uint64_t>(F.sub_base) + k - 1) * kMaxBpm + cidx].x;
    uint32_t slot = cidx;
    for (int level = 0;; ++level) {
        const uint64_t row = static_cast<uint64_t>(F.sub_base) + k;
        CandRec r;
        const uint32_t nx = cand_run(c, k, e, S, b.spec + row * kMaxBpm, P, r);
        b.cand[row * kCandRow + slot] = r;
        if (nx != kNoCand || level == kOvfLevels || k + 1 >= F.nsub) {
            b.cmap[row * kSlotRow + slot] = static_cast<uint8_t>(nx);
            return;
        }
        const uint32_t next = static_cast<uint32_t>(level + 1) * P + cidx;
        b.cmap[row * kSlotRow + slot] = static_cast<uint8_t>(next);
        e = r.y;
        slot = next;
        ++k;
    }
}

// The chain leaves every slot at subsequence brk (its predecessor, entered at
// slot sp, exits at a state none of brk's slots holds): run brk on from that
// exit in the repair slot, and its successors until the exit is a spec exit
// again, linking the predecessor's map to the repair slot.
__host__ __device__ __forceinline__ void chain_repair(const RunCtx& c, const EntBatchDev& b, const EntFrame& F,
                                                      uint32_t brk, uint32_t sp)
{
    uint8_t* cm = b.cmap + static_cast<uint64_t>(F.sub_base) * kSlotRow;
    uint64_t e = b.cand[(static_cast<uint64_t>(F.sub_base) + brk - 1) * kCandRow + sp].y;
    cm[static_cast<uint64_t>(brk - 1) * kSlotRow + sp] = static_cast<uint8_t>(kRepairSlot);
    for (uint32_t k = brk;; ++k) {
        const uint64_t row = static_cast<uint64_t>(F.sub_base) + k;
        CandRec r;
        const uint32_t nx = cand_run(c, k, e, b.sub_bits, b.spec + row * kMaxBpm, F.bpm, r);
        b.cand[row * kCandRow + kRepairSlot] = r;
        if (nx != kNoCand || k + 1 >= F.nsub) {
            cm[static_cast<uint64_t>(k) * kSlotRow + kRepairSlot] = static_cast<uint8_t>(nx);
            return;
        }
        cm[static_cast<uint64_t>(k) * kSlotRow + kRepairSlot] = static_cast<uint8_t>(kRepairSlot);
        e = r.y;
    }
}

// The verified chain's record of subsequence k: the speculative sync leaves it
// in the chain's slot of k (cslot), the round-based sync in the sync arrays.
// 16-B vector reads (a SubStats copy goes through scratch on the device).
__host__ __device__ __forceinline__ SubStats stats_of(const u32x4& v)
{
    SubStats r;
    memcpy(&r, &v, sizeof(r));
    return r;
}
__host__ __device__ __forceinline__ const u32x4* sub_rec(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    const uint64_t row = static_cast<uint64_t>(F.sub_base) + k;
    return reinterpret_cast<const u32x4*>(b.cand + row * kCandRow + b.cslot[row]);
}
__host__ __device__ __forceinline__ SubStats sub_stats(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    return b.spec ? stats_of(sub_rec(b, F, k)[1]) : b.stats[F.sub_base + k];
}
__host__ __device__ __forceinline__ SubStats sub_stats1(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    return b.spec ? stats_of(sub_rec(b, F, k)[0]) : b.stats1[F.sub_base + k];
}
__host__ __device__ __forceinline__ uint64_t sub_entry(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    if (!b.spec) return b.entries[F.sub_base + k];
    const u32x4 v = sub_rec(b, F, k)[2];
    return static_cast<uint64_t>(v.x) | static_cast<uint64_t>(v.y) << 32;
}
__host__ __device__ __forceinline__ uint64_t sub_mid(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    if (!b.spec) return b.mids[F.sub_base + k];
    const u32x4 v = sub_rec(b, F, k)[2];
    return static_cast<uint64_t>(v.z) | static_cast<uint64_t>(v.w) << 32;
}
// Speculative sync only: the quarter states and statistics (CandRec).
__host__ __device__ __forceinline__ uint64_t sub_q1(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    const u32x4 v = sub_rec(b, F, k)[3];
    return static_cast<uint64_t>(v.z) | static_cast<uint64_t>(v.w) << 32;
}
__host__ __device__ __forceinline__ uint64_t sub_q3(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    const u32x4 v = sub_rec(b, F, k)[6];
    return static_cast<uint64_t>(v.x) | static_cast<uint64_t>(v.y) << 32;
}
__host__ __device__ __forceinline__ SubStats sub_sq1(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    return stats_of(sub_rec(b, F, k)[4]);
}
__host__ __device__ __forceinline__ SubStats sub_sq3(const EntBatchDev& b, const EntFrame& F, uint32_t k)
{
    return stats_of(sub_rec(b, F, k)[5]);
}
// Piece p of the write kernel's split of subsequence k (pieces: 2 halves, or
// 4 quarters under the speculative sync): its entry state, its stop, and the
// statistics from k's entry to that state.
__host__ __device__ __forceinline__ uint32_t write_pieces(const EntBatchDev& b) { return b.spec ? 4u : 2u; }
__host__ __device__ __forceinline__ uint64_t piece_entry(const EntBatchDev& b, const EntFrame& F, uint32_t k,
                                                        uint32_t p, SubStats& pre)
{
    pre = stats_identity();
    if (p == 0) return sub_entry(b, F, k);
    if (!b.spec) {
        pre = sub_stats1(b, F, k);
        return sub_mid(b, F, k);
    }
    if (p == 1) {
        pre = sub_sq1(b, F, k);
        return sub_q1(b, F, k);
    }
    pre = sub_stats1(b, F, k);
    if (p == 2) return sub_mid(b, F, k);
    pre = stats_combine(pre, sub_sq3(b, F, k));
    return sub_q3(b, F, k);
}
__host__ __device__ __forceinline__ uint32_t piece_stop(const EntBatchDev& b, uint32_t k, uint32_t p)
{
    return quarter_stop(k, b.sub_bits, (p + 1) * (4 / write_pieces(b)));
}

// The look-back chain kernel's chunking (ent_chain_lb_kernel), which sizes its buffers.
constexpr int kChainThreads = 512;
constexpr int kChainRows = 2;                                  // rows per thread and chunk
constexpr int kChainChunk = kChainThreads * kChainRows;        // 1024 subsequences
constexpr int kLbWords = 8;   // look-back words per chunk (ent_chain_lb_kernel)

// Repair of unjoined group boundaries, in order, one lane per flagged frame:
// from the predecessor's last (verified) subsequence, re-decode forward until
// the true chain meets the recorded chain again, rewriting entries/statistics
// on the way; then recompute the aggregates of the groups touched.  Chains are
// deterministic, so once two agree at a boundary they agree from there on.
__host__ __device__ __forceinline__ void repair_frame(const EntBatchDev& b, uint32_t f, const HuffLut* tabs,
                                                     const BlockInfo* blocks)
{
    const EntFrame& F = b.frames[f];
    const RunCtx c = make_ctx(b, F, tabs, blocks);
    const uint32_t ng = frame_groups(F.nsub);
    uint32_t done = 0;          // subsequences < done are verified
    uint32_t g_lo = ng, g_hi = 0;
    for (uint32_t gl = 1; gl < ng; ++gl) {
        const uint32_t first = gl * kOwn;
        if (first < done || b.linked[F.wg_base + gl]) continue;
        uint32_t k = first - 1;
        uint64_t cur = b.entries[F.sub_base + k];
        for (;;) {
            SubStats st = stats_identity(), st2 = stats_identity();
            const uint64_t m = run<false>(c, cur, k * b.sub_bits + b.sub_bits / 2, st, nullptr);
            if (k >= first) {
                b.mids[F.sub_base + k] = m;
                b.stats1[F.sub_base + k] = st;
            }
            const uint64_t x = run<false>(c, m, (k + 1) * b.sub_bits, st2, nullptr);
            st = stats_combine(st, st2);
            if (k >= first) {
                b.entries[F.sub_base + k] = cur;
                b.stats[F.sub_base + k] = st;
                const uint32_t g = k / kOwn;
                g_lo = g < g_lo ? g : g_lo;
                g_hi = g > g_hi ? g : g_hi;
            }
            ++k;
            if (k >= F.nsub || same_state(x, b.entries[F.sub_base + k])) break;
            cur = x;
        }
        done = k;
    }
    for (uint32_t g = g_lo; g <= g_hi && g < ng; ++g) {
        SubStats a = stats_identity();
        const uint32_t end = (g + 1) * kOwn < F.nsub ? (g + 1) * kOwn : F.nsub;
        for (uint32_t i = g * kOwn; i < end; ++i) a = stats_combine(a, b.stats[F.sub_base + i]);
        b.agg[F.wg_base + g] = a;
    }
}
// Lead-in of the speculative sync's spec runs at a ladder step, in bits (the
// decoder's policy, hjd_gdec.hip; the emulation runs step 0).
uint32_t spec_lead_bits(uint32_t step);

// pull_kernel's argument: 16-B words of `src` copied to the same offsets of `dst`.
constexpr int kPullSegs = 4;
struct PullSegs {
    uint64_t off[kPullSegs];     // 16-B words
    uint64_t words[kPullSegs];
    uint32_t n;
    // The next segment: `bytes` at byte offset `off16` (a multiple of 16) of the staging.
    void add(size_t off16, size_t bytes)
    {
        off[n] = off16 / 16;
        words[n++] = (bytes + 15) / 16;
    }
};

#ifdef __HIPCC__
// The launches live with the kernels (hjd_entropy.hip).
//
// Entropy kernels on `s`; coefficients land in b.coefs.  tabs_h: the batch's
// staged Huffman tables; steps_tabs: the caller's copy of the tables b.steps_g
// was last derived from (updated here).
int launch_entropy(const EntBatchDev& b, const uint8_t* tabs_h, std::vector<uint8_t>& steps_tabs, hipStream_t s);

hipError_t launch_pull(const uint8_t* src, uint8_t* dst, const PullSegs& segs, hipStream_t s);
#endif

}  // namespace ent
}  // namespace hjd
