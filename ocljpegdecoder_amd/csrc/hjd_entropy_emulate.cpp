// hjd_entropy_emulate.cpp -- host emulation of the GPU entropy decoder
//  and the host-only debug hooks of include/hjd_host.h: the
// kernels' steps (hjd_entropy_batch.hpp, hjd_entropy.hpp) run in plain C++ on
// a batch staged by hjd_entropy_prep.cpp.  What the CPU tests and the fuzzer
// (tools/fuzz/run_entropy.sh) exercise; nothing here touches the GPU runtime.
#include <time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "hjd.h"
#include "hjd_entropy_prep.hpp"
#include "hjd_host.h"
#include "hjd_internal.h"

using hjd_internal::set_error;
using hjd_internal::tuning;
using namespace hjd::ent;

namespace {

// ---------------------------------------------------------------------------
// Host emulation of the four kernels (test hook; same state machine and the
// same group geometry, without the LDS window)
// ---------------------------------------------------------------------------
// Host emulation of ent_spec_kernel, ent_cand_kernel and ent_chain_kernel.
void emulate_spec_sync(const EntBatchDev& b)
{
    const uint32_t S = b.sub_bits;
    for (int pass = 0; pass < 2; ++pass) {   // 0: spec runs, 1: candidate chains
        for (uint32_t w = 0; w < b.nwg; ++w) {
            const EntFrame& F = b.frames[b.wg_frame[w]];
            const uint32_t gl = w - F.wg_base;
            if (gl >= frame_groups(F.nsub)) continue;
            BlockInfo blocks[kMaxBpm];
            fill_blocks(blocks, F);
            std::vector<uint8_t> steps(static_cast<size_t>(F.ntab) << kStepBits);
            fill_steps(steps.data(), b.tabs + F.tab_base, F.ntab, 0, 1);
            const RunCtx c = make_ctx(b, F, b.tabs + F.tab_base, blocks, steps.data());
            for (int t = kWarm; t < kGroupSubs; ++t) {
                const int64_t k = group_sub(gl, t);
                if (k >= static_cast<int64_t>(F.nsub)) break;
                for (uint32_t j = 0; j < F.bpm; ++j) {
                    if (pass == 0)
                        b.spec[(static_cast<uint64_t>(F.sub_base) + static_cast<uint64_t>(k)) * kMaxBpm + j] =
                            spec_run(c, static_cast<uint32_t>(k), j, S, b.spec_lead);
                    else
                        cand_chain(c, b, F, static_cast<uint32_t>(k), j);
                }
            }
        }
    }
    for (uint32_t f = 0; f < b.nframes; ++f) {   // the chain kernel's walk, in order, with its repairs
        const EntFrame& F = b.frames[f];
        const uint32_t n = F.nsub;
        BlockInfo blocks[kMaxBpm];
        fill_blocks(blocks, F);
        std::vector<uint8_t> steps(static_cast<size_t>(F.ntab) << kStepBits);
        fill_steps(steps.data(), b.tabs + F.tab_base, F.ntab, 0, 1);
        const RunCtx c = make_ctx(b, F, b.tabs + F.tab_base, blocks, steps.data());
        uint32_t slot = 0, prev = 0;
        int nrepair = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const uint64_t row = static_cast<uint64_t>(F.sub_base) + k;
            if (slot == kNoCand) {
                chain_repair(c, b, F, k, prev);
                slot = kRepairSlot;
                ++nrepair;
            }
            const CandRec& r = b.cand[row * kCandRow + slot];
            b.cslot[row] = static_cast<uint8_t>(slot);
            b.entries[row] = r.e;
            b.stats[row] = r.s;
            b.mids[row] = r.mid;
            b.stats1[row] = r.s1;
            prev = slot;
            slot = b.cmap[row * kSlotRow + slot];
        }
        if (nrepair) b.status[f] |= kStatusFallback;
        if (tuning().emu_rounds.get()) {
            int novf[kOvfLevels + 2] = {};
            for (uint32_t k = 0; k < n; ++k)
                for (uint32_t q = 0; q < F.bpm; ++q) {
                    const uint32_t v = b.cmap[(static_cast<uint64_t>(F.sub_base) + k) * kSlotRow + q];
                    novf[v == kNoCand ? kOvfLevels + 1 : v >= static_cast<uint32_t>(kSlots) ? 0 : v / F.bpm]++;
                }
            fprintf(stderr, "chain: nsub %u repairs %d; level-0 candidates -> spec %d, overflow %d, none %d\n", n,
                    nrepair, novf[0], novf[1], novf[kOvfLevels + 1]);
            int chain_lvl[kOvfLevels + 2] = {};   // the verified chain's slots by level (last: repair)
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t sl = b.cslot[F.sub_base + k];
                ++chain_lvl[sl >= static_cast<uint32_t>(kSlots) ? kOvfLevels + 1 : sl / F.bpm];
            }
            fprintf(stderr, "chain: slots by level %d / %d / %d, repair %d\n", chain_lvl[0], chain_lvl[1], chain_lvl[2],
                    chain_lvl[3]);
            // ent_cand_kernel's serial bits per thread (k, c) and per wave (64 lanes of one c)
            std::vector<uint32_t> cost, wmax;
            uint32_t nlev[kOvfLevels + 1] = {}, nmiss = 0;
            for (uint32_t g = 0; g < frame_groups(n); ++g)
                for (uint32_t c0 = 0; c0 < F.bpm; ++c0)
                    for (int wv = 0; wv < kGroupSubs / 64; ++wv) {
                        uint32_t wm = 0;
                        for (int l = 0; l < 64; ++l) {
                            const int t = wv * 64 + l;
                            const int64_t k0 = group_sub(g, t);
                            if (t < kWarm || k0 >= static_cast<int64_t>(n)) continue;
                            uint32_t kk = static_cast<uint32_t>(k0), slot = c0, bits = 0;
                            for (int level = 0;; ++level) {
                                const uint64_t row = static_cast<uint64_t>(F.sub_base) + kk;
                                const CandRec& r = b.cand[row * kCandRow + slot];
                                bits += st_pos(r.mid) - st_pos(r.e);
                                bool hit = false;
                                for (uint32_t j = 0; j < F.bpm; ++j) hit |= same_state(r.mid, b.spec[row * kMaxBpm + j].cp);
                                if (!hit) {
                                    bits += st_pos(r.y) - st_pos(r.mid);
                                    ++nmiss;
                                }
                                const uint32_t nx = b.cmap[row * kSlotRow + slot];
                                if (nx == kNoCand || nx < F.bpm || level == kOvfLevels || kk + 1 >= n) {
                                    ++nlev[level];
                                    break;
                                }
                                slot = nx;
                                ++kk;
                            }
                            cost.push_back(bits);
                            wm = std::max(wm, bits);
                        }
                        if (wm) wmax.push_back(wm);
                    }
            auto pct = [](std::vector<uint32_t> v, double q) {
                std::sort(v.begin(), v.end());
                return v.empty() ? 0u : v[static_cast<size_t>(q * (v.size() - 1))];
            };
            fprintf(stderr, "cand threads %zu: levels %u/%u/%u, mid misses %u; bits p50 %u p90 %u p99 %u max %u; "
                    "wave max p50 %u p90 %u max %u\n", cost.size(), nlev[0], nlev[1], nlev[2], nmiss, pct(cost, 0.5),
                    pct(cost, 0.9), pct(cost, 0.99), pct(cost, 1.0), pct(wmax, 0.5), pct(wmax, 0.9), pct(wmax, 1.0));
        }
        for (uint32_t g = 0; g < frame_groups(n); ++g) {
            const uint32_t w = F.wg_base + g;
            SubStats a = stats_identity();
            const uint32_t end = (g + 1) * kOwn < n ? (g + 1) * kOwn : n;
            for (uint32_t k = g * kOwn; k < end; ++k) a = stats_combine(a, b.stats[F.sub_base + k]);
            b.agg[w] = a;
            for (int t = 0; t < kWarm; ++t) {
                const int64_t k = group_sub(g, t);
                b.wentries[static_cast<uint64_t>(w) * kWarm + t] = k >= 0 ? b.entries[F.sub_base + k] : 0;
            }
            b.linked[w] = 1u;
        }
    }
}

void emulate(const EntBatchDev& b)
{
    const uint32_t S = b.sub_bits;
    // sync: per group, phase 1 then the rounds (or the speculative sync)
    if (b.spec) emulate_spec_sync(b);
    for (uint32_t w = 0; w < (b.spec ? 0u : b.nwg); ++w) {
        const EntFrame& F = b.frames[b.wg_frame[w]];
        BlockInfo blocks[kMaxBpm];
        fill_blocks(blocks, F);
        std::vector<uint8_t> steps(static_cast<size_t>(F.ntab) << kStepBits);
        fill_steps(steps.data(), b.tabs + F.tab_base, F.ntab, 0, 1);
        const RunCtx c = make_ctx(b, F, b.tabs + F.tab_base, blocks, steps.data());
        const uint32_t gl = w - F.wg_base;
        std::vector<uint64_t> used(kGroupSubs, 0), x(kGroupSubs, 0), xs0(kGroupSubs, 0), xs1(kGroupSubs, 0);
        std::vector<SubStats> st(kGroupSubs, stats_identity()), suf(kGroupSubs, stats_identity());
        std::vector<uint64_t> cp(kGroupSubs, 0);
        auto valid = [&](int t) { const int64_t k = group_sub(gl, t); return k >= 0 && k < int64_t(F.nsub); };
        auto record = [&](int t, uint64_t m, const SubStats& s1) {   // as the device: owned subsequences
            if (t < kWarm) return;
            const uint32_t k = static_cast<uint32_t>(group_sub(gl, t));
            b.mids[F.sub_base + k] = m;
            b.stats1[F.sub_base + k] = s1;
        };
        for (int t = 0; t < kGroupSubs; ++t) {   // phase 1, split at the checkpoint
            if (!valid(t)) continue;
            const uint32_t k = static_cast<uint32_t>(group_sub(gl, t));
            used[t] = guess_entry(c, k * S);
            cp[t] = run<false>(c, used[t], k * S + S / 2, st[t], nullptr);
            record(t, cp[t], st[t]);
            x[t] = run<false>(c, cp[t], (k + 1) * S, suf[t], nullptr);
            st[t] = stats_combine(st[t], suf[t]);
            xs0[t] = x[t];
        }
        std::vector<uint64_t>* cur = &xs0;
        std::vector<uint64_t>* nxt = &xs1;
        for (int round = 0;; ++round) {
            bool changed = false;
            for (int t = 0; t < kGroupSubs; ++t) {
                const int64_t k = group_sub(gl, t);
                if (valid(t) && t > 0 && k > 0 && !same_state((*cur)[t - 1], used[t])) {
                    const uint32_t ku = static_cast<uint32_t>(k);
                    SubStats s2 = stats_identity();
                    uint64_t x2;
                    if (round == 0) {   // round 0: to the checkpoint, on if phase 1 is not joined there
                        const uint64_t r = run<false>(c, (*cur)[t - 1], ku * S + S / 2, s2, nullptr);
                        record(t, r, s2);
                        if (same_state(r, cp[t])) {
                            x2 = x[t];
                            s2 = stats_combine(s2, suf[t]);
                        } else {
                            SubStats s3 = stats_identity();
                            x2 = run<false>(c, r, (ku + 1) * S, s3, nullptr);
                            s2 = stats_combine(s2, s3);
                        }
                    } else {
                        const uint64_t m2 = run<false>(c, (*cur)[t - 1], ku * S + S / 2, s2, nullptr);
                        record(t, m2, s2);
                        SubStats s3 = stats_identity();
                        x2 = run<false>(c, m2, (ku + 1) * S, s3, nullptr);
                        s2 = stats_combine(s2, s3);
                    }
                    changed |= !same_state(x2, x[t]);
                    used[t] = (*cur)[t - 1];
                    st[t] = s2;
                    x[t] = x2;
                }
                (*nxt)[t] = x[t];
            }
            std::swap(cur, nxt);
            if (!changed) {
                if (tuning().emu_rounds.get()) fprintf(stderr, "group %u: %d rounds\n", gl, round + 1);
                break;
            }
        }
        SubStats a = stats_identity();
        for (int t = 0; t < kGroupSubs; ++t) {
            const bool own = valid(t) && t >= kWarm;
            const uint32_t k = static_cast<uint32_t>(group_sub(gl, t));
            if (own) {
                b.entries[F.sub_base + k] = used[t];
                b.stats[F.sub_base + k] = st[t];
                a = stats_combine(a, st[t]);
            } else if (t < kWarm) {
                b.wentries[static_cast<uint64_t>(w) * kWarm + t] = used[t];
            }
        }
        b.agg[w] = a;
    }
    // link (the speculative sync's chain kernel writes the group records itself)
    for (uint32_t w = 0; w < (b.spec ? 0u : b.nwg); ++w) {
        const uint32_t f = b.wg_frame[w];
        const EntFrame& F = b.frames[f];
        const uint32_t gl = w - F.wg_base;
        bool joined = gl == 0;
        for (int t = 0; t < kWarm && !joined; ++t)
            joined = same_state(b.wentries[static_cast<uint64_t>(w) * kWarm + t],
                                b.entries[F.sub_base + static_cast<uint64_t>(group_sub(gl, t))]);
        b.linked[w] = joined ? 1u : 0u;
        if (!joined) b.status[f] |= kStatusFallback;
    }
    // repair
    for (uint32_t f = 0; f < b.nframes; ++f) {
        if (!(b.status[f] & kStatusFallback)) continue;
        BlockInfo blocks[kMaxBpm];
        fill_blocks(blocks, b.frames[f]);
        repair_frame(b, f, b.tabs + b.frames[f].tab_base, blocks);
    }
    // write (group order = subsequence order)
    alignas(16) int16_t stage[kStageStride];
    for (uint32_t f = 0; f < b.nframes; ++f) {
        const EntFrame& F = b.frames[f];
        BlockInfo blocks[kMaxBpm];
        fill_blocks(blocks, F);
        const RunCtx c = make_ctx(b, F, b.tabs + F.tab_base, blocks);
        SubStats pre = stats_identity();
        for (uint32_t i = 0; i < F.nsub; ++i) {
            for (uint32_t piece = 0; piece < write_pieces(b); ++piece) {   // as ent_write_kernel
                SubStats lead;
                const uint64_t entry = piece_entry(b, F, i, piece, lead);
                const SubStats p = stats_combine(pre, lead);
                RunOut o;
                o.coefs = b.coefs + F.coef_off * 64;
                o.stage = stage;
                o.blk = p.nblk;
                o.nblocks = F.nblocks;
                o.nout = F.nout;
                o.pred[0] = p.dc[0];
                o.pred[1] = p.dc[1];
                o.pred[2] = p.dc[2];
                SubStats s = stats_identity();
                run<true>(c, entry, piece_stop(b, i, piece), s, &o);
                if (s.flags & kError) b.status[f] |= kStatusCorrupt;
                if (piece + 1 == write_pieces(b) && i == F.nsub - 1 && p.nblk + s.nblk != F.nblocks)
                    b.status[f] |= kStatusCount;
            }
            pre = stats_combine(pre, sub_stats(b, F, i));
        }
    }
}

}  // namespace

extern "C" {

// Tuning hook: for every subsequence start k*S (k >= 1), decode from the guess
// (k*S, 0, 0) and report after how many bits past k*S its state first equals
// the true decode's state at the same unit boundary (hist[min(bits/64, nbins-1)];
// never-synced within max_bits go to the last bin).
int hjd_debug_entropy_syncstats(const uint8_t* data, size_t size, int sub_bits, int max_bits, int64_t* hist, int nbins)
{
    if (!data || !hist || nbins < 2 || sub_bits < 32) return set_error(HJD_E_INVALID, "invalid arguments");
    std::vector<uint8_t> buf(size + 64);
    Prepared p;
    int rc = prepare(data, size, buf.data(), size + 32, p);
    if (rc) return rc;
    EntFrame F;
    memset(&F, 0, sizeof(F));
    F.data_bits = p.data_bits;
    F.nseg = static_cast<uint32_t>(p.seg_end.size());
    F.bpm = static_cast<uint8_t>(p.bpm);
    memcpy(F.jinfo, p.jinfo, sizeof(F.jinfo));
    EntBatchDev b;
    memset(&b, 0, sizeof(b));
    b.data = buf.data();
    b.seg_end = p.seg_end.data();
    BlockInfo blocks[kMaxBpm];
    fill_blocks(blocks, F);
    const RunCtx c = make_ctx(b, F, p.tabs, blocks);
    // true states at every unit boundary: decode one unit at a time (stop = pos + 1)
    std::vector<uint16_t> truth(p.data_bits + 1, 0xFFFF);
    uint64_t cur = pack_state(0, 0, 0, 0);
    while (st_seg(cur) < F.nseg) {
        truth[st_pos(cur)] = static_cast<uint16_t>(st_j(cur) << 8 | st_z(cur));
        SubStats st = stats_identity();
        const uint64_t nx = run<false>(c, cur, st_pos(cur) + 1, st, nullptr);
        if (st_pos(nx) <= st_pos(cur) && st_seg(nx) == st_seg(cur)) break;
        cur = nx;
    }
    for (int i = 0; i < nbins; ++i) hist[i] = 0;
    const uint32_t S = static_cast<uint32_t>(sub_bits);
    // HJD_SYNC_PHASES=n: guesses (k*S, j, 0) for j < n; the first of them to
    // meet the true decode counts (speculation over block-in-MCU positions)
    const auto& ph = tuning().sync_phases;
    const uint32_t nph = std::max(1, std::min(ph.is_set() ? static_cast<int>(ph.get()) : 1, static_cast<int>(F.bpm)));
    // HJD_SYNC_OFFSETS=m: also guesses m-1 bit positions before k*S (offsets
    // 7, 19, 37, 61, ... bits), each with the n phases
    const auto& os = tuning().sync_offsets;
    const uint32_t noff = std::max(1, os.is_set() ? static_cast<int>(os.get()) : 1);
    static const uint32_t kOffs[] = {0, 7, 19, 37, 61, 91, 127, 169, 217, 271, 331, 397};
    for (uint32_t k = 1; static_cast<uint64_t>(k) * S < p.data_bits; ++k) {
        int bin = nbins - 1;
        for (uint32_t oi = 0; oi < std::min<uint32_t>(noff, 12); ++oi) {
            if (kOffs[oi] > k * S) continue;
            for (uint32_t j0 = 0; j0 < nph; ++j0) {
                uint64_t g = guess_entry(c, k * S - kOffs[oi]);
                g = pack_state(st_pos(g), j0, 0, st_seg(g));
                while (st_pos(g) < static_cast<uint64_t>(k) * S + static_cast<uint32_t>(max_bits) && st_seg(g) < F.nseg) {
                    const uint32_t q = st_pos(g);
                    if (truth[q] == (st_j(g) << 8 | st_z(g))) {
                        bin = std::min<int>(bin, q > k * S ? static_cast<int>((q - k * S) / 64) : 0);
                        break;
                    }
                    SubStats st = stats_identity();
                    g = run<false>(c, g, q + 1, st, nullptr);
                }
            }
        }
        hist[bin]++;
    }
    return HJD_OK;
}

// Test hook for the sync-mode step decode: every run a sync kernel makes uses
// the AC step tables (several units per lookup) and must give exactly the
// state and statistics of the unit-by-unit decode.  Runs the first scan from
// guessed entries (k*S - o, j, 0) for every block-in-MCU j and a few offsets o,
// and from true unit boundaries, to stops S bits on, both ways; counts runs
// and mismatches (exit state, block count, flags or DC sums).
int hjd_debug_entropy_sync_check(const uint8_t* data, size_t size, int sub_bits, int64_t* runs, int64_t* mismatches)
{
    if (!data || !runs || !mismatches || sub_bits < 16) return set_error(HJD_E_INVALID, "invalid arguments");
    std::vector<uint8_t> buf(size + 256);
    Prepared p;
    int rc = prepare(data, size, buf.data(), size + 64, p);
    if (rc) return rc;
    EntFrame F;
    memset(&F, 0, sizeof(F));
    F.data_bits = p.data_bits;
    F.nseg = static_cast<uint32_t>(p.seg_end.size());
    F.bpm = static_cast<uint8_t>(p.bpm);
    F.ntab = static_cast<uint8_t>(p.ntab);
    memcpy(F.jinfo, p.jinfo, sizeof(F.jinfo));
    EntBatchDev b;
    memset(&b, 0, sizeof(b));
    b.data = buf.data();
    b.seg_end = p.seg_end.data();
    BlockInfo blocks[kMaxBpm];
    fill_blocks(blocks, F);
    std::vector<uint8_t> steps(static_cast<size_t>(F.ntab) << kStepBits);
    fill_steps(steps.data(), p.tabs, F.ntab, 0, 1);
    const RunCtx cs = make_ctx(b, F, p.tabs, blocks, steps.data());
    const RunCtx cu = make_ctx(b, F, p.tabs, blocks);
    const uint32_t S = static_cast<uint32_t>(sub_bits);
    int64_t n = 0, bad = 0;
    auto check = [&](uint64_t entry, uint32_t stop) {
        SubStats a = stats_identity(), u = stats_identity();
        const uint64_t xa = run<false>(cs, entry, stop, a, nullptr);
        const uint64_t xu = run<false>(cu, entry, stop, u, nullptr);
        ++n;
        if (xa != xu || a.nblk != u.nblk || a.flags != u.flags || a.dc[0] != u.dc[0] || a.dc[1] != u.dc[1] ||
            a.dc[2] != u.dc[2])
            ++bad;
    };
    static const uint32_t kOffs[] = {0, 5, 19, 61, 200};
    for (uint32_t k = 0; static_cast<uint64_t>(k) * S < p.data_bits; ++k)
        for (uint32_t o : kOffs) {
            if (o > k * S) continue;
            const uint64_t g = guess_entry(cu, k * S - o);
            for (uint32_t j = 0; j < F.bpm; ++j) check(pack_state(st_pos(g), j, 0, st_seg(g)), k * S + S);
        }
    // true unit boundaries, sampled
    uint64_t cur = pack_state(0, 0, 0, 0);
    for (uint32_t i = 0; st_seg(cur) < F.nseg; ++i) {
        if (i % 7 == 0) check(cur, st_pos(cur) + S / 2 + (i % 5) * 37);
        SubStats st = stats_identity();
        const uint64_t nx = run<false>(cu, cur, st_pos(cur) + 1, st, nullptr);
        if (st_pos(nx) <= st_pos(cur) && st_seg(nx) == st_seg(cur)) break;
        cur = nx;
    }
    *runs = n;
    *mismatches = bad;
    return HJD_OK;
}

// Test hook for the destuff step alone: the host routine (destuff()) on one
// raw scan (the device kernels: hjd_debug_destuff_gpu), so arbitrary byte
// strings (stuffing, fill bytes, RSTn in and out of order, truncation) can be
// compared directly.
int hjd_debug_destuff_host(const uint8_t* scan, size_t n, uint8_t* out, size_t cap, uint32_t* seg_end, int max_seg,
                           int* nseg, int64_t* out_bytes)
{
    if (!scan || !out || !seg_end || !nseg || !out_bytes) return set_error(HJD_E_INVALID, "NULL argument");
    std::vector<uint32_t> seg;
    size_t len = 0;
    const int rc = destuff(scan, scan + n, out, cap, seg, len);
    if (rc) return rc;
    *nseg = static_cast<int>(seg.size());
    for (int i = 0; i < static_cast<int>(seg.size()) && i < max_seg; ++i) seg_end[i] = seg[i];
    *out_bytes = static_cast<int64_t>(len);
    return HJD_OK;
}

// Test hook for the upload plan alone (Staging::plan_uploads): the frames come
// as numbers, nothing is staged.  frames[i][8]: destuff mode, data_off,
// data_bits, raw_len, raw_off, raw_src (an address, only compared), and a
// further scan's data_off and data_bits (data_bits < 0: none).
int hjd_debug_upload_plan(const int64_t* frames, int n, int64_t data_base, int64_t hdr_used, int latency,
                          int64_t prepulled, int64_t* rows, int cap_rows, int* nrows, int64_t* segs, int* nsegs,
                          int* pull, int64_t totals[2])
{
    if (!frames || n <= 0 || !rows || !nrows || !segs || !nsegs || !pull || !totals)
        return set_error(HJD_E_INVALID, "invalid upload-plan arguments");
    Staging st;
    st.caps.data = static_cast<size_t>(data_base);
    st.H.used = static_cast<size_t>(hdr_used);
    st.frames.resize(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        const int64_t* f = frames + 8 * i;
        Prepared& p = st.frames[i];
        p.destuff = static_cast<int>(f[0]);
        p.data_off = static_cast<size_t>(f[1]);
        p.data_bits = static_cast<uint32_t>(f[2]);
        p.raw_len = static_cast<uint32_t>(f[3]);
        p.raw_off = static_cast<uint64_t>(f[4]);
        p.raw_src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(f[5]));
        if (f[7] < 0) continue;
        p.more.resize(1);
        p.more[0].data_off = static_cast<size_t>(f[6]);
        p.more[0].data_bits = static_cast<uint32_t>(f[7]);
    }
    UploadPlan plan;
    st.plan_uploads(latency != 0, static_cast<size_t>(prepulled), plan);
    if (plan.copies.size() > static_cast<size_t>(cap_rows)) return set_error(HJD_E_INVALID, "more rows than cap_rows");
    *nrows = static_cast<int>(plan.copies.size());
    for (const UploadCopy& u : plan.copies) {
        const int64_t row[6] = {u.kind, static_cast<int64_t>(u.dst_off), static_cast<int64_t>(u.src),
                                static_cast<int64_t>(u.bytes), u.first, u.last};
        memcpy(rows, row, sizeof(row));
        rows += 6;
    }
    *pull = plan.pull;
    *nsegs = static_cast<int>(plan.segs.n);
    for (uint32_t k = 0; k < plan.segs.n; ++k) {
        segs[2 * k] = static_cast<int64_t>(plan.segs.off[k]);
        segs[2 * k + 1] = static_cast<int64_t>(plan.segs.words[k]);
    }
    totals[0] = plan.moved;
    totals[1] = plan.host_bytes;
    return HJD_OK;
}

// The decoder's steps on the host, one JPEG: staged as a batch of one
// (Staging, in calloc'd memory), then emulate() over work arrays of its own.
int hjd_debug_entropy_emulate(const uint8_t* data, size_t size, int sub_bits, int16_t* coefs,
                              int64_t capacity_blocks, int32_t* status)
{
    if (!data || !coefs) return set_error(HJD_E_INVALID, "NULL argument");
    if (sub_bits == 0) sub_bits = kDefaultSubBits;
    if (sub_bits < 32 || sub_bits > (1 << 20)) return set_error(HJD_E_INVALID, "sub_bits out of range [32, 2^20]");
    Staging st;
    st.caps = make_caps(1, static_cast<int64_t>(size), std::max<int64_t>(capacity_blocks, 1), sub_bits);
    const auto& se = tuning().sync_spec;   // the emulation takes the round-based sync unless asked
    const bool spec = se.is_set() && se.get() != 0;
    st.h_stage = static_cast<uint8_t*>(calloc(1, st.bytes()));
    if (!st.h_stage) return set_error(HJD_E_NOMEM, "staging allocation");
    struct Free {
        Staging* st;
        ~Free() { free(st->h_stage); st->h_stage = nullptr; }
    } guard{&st};
    const uint8_t* datas[1] = {data};
    const size_t sizes[1] = {size};
    int rc = st.stage_frames(datas, sizes, 1);
    if (rc) return rc;
    if (st.frames[0].out_blocks > capacity_blocks)
        return set_error(HJD_E_INVALID, "capacity %lld < %lld blocks", static_cast<long long>(capacity_blocks),
                         static_cast<long long>(st.frames[0].out_blocks));
    EntBatchDev b;
    rc = st.assemble(st.h_stage, coefs, nullptr, static_cast<uint32_t>(st.caps.sub_bits), 0, 0, b);
    if (rc) return rc;
    const int64_t total = st.frames[0].out_blocks;
    const size_t nsub = static_cast<size_t>(st.caps.max_subs), nwg = static_cast<size_t>(st.caps.max_wgs);
    std::vector<uint64_t> entries(nsub, 0), mids(nsub, 0), wentries(nwg * kWarm, 0);
    std::vector<SubStats> stats(nsub, stats_identity()), stats1(nsub, stats_identity()), agg(nwg, stats_identity());
    std::vector<uint32_t> linked(nwg, 0), bstatus(b.nframes, 0);
    std::vector<SpecRec> specs;
    std::vector<CandRec> cands;
    std::vector<uint8_t> cmap, cslot;
    if (spec) {
        specs.assign(nsub * kMaxBpm, SpecRec());
        cands.assign(nsub * kCandRow, CandRec());
        cmap.assign(nsub * kSlotRow, static_cast<uint8_t>(kNoCand));
        cslot.assign(nsub + 16, 0);
        b.spec = specs.data();
        b.cand = cands.data();
        b.cmap = cmap.data();
        b.cslot = cslot.data();
        b.spec_lead = spec_lead_bits(0);
    }
    b.entries = entries.data();
    b.stats = stats.data();
    b.mids = mids.data();
    b.stats1 = stats1.data();
    b.wentries = wentries.data();
    b.linked = linked.data();
    b.agg = agg.data();
    b.status = bstatus.data();
    memset(coefs, 0, static_cast<size_t>(total) * 128);
    emulate(b);
    for (uint32_t e = 1; e < b.nframes; ++e) bstatus[0] |= bstatus[e];   // the JPEG's further scans
    if (status) *status = static_cast<int32_t>(bstatus[0]);
    if (bstatus[0] & ~kStatusFallback) return set_error(HJD_E_INVALID, "corrupt entropy data (status %u)", bstatus[0]);
    return HJD_OK;
}

// Host-side stream preparation alone, no GPU (bench.py --host-prep-only: the
// host ceiling of the multi-GPU config-5 stream).  One call =
// one per-GPU worker pool: nthreads threads bound to NUMA node `node` (-1:
// unbound) prepare `frames` JPEGs.  The sources are an arena of `arena_bytes`
// (the pool's files replicated back to back, first-touched on that node, read
// in order) and each frame lands in the next slot of a staging ring of
// `ring_bytes`: with both larger than the node's L3 the traffic is DRAM's, as
// for a loader streaming fresh files.
//   mode 0: the host-destuff path (header, tables, destuff into staging);
//   mode 1: the GPU-destuff path (header and tables only);
//   mode 2: a plain memcpy of each file into staging (the DRAM reference).
// out[0] wall ns, out[1] summed thread CPU ns, out[2] JPEG bytes, out[3] frames.
int hjd_debug_host_prep(const uint8_t* const* datas, const size_t* sizes, int n, int mode, int nthreads, int node,
                        int64_t frames, int64_t arena_bytes, int64_t ring_bytes, int32_t* barrier, int parties,
                        int64_t out[4])
{
    if (!datas || !sizes || n <= 0 || nthreads <= 0 || frames <= 0 || !out || mode < 0 || mode > 2)
        return set_error(HJD_E_INVALID, "invalid host-prep arguments");
    const hjd_internal::CpuSet cpus = hjd_internal::node_cpus(node);
    size_t maxsz = 0, total = 0;
    for (int i = 0; i < n; ++i) {
        maxsz = std::max(maxsz, sizes[i]);
        total += sizes[i];
    }
    const size_t reps = std::max<size_t>(1, static_cast<size_t>(arena_bytes) / std::max<size_t>(total, 1));
    const size_t slot = align_up(maxsz + 4 * kDataPad, 4096);
    const size_t nslot = std::max<size_t>(static_cast<size_t>(nthreads),
                                          static_cast<size_t>(ring_bytes) / slot);
    std::vector<const uint8_t*> src;
    std::vector<size_t> src_size;
    uint8_t* arena = nullptr;
    uint8_t* ring = nullptr;
    {   // arena and ring first-touched by a thread on the pool's node
        std::thread t([&] {
            hjd_internal::bind_current_thread(cpus);
            arena = static_cast<uint8_t*>(malloc(total * reps));
            ring = static_cast<uint8_t*>(malloc(slot * nslot));
            if (!arena || !ring) return;
            size_t pos = 0;
            for (size_t r = 0; r < reps; ++r)
                for (int i = 0; i < n; ++i) {
                    memcpy(arena + pos, datas[i], sizes[i]);
                    src.push_back(arena + pos);
                    src_size.push_back(sizes[i]);
                    pos += sizes[i];
                }
            memset(ring, 0, slot * nslot);
        });
        t.join();
    }
    if (!arena || !ring) {
        free(arena);
        free(ring);
        return set_error(HJD_E_NOMEM, "host-prep arena");
    }
    if (barrier && parties > 1) {   // concurrent pools start their timed phase together
        __atomic_add_fetch(barrier, 1, __ATOMIC_SEQ_CST);
        while (__atomic_load_n(barrier, __ATOMIC_SEQ_CST) < parties) std::this_thread::yield();
    }
    std::atomic<int64_t> next{0}, cpu_ns{0}, bytes{0};
    std::atomic<int> err{HJD_OK};
    auto worker = [&] {
        hjd_internal::bind_current_thread(cpus);
        timespec c0, c1;
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &c0);
        int64_t my_bytes = 0;
        Prepared pf;
        for (;;) {
            const int64_t k = next.fetch_add(1);
            if (k >= frames) break;
            const size_t i = static_cast<size_t>(k) % src.size();
            uint8_t* dst = ring + slot * (static_cast<size_t>(k) % nslot);
            int rc = HJD_OK;
            if (mode == 2) memcpy(dst, src[i], src_size[i]);
            else rc = prepare(src[i], src_size[i], dst, slot - kDataPad, pf,
                              mode == 0 ? kDestuffHost : kDestuffFromCaller, 0);
            if (rc) err = rc;
            my_bytes += static_cast<int64_t>(src_size[i]);
        }
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &c1);
        cpu_ns += (c1.tv_sec - c0.tv_sec) * 1000000000ll + (c1.tv_nsec - c0.tv_nsec);
        bytes += my_bytes;
    };
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) th.emplace_back(worker);
    for (auto& t : th) t.join();
    out[0] = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    out[1] = cpu_ns;
    out[2] = bytes;
    out[3] = frames;
    free(arena);
    free(ring);
    return err == HJD_OK ? HJD_OK : set_error(err, "host prep failed: %s", hjd_last_error());
}

}  // extern "C"
