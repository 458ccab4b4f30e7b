// hjd_entropy_prep.cpp -- host preparation of a GPU entropy batch (DESIGN.md
// s10), at memcpy speed per JPEG: parse the header, build the device Huffman
// tables, copy the entropy-coded segment into the staging memory while
// removing byte stuffing (FF00 -> FF) and RST markers, recording where each
// restart interval ends; then lay out the batch header the kernels read.
#include "hjd_entropy_prep.hpp"

#include <cstring>

#include "hjd.h"

using hjd_internal::set_error;

namespace hjd {
namespace ent {

// Canonical Huffman code (T.81 C.2 / F.2.2.3) -> first-level LUT of unit
// entries + MAXCODE.  dc: the table's class (T.81 B.2.4.2 Tc = 0).
static int build_lut(HuffLut& t, const uint8_t counts[16], const uint8_t* syms, int nsym, bool dc)
{
    memset(&t, 0, sizeof(t));
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int n = counts[len - 1];
        const int first = code;
        for (int i = 0; i < n; ++i, ++k, ++code) {
            if (k >= nsym || code >= (1 << len)) return -1;
            t.vals[k] = syms[k];
            if (len <= kLutBits) {
                const int shift = kLutBits - len;
                for (int r = 0; r < (1 << shift); ++r)
                    t.lut[(code << shift) | r] = static_cast<uint16_t>(unit_entry(len, syms[k], dc));
            }
        }
        t.maxcode[len] = n ? code - 1 : -1;
        t.delta[len] = (k - n) - first;   // valptr - mincode
        code <<= 1;
    }
    t.maxcode[0] = -1;
    return 0;
}

int destuff(const uint8_t* p, const uint8_t* end, uint8_t* out, size_t cap, std::vector<uint32_t>& seg_end,
            size_t& out_len, DestuffHook* hook)
{
    uint8_t* q = out;
    uint8_t* const qend = out + cap;
    int nrst = 0;
    seg_end.clear();
    while (p < end) {
        p = hjd_internal::copy_until_ff(p, end, q, qend);
        if (hook && static_cast<size_t>(q - out) >= hook->next) hook->fire(hook, static_cast<size_t>(q - out));
        if (p == end) break;
        if (*p != 0xFF) return set_error(HJD_E_INVALID, "scan larger than the staging capacity");
        if (p + 1 >= end) break;                       // truncated at FF
        const uint8_t b = p[1];
        if (b == 0x00) {                               // stuffed FF
            if (q >= qend) return set_error(HJD_E_INVALID, "scan larger than the staging capacity");
            *q++ = 0xFF;
            p += 2;
        } else if (b == 0xFF) {                        // fill byte before a marker
            p += 1;
        } else if (b >= 0xD0 && b <= 0xD7) {           // RSTn (src/decoder.cpp:288-307)
            if (b != 0xD0 + (nrst & 7))
                return set_error(HJD_E_INVALID, "expected RST%d, found RST%d", nrst & 7, b - 0xD0);
            seg_end.push_back(static_cast<uint32_t>((q - out) * 8));
            ++nrst;
            p += 2;
        } else {
            break;                                     // EOI (or another marker): end of scan
        }
    }
    seg_end.push_back(static_cast<uint32_t>((q - out) * 8));
    out_len = static_cast<size_t>(q - out);
    return HJD_OK;
}

// The scan-level fields of q from its header: geometry, and the tables the
// scan references, deduplicated into slots.
static int scan_fields(const hjd_internal::ScanHeader& h, Prepared& q)
{
    q.bpm = h.bpm;
    q.nblocks = h.scan_blocks;
    q.restart_mcus = h.restart_interval;
    q.layout = h.layout ? kLayoutRaster : kLayoutMcu;
    q.geo = geo_make(static_cast<uint32_t>(h.out_bpm), static_cast<uint32_t>(h.comp_lh),
                     static_cast<uint32_t>(h.comp_lv), static_cast<uint32_t>(h.comp_bw));
    q.mcu_w = static_cast<uint32_t>(h.mcu_w);
    int slot_of[2][4];
    for (auto& a : slot_of)
        for (int& v : a) v = -1;
    q.ntab = 0;
    for (int j = 0; j < h.bpm; ++j) {
        const int ids[2] = {h.jdc[j], h.jac[j]};
        int slot[2];
        for (int cls = 0; cls < 2; ++cls) {
            int& s = slot_of[cls][ids[cls]];
            if (s < 0) {
                if (q.ntab >= kMaxTables) return set_error(HJD_E_INVALID, "too many Huffman tables");
                s = q.ntab++;
                if (build_lut(q.tabs[s], h.counts[cls][ids[cls]], h.symbols[cls][ids[cls]], h.nsym[cls][ids[cls]],
                              cls == 0))
                    return set_error(HJD_E_INVALID, "invalid Huffman table");
            }
            slot[cls] = s;
        }
        q.jinfo[j] = static_cast<uint16_t>(jinfo_make(slot[0], slot[1], h.jcomp[j], h.jslot[j]));
    }
    return HJD_OK;
}

// Restart intervals a scan must hold: DRI counts the scan's MCUs, which are
// single blocks in a non-interleaved scan.
static inline int64_t scan_segments(const hjd_internal::ScanHeader& h)
{
    const int64_t units = h.layout ? h.scan_blocks : static_cast<int64_t>(h.mcu_w) * h.mcu_h;
    return h.restart_interval > 0 ? (units + h.restart_interval - 1) / h.restart_interval : 1;
}

// Host destuff of one scan into dst (cap bytes, the pad included).
static int destuff_scan(const hjd_internal::ScanHeader& h, const uint8_t* data, size_t size, uint8_t* dst,
                        size_t cap, Prepared& q, DestuffHook* hook = nullptr)
{
    if (h.scan_offset > size) return set_error(HJD_E_INVALID, "scan offset past the end of the file");
    if (cap <= kDataPad) return set_error(HJD_E_INVALID, "scan bytes exceed the batch capacity");
    size_t len = 0;
    q.raw_len = static_cast<uint32_t>(std::min<size_t>(size - h.scan_offset, 0xFFFFFFFFu));   // bytes the host reads
    // a large scan: the first ~60 % of the output goes to the GPU while the host destuffs the rest
    if (hook) hook->next = size - h.scan_offset >= (256u << 10) ? (size - h.scan_offset) * 3 / 5 : SIZE_MAX;
    int rc = destuff(data + h.scan_offset, data + size, dst, cap - kDataPad, q.seg_end, len, hook);
    if (rc) return rc;
    if (len == 0) return set_error(HJD_E_INVALID, "empty scan");
    if (len >= (1u << 28)) return set_error(HJD_E_INVALID, "scan too large for one frame (>= 256 MiB)");
    const int64_t want = scan_segments(h);
    if (static_cast<int64_t>(q.seg_end.size()) != want)
        return set_error(HJD_E_INVALID, "%zu restart intervals in the scan, %lld expected", q.seg_end.size(),
                         static_cast<long long>(want));
    if (h.nblocks >= (1ll << 31)) return set_error(HJD_E_INVALID, "frame too large");
    memset(dst + len, 0xFF, kDataPad);
    q.data_bits = static_cast<uint32_t>(len * 8);
    return HJD_OK;
}

// A sequential file with several scans: every scan destuffed on the host, one
// after the other from dst (cap bytes); quantisation tables as of each
// component's scan.
static int prepare_multiscan(const uint8_t* data, size_t size, uint8_t* dst, size_t cap, Prepared& pf)
{
    std::vector<hjd_internal::ScanHeader> hs;
    int rc = hjd_internal::parse_scan_headers(data, size, &hs);
    if (rc) return rc;
    if (hs.empty() || hs.size() > static_cast<size_t>(kMaxScans)) return set_error(HJD_E_INVALID, "bad scan count");
    pf.more.resize(hs.size() - 1);
    size_t off = 0;
    for (size_t k = 0; k < hs.size(); ++k) {
        Prepared& q = k == 0 ? pf : pf.more[k - 1];
        rc = scan_fields(hs[k], q);
        if (rc) return rc;
        if (off >= cap) return set_error(HJD_E_INVALID, "scan bytes exceed the batch capacity");
        q.data_off = pf.data_off + off;
        rc = destuff_scan(hs[k], data, size, dst + off, cap - off, q);
        if (rc) return rc;
        for (int j = 0; j < hs[k].bpm; ++j) {
            const int c = hs[k].jcomp[j];
            memcpy(pf.qt[c], hs[k].qt[c], sizeof(pf.qt[c]));
        }
        off = align_up(off + q.data_bits / 8 + kDataPad, 16);
    }
    return HJD_OK;
}

int prepare(const uint8_t* data, size_t size, uint8_t* dst, size_t cap, Prepared& pf, int mode, uint64_t raw_off,
            DestuffHook* hook)
{
    hjd_internal::ScanHeader h;
    int rc = hjd_internal::parse_scan_header(data, size, &h);
    if (rc) return rc;
    pf.width = h.width;
    pf.height = h.height;
    pf.sampling = h.sampling;
    pf.out_blocks = h.nblocks;
    memcpy(pf.qt, h.qt, sizeof(pf.qt));
    if (h.extra_scans > 0) {   // several scans: plan_raw keeps them on the host destuff path
        if (mode != kDestuffHost) return set_error(HJD_E_INVALID, "multi-scan JPEG: host destuff only");
        return prepare_multiscan(data, size, dst, cap + kDataPad, pf);
    }
    rc = scan_fields(h, pf);
    if (rc) return rc;
    if (h.scan_offset > size) return set_error(HJD_E_INVALID, "scan offset past the end of the file");
    if (mode != kDestuffHost) {
        // the header is all the host reads; the GPU finds stuffing, markers and the scan's end
        const size_t raw = size - h.scan_offset;
        if (raw == 0) return set_error(HJD_E_INVALID, "empty scan");
        if (raw >= (1u << 28)) return set_error(HJD_E_INVALID, "scan too large for one frame (>= 256 MiB)");
        if (raw > cap) return set_error(HJD_E_INVALID, "scan larger than the staging capacity");
        if (h.nblocks >= (1ll << 31)) return set_error(HJD_E_INVALID, "frame too large");
        const int64_t nmcu = static_cast<int64_t>(h.mcu_w) * h.mcu_h;
        const int64_t want = h.restart_interval > 0 ? (nmcu + h.restart_interval - 1) / h.restart_interval : 1;
        if (want > raw / 2 + 1) return set_error(HJD_E_INVALID, "%lld restart intervals cannot fit %zu scan bytes",
                                                 static_cast<long long>(want), raw);
        pf.seg_end.assign(static_cast<size_t>(want), 0u);   // filled on the device
        pf.destuff = mode;
        pf.raw_len = static_cast<uint32_t>(raw);
        pf.raw_src = data + h.scan_offset;
        pf.raw_off = raw_off;
        if (mode == kDestuffFromStaging) memcpy(dst, pf.raw_src, raw);
        pf.data_bits = static_cast<uint32_t>(raw * 8);      // upper bound (groups are laid out for it)
        return HJD_OK;
    }
    return destuff_scan(h, data, size, dst, cap + kDataPad, pf, hook);
}

// ---------------------------------------------------------------------------
// Staging of a batch
// ---------------------------------------------------------------------------
int Staging::prepare_frame(int i, const uint8_t* data, size_t size, size_t data_off, size_t cap, int mode,
                           uint64_t raw_off, DestuffHook* hook)
{
    Prepared& p = frames[static_cast<size_t>(i)];
    p = Prepared();
    p.data_off = data_off;
    if (!data) return p.rc = set_error(HJD_E_INVALID, "frame %d: NULL data", i);
    if (cap <= kDataPad) return p.rc = set_error(HJD_E_INVALID, "scan bytes exceed the batch capacity");
    int rc = prepare(data, size, data_area() + data_off, cap - kDataPad, p, mode, raw_off, hook);
    if (rc) return p.rc = rc;
    return HJD_OK;
}

int Staging::stage_frames(const uint8_t* const* datas, const size_t* sizes, int n, PlanFn plan, DestuffHook* hook)
{
    if (n <= 0 || n > caps.max_frames) return set_error(HJD_E_INVALID, "batch of %d frames (capacity %d)", n,
                                                        caps.max_frames);
    frames.assign(static_cast<size_t>(n), Prepared());
    data_used = 0;
    int64_t blocks = 0;
    RawCursor cur;
    // what the frames after i need at least in the data area, whichever path
    // they take: a frame with a device-destuffed scan is placed only if the
    // rest still fit, so a batch sized by its file bytes never fails on
    // placement.  A single-scan file needs its entropy-coded bytes plus pad
    // (destuffed or raw), a multi-scan file data_need() of its size; so a
    // batch sized by its scan bytes (hjd_gdec_create) keeps the device destuff
    // for its pinned files wherever their raw scans fit.
    std::vector<uint64_t> tail(static_cast<size_t>(n) + 1, 0);
    for (int i = n - 1; i >= 0; --i) {
        hjd_internal::ScanHeader h;
        const bool one_scan = datas[i] && hjd_internal::parse_scan_header(datas[i], sizes[i], &h) == HJD_OK &&
                              h.extra_scans == 0 && h.scan_offset <= sizes[i];
        tail[i] = tail[i + 1] + (one_scan ? align_up(sizes[i] - h.scan_offset + kDataPad, 16) : data_need(sizes[i]));
    }
    for (int i = 0; i < n; ++i) {
        if (data_used >= data_cap()) return set_error(HJD_E_INVALID, "scan bytes exceed the batch capacity");
        int mode = kDestuffHost;
        uint64_t raw_off = 0;
        bool fits = true;
        int rc = plan ? plan(*this, datas[i], sizes[i], cur, mode, raw_off, fits, data_cap() - data_used, tail[i + 1])
                      : HJD_OK;
        if (rc) return set_error(rc, "frame %d: %s", i, hjd_last_error());
        if (!fits) return set_error(HJD_E_INVALID, "scan bytes exceed the batch capacity");
        rc = prepare_frame(i, datas[i], sizes[i], data_used, data_cap() - data_used, mode, raw_off,
                           i == 0 ? hook : nullptr);
        if (rc) return set_error(rc, "frame %d: %s", i, hjd_last_error());
        data_used = align_up(frames[i].data_end(), 16);
        blocks += frames[i].out_blocks;
    }
    if (blocks > caps.max_blocks)
        return set_error(HJD_E_INVALID, "batch needs %lld blocks (capacity %lld)", static_cast<long long>(blocks),
                         static_cast<long long>(caps.max_blocks));
    return HJD_OK;
}

int Staging::assemble(uint8_t* blob, int16_t* coefs, int64_t* block_offsets, uint32_t S, size_t recs_bytes,
                      size_t qt_bytes, EntBatchDev& d)
{
    const int n = static_cast<int>(frames.size());
    // entropy frames: the n JPEGs' (first) scans, then the further scans of
    // multi-scan files (scan_file: their JPEG), all writing the JPEG's blocks
    std::vector<const Prepared*> ents;
    std::vector<int> ent_file;
    scan_file.clear();
    for (int i = 0; i < n; ++i) {
        ents.push_back(&frames[i]);
        ent_file.push_back(i);
    }
    for (int i = 0; i < n; ++i)
        for (const Prepared& q : frames[i].more) {
            ents.push_back(&q);
            ent_file.push_back(i);
            scan_file.push_back(i);
        }
    const int ne = static_cast<int>(ents.size());
    std::vector<uint64_t> file_coef(static_cast<size_t>(n), 0);
    uint64_t coef_off = 0;
    for (int i = 0; i < n; ++i) {
        file_coef[i] = coef_off;
        coef_off += static_cast<uint64_t>(frames[i].out_blocks);
    }
    size_t ntab = 0, nseg = 0, nwg = 0;
    for (const Prepared* p : ents) {
        ntab += static_cast<size_t>(p->ntab);
        nseg += p->seg_end.size();
        const uint32_t ns = (p->data_bits + S - 1) / S;
        nwg += frame_groups(ns);
    }
    HdrOffsets& o = H;
    o.frames = 0;
    o.tabs = align_up(sizeof(EntFrame) * ne, kAlign);
    o.seg = align_up(o.tabs + sizeof(HuffLut) * ntab, kAlign);
    o.wg = align_up(o.seg + 4 * nseg, kAlign);
    o.recs = align_up(o.wg + 4 * nwg, kAlign);
    o.qt = align_up(o.recs + recs_bytes, kAlign);
    size_t ntiles = 0;
    for (const Prepared& p : frames)
        if (p.destuff != kDestuffHost)
            ntiles += (raw_region_len(static_cast<uint32_t>(p.raw_off & 15), p.raw_len) + kTileBytes - 1) / kTileBytes;
    o.rawf = align_up(o.qt + qt_bytes, kAlign);
    o.tilef = align_up(o.rawf + (ntiles ? sizeof(RawFrame) * ne : 0), kAlign);
    // per entropy frame status words, zero in the header's upload (no memset)
    o.status = align_up(o.tilef + 4 * ntiles, kAlign);
    o.used = align_up(o.status + 4 * (2 * static_cast<size_t>(ne) + 1), kAlign);
    if (o.used > caps.hdr_cap || ntiles > static_cast<size_t>(caps.max_tiles))
        return set_error(HJD_E_INVALID, "batch header exceeds its capacity");

    EntFrame* ef = reinterpret_cast<EntFrame*>(h_stage + o.frames);
    memset(h_stage + o.status, 0, 4 * (2 * static_cast<size_t>(ne) + 1));
    HuffLut* tb = reinterpret_cast<HuffLut*>(h_stage + o.tabs);
    uint32_t* seg = reinterpret_cast<uint32_t*>(h_stage + o.seg);
    uint32_t* wgf = reinterpret_cast<uint32_t*>(h_stage + o.wg);
    uint32_t sub_base = 0, wg_base = 0, seg_base = 0, tab_base = 0;
    for (int e = 0; e < ne; ++e) {
        const Prepared& p = *ents[e];
        const Prepared& file = frames[ent_file[e]];
        EntFrame F;
        memset(&F, 0, sizeof(F));
        F.data_off = p.data_off;
        F.coef_off = file_coef[ent_file[e]];
        F.data_bits = p.data_bits;
        F.nsub = (p.data_bits + S - 1) / S;
        F.sub_base = sub_base;
        F.wg_base = wg_base;
        F.seg_base = seg_base;
        F.nseg = static_cast<uint32_t>(p.seg_end.size());
        F.nblocks = static_cast<uint32_t>(p.nblocks);
        F.tab_base = tab_base;
        F.ntab = static_cast<uint8_t>(p.ntab);
        F.bpm = static_cast<uint8_t>(p.bpm);
        F.sampling = static_cast<uint8_t>(file.sampling);
        F.layout = static_cast<uint8_t>(p.layout);
        memcpy(F.jinfo, p.jinfo, sizeof(F.jinfo));
        F.seg_blocks = F.nseg > 1 ? static_cast<uint32_t>(p.restart_mcus * p.bpm) : 0u;
        F.geo = p.geo;
        F.mcu_w = p.mcu_w;
        F.nout = static_cast<uint32_t>(file.out_blocks);
        ef[e] = F;
        memcpy(tb + tab_base, p.tabs, sizeof(HuffLut) * p.ntab);
        memcpy(seg + seg_base, p.seg_end.data(), 4 * p.seg_end.size());
        const uint32_t nw = frame_groups(F.nsub);
        for (uint32_t g = 0; g < nw; ++g) wgf[wg_base + g] = static_cast<uint32_t>(e);
        sub_base += F.nsub;
        wg_base += nw;
        seg_base += F.nseg;
        tab_base += p.ntab;
    }
    if (block_offsets)
        for (int i = 0; i < n; ++i) block_offsets[i] = static_cast<int64_t>(file_coef[i]);
    if (coef_off > static_cast<uint64_t>(caps.max_blocks) || sub_base > caps.max_subs || wg_base > caps.max_wgs)
        return set_error(HJD_E_INVALID, "batch exceeds the decoder's capacity");

    d.ntiles = static_cast<uint32_t>(ntiles);
    uint32_t max_nsub = 0;
    for (int e = 0; e < ne; ++e) max_nsub = ef[e].nsub > max_nsub ? ef[e].nsub : max_nsub;
    d.chain_chunks = (max_nsub + kChainChunk - 1) / kChainChunk;
    if (d.chain_chunks == 0) d.chain_chunks = 1;
    d.chainfn = nullptr;
    d.chain_broken = nullptr;
    d.chain_epoch = 0;
    d.agg2 = nullptr;
    d.host_status = nullptr;
    d.spec = nullptr;
    d.cand = nullptr;
    d.cmap = nullptr;
    d.cslot = nullptr;
    d.spec_lead = 0;
    d.nsub_total = sub_base;
    d.rawf = nullptr;
    d.tile_frame = nullptr;
    if (ntiles) {
        RawFrame* rf = reinterpret_cast<RawFrame*>(h_stage + o.rawf);
        uint32_t* tf = reinterpret_cast<uint32_t*>(h_stage + o.tilef);
        uint32_t tbase = 0;
        for (int e = 0; e < ne; ++e) {   // further scans are host-destuffed (ntiles 0)
            const Prepared& p = *ents[e];
            RawFrame r{p.raw_off, p.raw_len, static_cast<uint32_t>(p.raw_off & 15), tbase, 0, 0, 0};
            if (p.destuff != kDestuffHost) {
                r.ntiles = (raw_region_len(r.begin, p.raw_len) + kTileBytes - 1) / kTileBytes;
                for (uint32_t k = 0; k < r.ntiles; ++k) tf[tbase + k] = static_cast<uint32_t>(e);
                tbase += r.ntiles;
            }
            rf[e] = r;
        }
        d.rawf = reinterpret_cast<RawFrame*>(blob + o.rawf);
        d.tile_frame = reinterpret_cast<const uint32_t*>(blob + o.tilef);
    }
    d.frames = reinterpret_cast<const EntFrame*>(blob + o.frames);
    d.tabs = reinterpret_cast<const HuffLut*>(blob + o.tabs);
    d.seg_end = reinterpret_cast<const uint32_t*>(blob + o.seg);
    d.wg_frame = reinterpret_cast<const uint32_t*>(blob + o.wg);
    d.data = blob + caps.data;
    d.coefs = coefs;
    d.nframes = static_cast<uint32_t>(ne);
    d.nwg = wg_base;
    d.sub_bits = S;
    d.ntab_max = 1;
    for (const Prepared* p : ents) d.ntab_max = std::max<uint32_t>(d.ntab_max, static_cast<uint32_t>(p->ntab));
    d.ntab_total = tab_base;
    d.steps_g = nullptr;
    return HJD_OK;
}

void Staging::plan_uploads(bool latency, size_t prepulled, UploadPlan& out) const
{
    const int n = static_cast<int>(frames.size());
    out.copies.clear();
    out.segs = PullSegs{};
    out.moved = static_cast<int64_t>(H.used);
    out.host_bytes = 0;
    out.pull = latency;
    for (const Prepared& p : frames) {
        out.pull = out.pull && p.destuff == kDestuffHost;
        if (p.destuff == kDestuffFromStaging) out.host_bytes += 2 * static_cast<int64_t>(p.raw_len);
        if (p.destuff != kDestuffHost) continue;
        out.host_bytes += static_cast<int64_t>(p.raw_len) + p.data_bits / 8;
        for (const Prepared& q : p.more) out.host_bytes += q.data_bits / 8;
    }
    if (out.pull) out.segs.add(0, H.used);
    else out.copies.push_back({kUploadHeader, 0, 0, H.used, 0, 0});
    // In batch order: a run of consecutive host-destuffed frames (all their scans) moves in one
    // copy to the data area, a raw scan in the staging in one to the raw area.
    for (int i = 0, j; i < n; i = j) {
        const Prepared& p = frames[i];
        j = i + 1;
        if (p.destuff == kDestuffFromStaging) {
            out.copies.push_back({kUploadRawStaged, p.raw_off, caps.data + p.data_off, p.raw_len, i, j});
            out.moved += p.raw_len;
        } else if (p.destuff == kDestuffHost) {
            while (j < n && frames[j].destuff == kDestuffHost) ++j;
            const size_t off = caps.data + p.data_off, len = frames[j - 1].data_end() - p.data_off;
            // Pulled: every frame is host-destuffed, so this run is the whole batch, i is 0 (frame 0
            // starts the data area, where an early pull began) and segs holds two of its kPullSegs.
            if (out.pull) out.segs.add(off + prepulled, len - prepulled);
            else out.copies.push_back({kUploadData, off, off, len, i, j});
            out.moved += static_cast<int64_t>(len);
        }
    }
    // Last, raw scans in the caller's pinned memory, straight from there to the raw area: a run
    // of scans placed at their distance in the caller's memory (RawCursor) moves in one DMA.
    for (int i = 0, j; i < n; i = j) {
        const Prepared& p = frames[i];
        j = i + 1;
        if (p.destuff != kDestuffFromCaller) continue;
        size_t span = p.raw_len;
        while (j < n && frames[j].destuff == kDestuffFromCaller && frames[j].raw_src > p.raw_src &&
               frames[j].raw_off - p.raw_off == static_cast<uint64_t>(frames[j].raw_src - p.raw_src)) {
            span = static_cast<size_t>(frames[j].raw_src - p.raw_src) + frames[j].raw_len;
            ++j;
        }
        out.copies.push_back({kUploadRawCaller, p.raw_off, reinterpret_cast<uintptr_t>(p.raw_src), span, i, j});
        out.moved += static_cast<int64_t>(span);
    }
}

}  // namespace ent
}  // namespace hjd
