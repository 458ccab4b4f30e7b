// hjd_entropy_prep.hpp -- host preparation of a GPU entropy batch
// (hjd_entropy_prep.cpp): one JPEG to tables + destuffed scan (Prepared), and
// the staging of a batch of them under the layout of hjd_entropy_batch.hpp,
// with the plan of its uploads.  Plain C++: nothing here touches the GPU runtime.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hjd_entropy_batch.hpp"

namespace hjd {
namespace ent {

// A host destuff that hands finished output to the GPU while it runs (a
// latency decoder's lone image): fire(h, done) once `done` >= next output
// bytes are final; fire sets the next threshold.
struct DestuffHook {
    size_t next;
    void (*fire)(DestuffHook* h, size_t done);
    void* ctx;
};

// Copy an entropy-coded segment without byte stuffing and RST markers.  Ends
// at the first marker that is not RSTn (normally EOI) or at the end of the
// buffer.  seg_end receives the destuffed BIT offset where each restart
// interval ends (the last one = total length).
int destuff(const uint8_t* p, const uint8_t* end, uint8_t* out, size_t cap, std::vector<uint32_t>& seg_end,
            size_t& out_len, DestuffHook* hook = nullptr);

// Host-side result of preparing one JPEG: its (first) scan, which is the
// whole image for the reference's single interleaved scan, plus `more` for
// the further scans of a sequential file with several (an extension; each
// becomes an entropy frame of its own writing into the same coefficients).
struct Prepared {
    int rc = HJD_OK;
    int width = 0, height = 0, sampling = 0, bpm = 0;
    int64_t nblocks = 0;       // blocks this scan codes
    int64_t out_blocks = 0;    // blocks of the image
    uint32_t layout = kLayoutMcu, geo = 0, mcu_w = 0;   // EntFrame fields (block_dest)
    std::vector<Prepared> more;
    uint32_t data_bits = 0;
    size_t data_off = 0;       // in the batch data area
    int ntab = 0;
    int restart_mcus = 0;      // DRI (0: none)
    HuffLut tabs[kMaxTables];
    uint16_t jinfo[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> seg_end;
    int32_t qt[3][64];         // zigzag
    void* d_out = nullptr;
    int32_t pitch = 0;
    // device destuff: the raw scan goes to the device (data_bits is then the
    // raw upper bound until destuff_scan_kernel writes the real length)
    int destuff = 0;           // kDestuffHost / kDestuffFromCaller / kDestuffFromStaging
    const uint8_t* raw_src = nullptr;   // caller's pinned bytes (kDestuffFromCaller)
    uint32_t raw_len = 0;
    uint64_t raw_off = 0;      // raw-area offset of the first scan byte (RawCursor::place)

    // end of the data area this file uses (all scans, with their pads)
    size_t data_end() const
    {
        size_t e = data_off + data_bits / 8 + kDataPad;
        for (const Prepared& q : more) e = std::max(e, q.data_off + q.data_bits / 8 + kDataPad);
        return e;
    }
};

// Data-area bytes a JPEG of `size` bytes may need: its destuffed scans are
// shorter than the file, but each scan is padded and aligned.
inline size_t data_need(size_t size) { return align_up(size + kDataPad, 16) + (kMaxScans - 1) * (kDataPad + 16); }

// Places raw scans in a batch's raw area.  A caller-pinned scan that follows
// the previous one in the caller's memory within kMirrorGap bytes (a JPEG
// header, typically) is placed at the same distance, so the run moves with one
// DMA; anything else goes after the area in use, at the source's alignment mod 16.
//
// Capacity contract: a batch whose files total F bytes fits a raw area of
// F + kSlack bytes per frame, whatever lies between the files.  Mirroring
// consumes the gap between two scans (the next file's header, plus whatever
// the caller left between the files), so it is taken only while the area in
// use stays within the bytes of the files placed so far plus kSlack each
// (`allow`); otherwise, or when the mirrored offset would not fit, the scan
// is placed compactly (<= 30 bytes of alignment) and starts a new DMA run.
// By induction the area in use never exceeds F + 48 bytes per frame, and the
// 32-byte read-ahead fits in the kDataPad + 16 bytes data_cap() adds per frame.
struct RawCursor {
    static constexpr uint64_t kMirrorGap = 64 * 1024;
    static constexpr uint64_t kSlack = 48;
    static constexpr uint64_t kReadAhead = 32;   // destuff kernels' 16-B loads straddling the end
    const uint8_t* last_src = nullptr;
    uint64_t last_off = 0;
    uint64_t end = 0;
    uint64_t allow = 0;      // sum of (file bytes + kSlack) over the frames placed
    // n = scan bytes at src; file = bytes of the whole file; reserve = area
    // that must stay free after this scan (for frames still to come).
    bool place(const uint8_t* src, size_t n, size_t file, bool mirror, size_t cap, uint64_t& off,
               uint64_t reserve = 0)
    {
        const uint64_t allow_next = allow + file + kSlack;
        uint64_t o = ~0ull;
        if (mirror && last_src && src > last_src && last_off + static_cast<uint64_t>(src - last_src) >= end &&
            last_off + static_cast<uint64_t>(src - last_src) - end <= kMirrorGap) {
            o = last_off + static_cast<uint64_t>(src - last_src);
            if (o + n > allow_next || o + n + kReadAhead + reserve > cap) o = ~0ull;
        }
        if (o == ~0ull) {
            o = (end + 15) / 16 * 16 + (reinterpret_cast<uintptr_t>(src) & 15);
            if (o + n + kReadAhead + reserve > cap) return false;
        }
        off = o;
        end = o + n;
        allow = allow_next;
        last_src = mirror ? src : nullptr;
        last_off = o;
        return true;
    }
};

// Parse one JPEG and prepare its scans at dst (cap bytes, plus kDataPad after
// them): destuffed there (kDestuffHost; `hook` as destuff()), or for the
// device modes only described, with the raw scan copied there
// (kDestuffFromStaging) or left with the caller (kDestuffFromCaller) and
// placed at raw_off of the raw area.
int prepare(const uint8_t* data, size_t size, uint8_t* dst, size_t cap, Prepared& pf, int mode = kDestuffHost,
            uint64_t raw_off = 0, DestuffHook* hook = nullptr);

struct Staging;
// Destuff mode of a JPEG and, for the device modes, its place in the raw
// area.  fits = false when the raw scan does not fit the raw area, or
// data_room (free bytes of the data area) minus `reserve` (bytes kept for
// the frames still to come).
typedef int (*PlanFn)(const Staging& st, const uint8_t* data, size_t size, RawCursor& cur, int& mode,
                      uint64_t& raw_off, bool& fits, size_t data_room, uint64_t reserve);

// The uploads of a staged batch as data (Staging::plan_uploads), in the order
// they are issued.  Staging and device blob share their layout, so a header or
// data copy has one offset for both sides.
enum UploadKind {
    kUploadHeader,      // staging [0, bytes) -> blob
    kUploadData,        // a run of host-destuffed frames: staging [dst_off, + bytes) -> blob, same offset
    kUploadRawStaged,   // a raw scan in the staging's data area at `src` -> raw area at dst_off
    kUploadRawCaller,   // raw scans in the caller's pinned memory at address `src` -> raw area at dst_off
};
struct UploadCopy {
    int kind;
    uint64_t dst_off, src;
    size_t bytes;
    int first, last;    // the frames [first, last) it covers (the header: none)
};
struct UploadPlan {
    std::vector<UploadCopy> copies;
    bool pull;          // pull_kernel moves `segs` (header, then the one data run) and there are no copies
    PullSegs segs;
    int64_t moved;      // bytes host -> device, counted as ever: a data run in full though part of it was
                        // pulled early, a caller span with the gaps between its scans
    int64_t host_bytes; // scan bytes the host CPU read + wrote (a caller-pinned scan: none)
};

// The host side of one batch: the frames prepared into the owner's staging
// memory (caps.data + data_cap() bytes: header, then the data area), and the
// entropy header that describes them.
struct Staging {
    Caps caps{};
    HdrOffsets H{};
    uint8_t* h_stage = nullptr;         // the owner's: header + data
    std::vector<Prepared> frames;
    size_t data_used = 0;
    std::vector<int> scan_file;         // file of each entropy frame past the first n (a file's further scans)

    uint8_t* data_area() { return h_stage + caps.data; }
    // data_need() of every frame: the scan bytes, plus pad and alignment per scan
    size_t data_cap() const { return static_cast<size_t>(caps.max_scan_bytes) +
                                     (kDataPad + 16) * kMaxScans * static_cast<size_t>(caps.max_frames); }
    size_t bytes() const { return caps.data + data_cap(); }

    // Stage n JPEGs on the calling thread.  plan: each frame's destuff mode
    // (none: all on the host); hook: frame 0's host destuff (DestuffHook).
    int stage_frames(const uint8_t* const* datas, const size_t* sizes, int n, PlanFn plan = nullptr,
                     DestuffHook* hook = nullptr);
    // Parse + destuff one JPEG into frames[i] / the data area at data_off
    // (thread-safe for distinct i and disjoint data ranges).
    int prepare_frame(int i, const uint8_t* data, size_t size, size_t data_off, size_t cap, int mode,
                      uint64_t raw_off, DestuffHook* hook = nullptr);
    // Lays out and fills the entropy header for the staged frames at
    // subsequence length S, leaving recs_bytes at H.recs and qt_bytes at H.qt
    // for the owner (the pixel kernel's tables); returns the device view
    // (pointers into `blob`, the work arrays left null).
    int assemble(uint8_t* blob, int16_t* coefs, int64_t* block_offsets, uint32_t S, size_t recs_bytes,
                 size_t qt_bytes, EntBatchDev& d);
    // What moves the assembled batch (H.used header bytes, the frames' scans) to the device, and how.
    // latency: the owner is a latency decoder, whose all-host-destuffed batches are pulled;
    // prepulled: data-area bytes of frame 0 an early pull has moved already.  `out` keeps its storage.
    void plan_uploads(bool latency, size_t prepulled, UploadPlan& out) const;
};

}  // namespace ent
}  // namespace hjd
