"""GPU: one Huffman decoder (hjd_gdec) fed different work call after call.

A decoder is built once and called thousands of times, and it carries state
from launch to launch: the look-back words of ent_chain_lb_kernel and their
24-bit tag, device buffers and caches that are never cleared (d_linked, d_agg,
d_agg2, d_cslot, d_cand, d_cmap, d_chain_broken, the step tables' cache,
batch_sub_bits, batch_spec) and the lead-in ladder.  Each is right
only if every launch rewrites what it later reads, whatever the launch before
it was.  Here consecutive calls differ in every way the decoder distinguishes,
and the carried state is read back through GpuDecoder.debug_state().

Everywhere: coefficients equal hjd.decode_coefs(data) exactly (the host decoder
pinned to the reference's mcu_data, tests/test_jpeg_host.py), pixels equal the
oracle's of those coefficients, outputs are prefilled (0x5A5A / -1) before
every call, and the status words equal, unmasked, those of a fresh decoder
(the control) created with the same arguments and given the same files at the
lead-in the reused decoder reports for the call (its ladder may have moved;
the control's has not, so HJD_SPEC_LEAD holds the control at that lead-in)."""
import contextlib
import functools

import numpy as np
import pytest

import jpeg_writer as JW
import oracle_py as O
from test_entropy_emulation import _pil

pytestmark = pytest.mark.gpu

kChainChunk = 1024               # subsequences per look-back chunk (kChainChunk, hjd_entropy_batch.hpp)
kLeadLadder = (512, 1536, 2560)  # kLeadLadder, hjd_gdec.hip
kLeadBatches = 32                # kLeadBatches, hjd_gdec.hip
kEpochMax = 0xFFFFFF             # the tag's last value before it wraps to 1 (gdec_issue, hjd_gdec.hip)


@pytest.fixture
def tuning(hjd):
    """tuning(name, value): hjd.debug_tuning for the rest of the test."""
    with contextlib.ExitStack() as stack:
        yield lambda name, value: stack.enter_context(hjd.debug_tuning(name, value))


@functools.lru_cache(maxsize=None)
def _ref(data):
    """(host decoder's coefficients, info) of a file, computed once."""
    import ocljpegdecoder_amd as hjd
    coefs, info = hjd.decode_coefs(data)
    coefs.setflags(write=False)
    return coefs, info


@functools.lru_cache(maxsize=None)
def _ref_pixels(data):
    coefs, info = _ref(data)
    px = O.decode_q16(coefs, info.qt, info.width, info.height, info.sampling)
    px.setflags(write=False)
    return px


def _scan_bytes(data):
    """Entropy-coded bytes of a single-scan file as the decoder sees them:
    restart markers and byte stuffing removed."""
    s = data[_ref(data)[1].scan_offset:data.rindex(b"\xff\xd9")]
    for k in range(8):
        s = s.replace(bytes([0xFF, 0xD0 + k]), b"")
    return len(s.replace(b"\xff\x00", b"\xff"))


def _chunks(data, sub_bits):
    """Look-back chunks of a single-scan frame at S = sub_bits, worked out on
    the CPU (scan bits / S / 1024), well away from a chunk boundary so that the
    count cannot hinge on a few bytes of padding."""
    chunk_bytes = kChainChunk * sub_bits // 8
    n = _scan_bytes(data)
    assert 64 <= n % chunk_bytes <= chunk_bytes - 64, (n, chunk_bytes)
    return -(-n // chunk_bytes)


class _Reused:
    """A decoder kept for a whole test, and fresh controls with its arguments."""

    def __init__(self, hjd, ctx, max_frames, sub_bits, batches):
        self.hjd, self.ctx = hjd, ctx
        self.args = (max_frames, max(sum(len(d) for d in b) for b in batches),
                     max(sum(hjd.parse(d).nblocks for d in b) for b in batches), sub_bits)   # (headers only)
        self.gd = hjd.GpuDecoder(ctx, *self.args)
        self._controls = {}
        self.bits = []   # every call's status words

    def close(self):
        self.gd.close()

    def control(self, datas, lead):
        """Status words of a fresh decoder for the same files (lead: the
        lead-in of the call it controls, 0 for a round-based one)."""
        import torch
        key = (tuple(datas), lead)
        if key not in self._controls:
            total = sum(_ref(d)[1].nblocks for d in datas)
            coefs = torch.full((total, 64), 0x5A5A, dtype=torch.int16, device="cuda")
            with self.hjd.debug_tuning("HJD_SPEC_LEAD", lead or None):
                with self.hjd.GpuDecoder(self.ctx, *self.args) as fresh:
                    fresh.decode_coefs(list(datas), coefs)
                    self._controls[key] = fresh.sync()
        return self._controls[key]

    def _finish(self, datas, what):
        status = self.gd.sync()
        self.bits.append(status)
        st = self.gd.debug_state()
        assert status == self.control(datas, st["batch_lead_bits"]), (what, status, st)
        return st

    def coefs(self, datas, what="", compare=True):
        """decode_coefs + sync: exact coefficients, the control's status; returns the state."""
        import torch
        total = sum(_ref(d)[1].nblocks for d in datas)
        out = torch.full((total, 64), 0x5A5A, dtype=torch.int16, device="cuda")
        offs = self.gd.decode_coefs(list(datas), out)
        st = self._finish(datas, what)
        if compare:
            host = out.cpu().numpy()
            for i, (d, o) in enumerate(zip(datas, offs)):
                ref, info = _ref(d)
                np.testing.assert_array_equal(host[o:o + info.nblocks], ref, err_msg=f"{what} file {i}")
        return st

    def pixels(self, datas, what=""):
        """decode to BGRX + sync: the oracle's pixels, the control's status; returns the state."""
        import torch
        infos = [_ref(d)[1] for d in datas]
        outs = [torch.full((i.height, i.width), -1, dtype=torch.int32, device="cuda") for i in infos]
        self.gd.decode(list(datas), outs)
        st = self._finish(datas, what)
        for i, (d, o) in enumerate(zip(datas, outs)):
            np.testing.assert_array_equal(o.cpu().numpy().view(np.uint32), _ref_pixels(d), err_msg=f"{what} file {i}")
        return st


def _rows(counts):
    """Word positions (in chunks) of a batch's look-back rows: frame f's chunk c
    lies at f * chain_chunks + c, chain_chunks the largest count of the batch."""
    cc = max(counts)
    return [[f * cc + c for c in range(n)] for f, n in enumerate(counts)]


@pytest.mark.parametrize("frames", [1, 2])
def test_lookback_tags_survive_the_epoch_wrap(hjd, ctx, tuning, frames):
    """The look-back words of ent_chain_lb_kernel carry a 24-bit tag, new per
    launch, and are not cleared between launches; a frame's word row lies at
    f * chain_chunks, so which words a launch rewrites changes with its batch.
    When the tag wraps from 2^24 - 1 to 1, a word written at tag 1 one full
    cycle earlier and not rewritten since carries the current tag again: the
    kernel (ent_chain_lb_kernel, hjd_entropy.hip) would take that stale exit
    slot or map for this launch's and enter a chunk at the wrong slot -- by
    the code wrong coefficients with a clean status, a spurious corrupt status
    or a spurious repair bit (stale slots are real slots, < kChainSlots, so a
    wrong answer, not a wild access).  gdec_issue therefore clears the words
    on the launch that takes the tag back to 1.  The unfixed wrap was never
    run on hardware: that this test would catch it is the reading above.

    X (large) writes every chunk's words at tag 1; the host counter is set to
    2^24 - 2; Z (one chunk) runs at tag 2^24 - 1 and rewrites chunk 0 only; Y1
    is then the launch that wraps to tag 1, over X's words of chunks 1 and up,
    and Y2..Y4 follow at 2, 3, 4 (which reader meets a stale word first depends
    on which chunk gets there first, hence four).  With two frames Y's first
    frame is smaller than X's, so its second frame's row starts inside X's old
    rows.  No Y chunk reads, as a predecessor, a position where X wrote a
    frame's last chunk (whose exit may be none, and would hold a reader that
    took it for this launch's up for good): asserted below, on the CPU."""
    tuning("HJD_SYNC_SPEC", None)   # decoders of one or two frames: speculative by default
    S = 64
    big = dict(w=640, h=480, q=90, sub=2)
    z = [_pil(33, 17, 90, 0, seed=900)]
    if frames == 1:
        x = [_pil(seed=901, **big)]
        ys = [[_pil(seed=902 + k, **big)] for k in range(4)]
    else:
        x = [_pil(seed=911, **big), _pil(seed=912, **big)]
        ys = [[_pil(320, 240, 90, 2, seed=913 + k), _pil(400, 300, 90, 2, seed=923 + k)] for k in range(4)]
    xc = [_chunks(d, S) for d in x]
    assert min(xc) >= 4 and _chunks(z[0], S) == 1
    written_x = {p for row in _rows(xc) for p in row}
    last_x = {row[-1] for row in _rows(xc)}
    for y in ys:
        yc = [_chunks(d, S) for d in y]
        assert all(n <= m for n, m in zip(yc, xc))
        if frames == 1:
            assert yc == xc
        else:
            assert yc[0] < yc[1] < xc[0]   # the second row starts at yc[1], inside X's first row
        read_y = {p for row in _rows(yc) for p in row[:-1]}   # positions read as predecessors
        assert not (read_y & last_x), (xc, yc)
        assert (read_y & written_x) - {0}, "Y reads no word that X wrote and Z left"
    r = _Reused(hjd, ctx, frames, S, [x, z] + ys)
    try:
        st = r.coefs(x, "X")
        assert (st["chain_epoch"], st["batch_spec"], st["batch_lookback"]) == (1, 1, 1), st
        assert st["batch_chain_chunks"] == max(xc) and st["batch_sub_bits"] == S, st
        r.gd.debug_set_chain_epoch(kEpochMax - 1)
        assert r.gd.debug_state()["chain_epoch"] == kEpochMax - 1
        st = r.coefs(z, "Z")
        assert (st["chain_epoch"], st["batch_lookback"], st["batch_chain_chunks"]) == (kEpochMax, 1, 1), st
        for k, y in enumerate(ys):
            st = r.coefs(y, f"Y{k + 1}")
            assert (st["chain_epoch"], st["batch_spec"], st["batch_lookback"]) == (k + 1, 1, 1), st   # Y1: wrapped
            assert st["batch_chain_chunks"] == max(_chunks(d, S) for d in y), st
        # the setter is refused while a call is pending, and then changes nothing
        import torch
        out = torch.full((_ref(z[0])[1].nblocks, 64), 0x5A5A, dtype=torch.int16, device="cuda")
        r.gd.decode_coefs(z, out)
        with pytest.raises(hjd._lib.HjdError) as e:
            r.gd.debug_set_chain_epoch(7)
        assert e.value.code == -5   # HJD_E_STATE
        assert r.gd.sync() == r.control(z, r.gd.debug_state()["batch_lead_bits"])
        assert r.gd.debug_state()["chain_epoch"] == 5
        np.testing.assert_array_equal(out.cpu().numpy(), _ref(z[0])[0])
    finally:
        r.close()


def _wrong_rst(good):
    """The file with a late RSTn replaced by a wrong one: the host destuff
    refuses it ("expected RST"), after the early pull of a lone large scan
    (test_gpu_entropy_spec.py, test_early_pull_and_a_late_destuff_error)."""
    info = _ref(good)[1]
    assert len(good) - info.scan_offset >= 256 << 10   # the early pull's threshold
    at = good.rindex(b"\xff\xd0", 0, len(good) - 64)
    assert at > info.scan_offset + (len(good) - info.scan_offset) * 3 // 4
    return good[:at + 1] + bytes([0xD0 + (good[at + 1] - 0xD0 + 3) % 8]) + good[at + 2:]


def test_one_decoder_mixed_sequence(hjd, ctx, tuning):
    """One three-frame decoder (speculative sync forced, S = 64) through a fixed
    sequence in which consecutive batches differ in frame count (1 <-> 3), in
    size (19 chunks <-> 1), in the sync they take (sparse: speculative; the
    q100 frame, 438 bits per block: round-based at S = 8192), in their Huffman
    tables (default <-> optimize=True and back, which the step tables' cache
    must notice), in restart markers, in scans per file (a two-scan sequential
    file), in sampling (4:2:0, 4:4:4, gray), and in the call (coefficients <->
    pixels); one call fails in host staging after an early pull, and a good
    batch follows it.  Every batch is exact with the control's status."""
    import torch
    tuning("HJD_SYNC_SPEC", 1)
    a = [_pil(640, 480, 90, 2, seed=930 + k) for k in range(4)]
    t1 = _pil(33, 17, 90, 0, seed=940, restart_marker_blocks=1)
    t2 = _pil(17, 9, 90, 2, seed=941)
    tg = _pil(9, 17, 95, 0, seed=942, gray=True)
    gray = _pil(640, 480, 90, 0, seed=943, gray=True)
    dense = _pil(1280, 720, 100, 2, seed=944)
    opt = _pil(640, 480, 75, 2, seed=945, optimize=True)
    rst = _pil(640, 480, 90, 0, seed=946, restart_marker_rows=1)
    base = _pil(320, 240, 90, 2, seed=947)
    two_scans = JW.rewrite_scans(base, hjd.decode_coefs(base)[0], [(0,), (1, 2)], 0)[0]
    scan_src = {two_scans: base}   # (the same coefficients with the same tables: the single-scan file's bits)
    bad_src = _pil(640, 480, 100, 0, seed=948, restart_marker_blocks=8)
    bad = _wrong_rst(bad_src)
    assert 8 * _scan_bytes(dense) > 200 * _ref(dense)[1].nblocks   # kDenseBitsPerBlock (hjd_gdec.hip)
    seq = [
        ("coefs", [a[0]]),                 # one large frame, default tables
        ("pixels", [t1, a[1], gray]),      # three frames: tiny with restarts, large, gray
        ("coefs", [t2]),                   # one chunk
        ("coefs", [dense]),                # round-based
        ("pixels", [a[2], rst, t1]),       # speculative again, restart markers, 4:4:4
        ("coefs", [opt]),                  # other Huffman tables
        ("coefs", [a[0]]),                 # ... and back to the first batch's
        ("pixels", [opt, two_scans, t2]),  # both kinds of tables, a two-scan file
        ("raises", [bad]),                 # fails in host staging, part of it already pulled
        ("coefs", [a[3]]),                 # a good batch after the failure
        ("pixels", [dense]),               # round-based, to pixels
        ("coefs", [two_scans]),            # two entropy frames of one file
        ("pixels", [rst, gray, a[1]]),
        ("coefs", [t1, t2, tg]),           # three tiny frames
        ("pixels", [a[0]]),
        ("coefs", [gray, opt, rst]),
    ]
    r = _Reused(hjd, ctx, 3, 64, [b for _, b in seq])
    seen = []
    try:
        for k, (kind, datas) in enumerate(seq):
            if kind == "raises":
                out = torch.full((_ref(bad_src)[1].nblocks, 64), 0x5A5A, dtype=torch.int16, device="cuda")
                with pytest.raises(hjd._lib.HjdError, match="expected RST"):
                    r.gd.decode_coefs(datas, out)
                continue
            # the sync a batch takes, worked out on the CPU (kDenseBitsPerBlock = 200, hjd_gdec.hip)
            bpb = 8 * sum(_scan_bytes(scan_src.get(d, d)) for d in datas) / sum(_ref(d)[1].nblocks for d in datas)
            assert bpb > 400 if dense in datas else bpb < 190, (k, bpb)
            st = (r.coefs if kind == "coefs" else r.pixels)(datas, f"batch {k} ({kind})")
            seen.append((len(datas), st["batch_spec"], st["batch_lookback"], st["batch_chain_chunks"],
                         st["batch_sub_bits"]))
            if dense in datas:
                assert (st["batch_spec"], st["batch_lookback"], st["batch_sub_bits"]) == (0, 0, 8192), (k, st)
            else:
                assert (st["batch_spec"], st["batch_lookback"], st["batch_sub_bits"]) == (1, 1, 64), (k, st)
                assert st["batch_lead_bits"] in kLeadLadder, (k, st)
    finally:
        r.close()
    assert {s[1] for s in seen} == {0, 1}                       # both syncs ran on the one decoder
    assert {s[0] for s in seen} == {1, 3}
    assert min(s[3] for s in seen) == 1 and max(s[3] for s in seen if s[1]) >= 16   # one chunk <-> many


def test_failed_roi_call_leaves_nothing_behind(hjd, ctx):
    """What belongs to one call (its rectangles, its outputs, its early-pull
    bookkeeping) travels in the call's descriptor (GdecCall), not on the
    decoder: a ROI call that fails in staging (a) and one refused before
    staging (b) leave nothing that the next calls could pick up.  (c) a plain
    decode of whole frames into tensors with a guard row, then (d) a ROI
    decode, both exact against the oracle, on the one two-frame decoder."""
    import torch
    f420 = _pil(48, 32, 90, 2, seed=960)
    f444 = _pil(40, 24, 90, 0, seed=961)
    datas = [f420, f444]
    infos = [_ref(d)[1] for d in datas]
    assert [(i.width, i.height, i.sampling) for i in infos] == [(48, 32, hjd.YUV420), (40, 24, hjd.YUV444)]
    sos = f444.index(b"\xff\xda")
    assert sos + 4 < infos[1].scan_offset
    cut = f444[:sos + 4]   # inside the SOS header: no pre-check reads it, staging refuses it
    rois = [(8, 4, 24, 16), (3, 5, 28, 12)]

    def roi_outs():
        return [torch.full((r[3], r[2]), -1, dtype=torch.int32, device="cuda") for r in rois]

    with hjd.GpuDecoder(ctx, 2, 2 * sum(map(len, datas)), 2 * sum(i.nblocks for i in infos)) as gd:
        with pytest.raises(hjd._lib.HjdError):                        # (a)
            gd.decode([f420, cut], roi_outs(), rois=rois)
        with pytest.raises(hjd._lib.HjdError, match="frame 0: roi") as e:   # (b)
            gd.decode(datas, roi_outs(), rois=[(40, 0, 16, 8), rois[1]])   # 56 px wide
        assert e.value.code == -1
        guarded = [torch.full((i.height + 1, i.width), -1, dtype=torch.int32, device="cuda") for i in infos]
        gd.decode(datas, [g[:i.height] for g, i in zip(guarded, infos)])   # (c)
        assert gd.sync() == [0, 0]
        for k, (d, g, i) in enumerate(zip(datas, guarded, infos)):
            host = g.cpu().numpy()
            np.testing.assert_array_equal(host[:i.height].view(np.uint32), _ref_pixels(d), err_msg=f"(c) file {k}")
            assert (host[i.height] == -1).all(), f"(c) file {k}: guard row written"
        outs = roi_outs()
        gd.decode(datas, outs, rois=rois)                             # (d)
        assert gd.sync() == [0, 0]
        for k, (d, o, (x, y, w, h)) in enumerate(zip(datas, outs, rois)):
            np.testing.assert_array_equal(o.cpu().numpy().view(np.uint32), _ref_pixels(d)[y:y + h, x:x + w],
                                          err_msg=f"(d) file {k}")


def test_lead_ladder_walks_down_and_doubles_its_hold(hjd, ctx, tuning):
    """The lead-in ladder of hjd_gdec_sync ("the lead-in of the next batches",
    hjd_gdec.hip) on a one-frame decoder at its default S (512):
    kLeadLadder = {512, 1536, 2560}, kLeadBatches = 32.  B (320x240 q90 4:4:4
    seed 0) needs a repair at a lead-in of 512 bits and none at 1536; C (seed 1)
    is clean at both (pinned on the CPU, test_entropy_emulation_spec.py).
    B steps up with 32 clean batches to wait; 31 x C count them down; the 32nd
    steps down; a repair right after a step down doubles the hold to 64; 64 x C
    step down again.  A dense batch (round-based sync) in between leaves the
    ladder alone.  The state is asserted after every sync, the status bit
    recorded on every call, coefficients compared on the transitions and
    every 8th call."""
    tuning("HJD_SYNC_SPEC", None)
    tuning("HJD_SPEC_LEAD", None)
    B = _pil(320, 240, 90, 0, seed=0)
    C = _pil(320, 240, 90, 0, seed=1)
    D = _pil(320, 240, 100, 2, seed=2)   # 441 bits per block: round-based
    assert 8 * _scan_bytes(D) > 200 * _ref(D)[1].nblocks
    r = _Reused(hjd, ctx, 1, 0, [[B], [C], [D]])
    calls = [0]

    def ladder(st):
        return st["lead_step"], st["lead_left"], st["lead_hold"], st["lead_stepped_down"]

    def run(d, step_before, expect, what, compare=False):
        calls[0] += 1
        st = r.coefs([d], what, compare=compare or calls[0] % 8 == 0)
        assert (st["batch_spec"], st["batch_lookback"], st["batch_sub_bits"]) == (1, 1, 512), (what, st)
        assert st["batch_lead_bits"] == kLeadLadder[step_before], (what, st)
        assert r.bits[-1] == [1 if d is B else 0], (what, r.bits[-1])
        assert ladder(st) == expect, (what, st)

    try:
        assert ladder(r.gd.debug_state()) == (0, 0, kLeadBatches, 0)
        run(B, 0, (1, 32, 32, 0), "B", compare=True)
        for k in range(1, 32):
            run(C, 1, (1, 32 - k, 32, 0), f"C {k}", compare=k == 1)
            if k == 10:   # a dense batch does not touch the ladder
                st = r.coefs([D], "dense")
                assert (st["batch_spec"], st["batch_lookback"], st["batch_lead_bits"]) == (0, 0, 0), st
                assert st["batch_sub_bits"] == 8192, st   # kDenseTiers' last (hjd_gdec.hip)
                assert ladder(st) == (1, 32 - k, 32, 0), st
        run(C, 1, (0, 0, 32, 1), "C 32", compare=True)
        run(B, 0, (1, 64, 64, 0), "B after the step down", compare=True)
        for k in range(1, 64):
            run(C, 1, (1, 64 - k, 64, 0), f"C' {k}", compare=k == 1)
        run(C, 1, (0, 0, 64, 1), "C' 64", compare=True)
        run(C, 0, (0, 0, 64, 0), "C at the bottom", compare=True)
    finally:
        r.close()
    assert len(r.bits) == 1 + 31 + 1 + 1 + 1 + 64 + 1
